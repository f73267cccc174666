"""Times spectra.broaden and spectra.resample for a whole dataset against the numpy twin on the same host - the once-per-dataset cost
of building DOS targets from raw spectra.

The dataset: C crystals, each a tabulated curve of n sorted samples on a grid of its own (from 11-14 below to 9-12 above its own
Fermi level), broadened by sigma = 0.3 onto S bins between -8 and 6 relative to the Fermi level.  Per call:

* the launch alone, inputs already on the device: median of event-timed calls after a warm-up;
* the whole call on the host clock: flattening the lists, uploads, the launch, the report's read-back;
* the numpy twin in its fastest honest form - ``broaden_rows_host(vectorized=True)``: per crystal one [n, S] term matrix, summed by
  numpy - and ``interp_rows_host`` (a ``searchsorted`` per crystal); with ``--twin-crystals K`` on the first K crystals only,
  scaled to C (the twin's cost is linear in the crystals; the log shows both figures and the factor).

What is not timed: reading the spectra from disk, and the ordered twin the tests compare with (a Python loop over the samples).

usage: python tools/bench_spectra.py [--crystals C] [--samples N] [--bins S] [--twin-crystals K] [--reps R] [--log PATH]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dostransformer_amd import ops, spectra  # noqa: E402


def event_median(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ms.append(s.elapsed_time(e))
    return statistics.median(ms), min(ms), max(ms)


def host_ms(fn, reps=1):
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), out


def dataset(C, n, seed=0):
    rng = np.random.default_rng(seed)
    es, vs, ef = [], [], []
    for _ in range(C):
        f = float(rng.uniform(-3.0, 7.0))
        e = np.linspace(f - rng.uniform(11.0, 14.0), f + rng.uniform(9.0, 12.0), n)
        es.append(e)
        vs.append(sum(a * np.exp(-((e - f - c) / w) ** 2) for a, c, w in
                      zip(rng.uniform(0.5, 4.0, 6), rng.uniform(-10.0, 8.0, 6), rng.uniform(0.05, 1.2, 6))))
        ef.append(f)
    return es, vs, np.array(ef)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crystals", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=2000)
    ap.add_argument("--bins", type=int, default=201)
    ap.add_argument("--twin-crystals", type=int, default=None)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "spectra_bench.log"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    C, n, S = args.crystals, args.samples, args.bins
    K = C if args.twin_crystals is None else min(args.twin_crystals, C)
    grid, sigma = spectra.Grid.linspace(-8.0, 6.0, S), 0.3
    es, vs, ef = dataset(C, n)
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as log:
        def say(line):
            print(line, flush=True)
            log.write(line + "\n")
        say(f"bench_spectra: {torch.cuda.get_device_name(0)}, C={C} curves of n={n} sorted samples, S={S} bins, sigma {sigma}, "
            f"cutoff 6, {args.reps} event-timed calls per launch after 3 warm-ups")
        ptr, e, v = spectra._flatten(es, vs, None, "curve")
        sg = np.full(C, sigma)
        up = lambda a: torch.from_numpy(a).to(dev)
        d = [up(a) for a in (ptr, e, v, ef, sg)]
        t_b = event_median(lambda: ops.spectra_broaden(*d, grid.e0, grid.de, S, n, n, cutoff=6.0, normalize=True), args.reps)
        t_i = event_median(lambda: ops.spectra_interp(*d[:4], grid.e0, grid.de, S, n, n, normalize=True), args.reps)
        w_b, res_b = host_ms(lambda: spectra.broaden(es, vs, grid, sigma, shift=ef, normalize=True, device=dev), 3)
        w_i, res_i = host_ms(lambda: spectra.resample(es, vs, grid, shift=ef, normalize=True, device=dev), 3)
        sub = (ptr[:K + 1], e[:ptr[K]], v[:ptr[K]], ef[:K])
        h_b, twin_b = host_ms(lambda: spectra.broaden_rows_host(*sub, sg[:K], grid, 6.0, "curve", normalize=True, vectorized=True))
        h_i, twin_i = host_ms(lambda: spectra.interp_rows_host(*sub, grid, normalize=True))
        err_b = float(np.abs(res_b.y[:K].cpu().numpy() - twin_b[0]).max() / np.abs(twin_b[0]).max())
        same_i = bool(np.array_equal(res_i.y[:K].cpu().numpy(), twin_i[0]))
        scale = C / K
        say(f"  broaden   launch {t_b[0]:9.3f} ms (min {t_b[1]:.3f} max {t_b[2]:.3f}) | whole call {w_b:9.1f} ms | twin, vectorized, "
            f"{K} crystals {h_b:9.1f} ms -> x{scale:g} = {h_b * scale:9.1f} ms for {C} | twin / whole call x{h_b * scale / w_b:.0f}, "
            f"twin / launch x{h_b * scale / t_b[0]:.0f} | largest |gpu - twin| / max |twin| {err_b:.1e}")
        say(f"  resample  launch {t_i[0]:9.3f} ms (min {t_i[1]:.3f} max {t_i[2]:.3f}) | whole call {w_i:9.1f} ms | twin, "
            f"{K} crystals {h_i:9.1f} ms -> x{scale:g} = {h_i * scale:9.1f} ms for {C} | twin / whole call x{h_i * scale / w_i:.1f}, "
            f"twin / launch x{h_i * scale / t_i[0]:.0f} | gpu == twin bitwise: {same_i}")
        say(f"  report    covered {int(res_b.report.covered.sum())}/{C}, refused {int(res_b.report.refused.sum())}, samples inside "
            f"the widened window {int(res_b.report.n_inside.sum())} of {C * n}")
        say("  not timed: reading spectra from disk; the ordered twin of the tests (a Python loop over the samples)")


if __name__ == "__main__":
    main()
