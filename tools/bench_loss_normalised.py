#!/usr/bin/env python3
"""What normalised functionals in the per-crystal losses cost (dosx_loss_rows_fn_norm, csrc/loss_functional.hip).
Report only - not an acceptance bar: this is not a speed feature.

* the launch alone: ``dosx_loss_rows_fn_norm_desc`` (RMSE kind, two outputs with per_crystal - the trainers' form, two launches
  per call) with every row of a cumulative table normalised, SQ and ABS, at (B, S, K) = (64, 51, 1), (64, 201, 1), (64, 51, 50)
  and (64, 201, 200), next to ``dosx_loss_rows_fn`` with the SAME table and K.  Every side is a recorded program of ``--iters``
  calls back to back, replayed from C and timed with device events; the sides alternate in rounds; best, median and spread per
  side.  A normalised row has three wave reductions where a plain row has two: about 3/2 of the linear entry's per-k cost is
  expected on the rows, and its cost at K = 1;
* the replayed training step of Phonon-DOS L3 T2 H128 B64 and Electron-DOS L3 T2 H256 B64 with ``loss="crystal_rmse"``, without a
  term, with the plain cumulative term and with centre + normalised cumulative, the trainers alternating in rounds.

Not timed here: the float64 entries, the one-workgroup form (per_crystal == NULL), the other three pointwise kinds, mixed tables,
the literal entries (the same kernels as their descriptor forms), and the parent commit's own library in a process of its own.

usage: python tools/bench_loss_normalised.py [--iters N] [--rounds R]"""
import argparse
import os
import sys

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.dirname(os.path.abspath(__file__))]
import torch  # noqa: E402
from bench_loss_functional import _workload, spread, timeit  # noqa: E402   (tools/bench_loss_functional.py: the same workloads)
from dostransformer_amd import functionals, ops  # noqa: E402
from dostransformer_amd.train import Trainer  # noqa: E402

SHAPES = ((64, 51, 1), (64, 201, 1), (64, 51, 50), (64, 201, 200))


def launch_sides(B, S, K):
    gen = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *s: torch.rand(*s, device="cuda", generator=gen)
    y = r(B, S)
    pg, ps = y + 0.1 * r(B, S), y + 0.1 * r(B, S)
    dpg, dps, per, loss = (torch.empty(*s, device="cuda") for s in ((B, S), (B, S), (B,), (1,)))
    kw = dict(clamp_target=True, beta=1.0, dpg=dpg, dps=dps, per_crystal=per, loss=loss)
    # the cumulative DOS at K evenly spaced bins below the last one, over the total
    rows = torch.linspace(0, S - 2, K).round().long()
    cdf = functionals.cumulative(S, 1.0 / S).table
    tab, den = cdf[rows].float().cuda().contiguous(), cdf[S - 1].float().cuda().contiguous()
    lin = lambda kind: (lambda: ops.loss_rows(pg, ps, y, "crystal_rmse", functionals=tab, functional_kind=kind,
                                              functional_weight=0.5, **kw))
    nrm = lambda kind: (lambda: ops.loss_rows(pg, ps, y, "crystal_rmse", functionals=tab, functional_kind=kind, functional_weight=0.5,
                                              functional_denominator=den, functional_norm_rows=K, functional_floor=1e-3, **kw))
    return {"loss_rows": lambda: ops.loss_rows(pg, ps, y, "crystal_rmse", **kw),
            "loss_rows_fn sq": lin("sq"), "loss_rows_fn_norm sq": nrm("sq"),
            "loss_rows_fn abs": lin("abs"), "loss_rows_fn_norm abs": nrm("abs")}


def report_launches(B, S, K, reps, rounds):
    progs = {}
    for key, f in launch_sides(B, S, K).items():
        with ops.recording_scope():
            ops.RECORDER.begin()
            for _ in range(reps):
                f()
            progs[key] = ops.RECORDER.end()
    us = {k: [] for k in progs}
    for _ in range(rounds):
        for k, p in progs.items():
            us[k].append(1e3 * timeit(p.run, 5, warm=1) / reps)
    print(f"launches alone B{B} S{S} K{K} ({reps} calls back to back, {rounds} alternated rounds, us per call):")
    for k, v in us.items():
        print(f"    {k:22s}: {spread(v)}")
    plain = min(us["loss_rows"])
    for kind in ("sq", "abs"):
        a, b = us[f"loss_rows_fn {kind}"], us[f"loss_rows_fn_norm {kind}"]
        over = min(a) - plain                  # the rows' cost; a ratio of two of them means something only above the rounds' spread
        ratio = f"ratio {(min(b) - plain) / over:.2f}" if over > 2.0 * (max(a) - min(a)) and over > 1.0 else "ratio n/a (inside the spread)"
        print(f"    normalised - linear, {kind}, best - best: {min(b) - min(a):+.2f} us; over loss_rows: linear {over:+.2f} us, "
              f"normalised {min(b) - plain:+.2f} us, {ratio} (spread of the linear side's rounds {max(a) - min(a):.2f} us)")


def step_case(kind, L, T, H, B, iters, rounds):
    trainers = []
    for name in ("crystal_rmse", "+ cumulative sq", "+ centre, ncdf sq", "+ centre, ncdf abs"):
        model, g = _workload(kind, L, T, H, B)
        S = int(model._cfg.S)
        e = (torch.arange(S, dtype=torch.float64) + 0.5) / S
        fn = {"crystal_rmse": None, "+ cumulative sq": functionals.cumulative(S, 1.0 / S)}.get(
            name, functionals.stack(functionals.centre(e, 1e-3, de=1.0 / S), functionals.normalised_cumulative(S, 1e-3, 1.0 / S)))
        kw = {} if fn is None else dict(functionals=fn, functional_kind=name.split()[-1], functional_weight=0.5)
        trainers.append((name, Trainer(model, replay=True, loss="crystal_rmse", **kw), g))
    ms = {name: [] for name, _, _ in trainers}
    for _ in range(rounds):
        for name, tr, g in trainers:
            ms[name].append(timeit(lambda: tr.step(g), iters))
    for name in ms:
        print(f"step {kind} L{L} T{T} H{H} B{B} {name:20s}: " + " ".join(f"{v:7.4f}" for v in ms[name]) +
              f" ms  best {min(ms[name]):7.4f} median {sorted(ms[name])[len(ms[name]) // 2]:7.4f} ms")
    a = min(ms["crystal_rmse"])
    for name in list(ms)[1:]:
        b = min(ms[name])
        print(f"     {name} / crystal_rmse (best of {rounds}): {b / a:.4f} ({1e3 * (b - a):+.1f} us); spread of the plain "
              f"trainer's rounds {1e3 * (max(ms['crystal_rmse']) - a):.1f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert args.rounds >= 3
    print(f"device: {torch.cuda.get_device_name(0)}")
    for B, S, K in SHAPES:
        report_launches(B, S, K, args.iters, args.rounds)
    step_case("phonon", 3, 2, 128, 64, args.iters, args.rounds)
    step_case("edos", 3, 2, 256, 64, args.iters, args.rounds)


if __name__ == "__main__":
    main()
