#!/usr/bin/env python3
"""What deriving the crystal-system labels costs (symmetry.crystal_systems, csrc/symmetry.hip), next to the numpy twin.  Report
only - not an acceptance bar; featurisation runs once per dataset, off the training step.

Two datasets of 4096 crystals: ``synth.edos_structures`` (random triclinic cells of 2-40 atoms: two lattice operations, hardly any
structure search) and the known-answer crystals of tests/symmetry_cases.py in all their forms, tiled (up to 48 lattice operations,
supercells with translations).  Per dataset:

* the two launches alone, inputs already on the device: medians of event-timed calls after a warm-up (dosx_sym_translations, then
  dosx_sym_point_group on the reduced primitive cells);
* the whole call ``crystal_systems(entries)`` on the host clock: entry parsing, the two Delaunay reductions per crystal and the
  primitive lattices in numpy, uploads, the two launches, read-back;
* the numpy twin: its two kernels' twins alone, and the whole ``crystal_systems_host(entries, margin=False)`` (early exits on).

usage: python tools/bench_symmetry.py [--crystals C] [--reps R] [--log PATH]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dostransformer_amd import ops, symmetry, synth  # noqa: E402
from tests import symmetry_cases as sc  # noqa: E402


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
    best = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        best.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(best), out


def case(name, entries, reps, dev, say):
    C = len(entries)
    whole_dev, rep = host_ms(lambda: symmetry.crystal_systems(entries, device=dev), 3)
    whole_host, ref = host_ms(lambda: symmetry.crystal_systems_host(entries, margin=False))
    same = all(torch.equal(getattr(rep, k), getattr(ref, k)) for k in ("system", "n_ops", "n_lattice_ops", "n_translations", "ops"))
    # the launches alone, on the inputs the call above gave them
    cells, pos, species, ptr = symmetry._prepare(entries)
    frac = symmetry._fractional(cells, pos)
    prim_frac = symmetry._fractional(rep.cells, pos)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    n = np.diff(ptr)
    kw = dict(n_min=int(n.min()), n_max=int(n.max()))
    a1, a2 = (up(cells), up(frac), up(species), up(ptr)), (up(rep.cells), up(prim_frac), up(species), up(ptr))
    t_tr = event_median(lambda: ops.sym_translations(*a1, 0.1, **kw), reps)
    t_pg = event_median(lambda: ops.sym_point_group(*a2, 0.1, **kw), reps)
    h_tr, _ = host_ms(lambda: symmetry.translations_host(cells, frac, species, ptr, 0.1))
    h_pg, _ = host_ms(lambda: symmetry.point_group_host(rep.cells, prim_frac, species, ptr, 0.1, margin=False))
    say(f"{name}: C={C} atoms={int(ptr[-1])} (largest {int(n.max())}), {int((rep.n_translations > 0).sum())} with translations, "
        f"systems {np.bincount(rep.system.numpy(), minlength=8).tolist()}, kernel == twin: {same}")
    say(f"  launches  translations {t_tr[0]:8.3f} ms (min {t_tr[1]:.3f} max {t_tr[2]:.3f}) | point group {t_pg[0]:8.3f} ms "
        f"(min {t_pg[1]:.3f} max {t_pg[2]:.3f}) | twin {h_tr:9.1f} ms + {h_pg:9.1f} ms = x{(h_tr + h_pg) / (t_tr[0] + t_pg[0]):.0f}")
    say(f"  whole call crystal_systems {whole_dev:9.1f} ms | crystal_systems_host {whole_host:9.1f} ms = x{whole_host / whole_dev:.1f} "
        f"(host share of the device call: {whole_dev - t_tr[0] - t_pg[0]:.1f} ms)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--crystals", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "symmetry_bench.log"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as log:
        def say(line):
            print(line, flush=True)
            log.write(line + "\n")
        say(f"bench_symmetry: {torch.cuda.get_device_name(0)}, symprec 0.1, {args.reps} event-timed calls per launch after 3 warm-ups")
        case("synth.edos_structures", synth.edos_structures(args.crystals, 0), args.reps, dev, say)
        forms = [f[1] for f in sc.all_forms()]
        case("known answers, tiled", [forms[i % len(forms)] for i in range(args.crystals)], args.reps, dev, say)


if __name__ == "__main__":
    main()
