#!/usr/bin/env python3
"""Timing of the fp32 training step with per-crystal keys (Trainer(per_crystal_keys=True), replay) next to the same step without
the flag, in one process.  Report only - not an acceptance bar.

* cfg2: DOSTransformer_phonon L3 T2 H128, 64 crystals (the headline shape; n_max 12: every crystal is one 16-key tile);
* an Electron-DOS batch: DOSTransformer L3 T2 H256, 64 crystals (41 key rows: the rows past a crystal's own atoms are idle).

The two trainers alternate in rounds so that a drift of the clocks shows in both columns.

usage: python tools/bench_per_crystal.py [--iters N] [--rounds R]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dostransformer_amd import synth  # noqa: E402
from dostransformer_amd.train import Trainer  # noqa: E402


def timeit(fn, iters, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters     # ms


def case(name, kind, L, T, H, B, iters, rounds):
    trainers = []
    for flag in (False, True):
        torch.manual_seed(0)
        if kind == "phonon":
            from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
            model = DOSTransformer_phonon(L, T, 118, 4, H, "cuda", 0.0).to("cuda")
            g = synth.phonon_batch(B, seed=1, dtype=torch.float32).to("cuda")
        else:
            from dostransformer_amd.embedder_eDOS.DOSTransformer import DOSTransformer
            model = DOSTransformer(L, T, 200, 41, 2, H, "cuda", 0.0).to("cuda")
            g = synth.edos_batch(B, seed=1, dtype=torch.float32).to("cuda")
        trainers.append((flag, Trainer(model, replay=True, per_crystal_keys=flag), g))
    counts = torch.bincount(trainers[0][2].batch)
    ms = {False: [], True: []}
    for _ in range(rounds):
        for flag, tr, g in trainers:
            ms[flag].append(timeit(lambda: tr.step(g), iters))
    for flag in (False, True):
        best = min(ms[flag])
        print(f"step {name} {kind} L{L} T{T} H{H} B{B} per_crystal_keys={str(flag):5s}: " +
              " ".join(f"{v:7.4f}" for v in ms[flag]) + f" ms  best {best:7.4f} ms ({B / (best * 1e-3):8.0f} crystals/s)")
    print(f"     atoms per crystal: min {int(counts.min())} mean {float(counts.float().mean()):.1f} max {int(counts.max())}; "
          f"flagged / unflagged (best of {rounds}): {min(ms[True]) / min(ms[False]):.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name(0)}")
    case("cfg2", "phonon", 3, 2, 128, 64, args.iters, args.rounds)
    case("edos", "edos", 3, 2, 256, 64, args.iters, args.rounds)


if __name__ == "__main__":
    main()
