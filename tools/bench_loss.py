#!/usr/bin/env python3
"""What the per-crystal losses (Trainer(loss=...), csrc/loss_rows.hip) cost, in one process.  Report only - not an acceptance
bar: this is not a speed feature.

* the launch alone: ``dosx_loss_rows`` for each kind at (B, S) = (64, 51), (512, 51), (64, 201), two outputs with per_crystal
  (the trainers' form: two launches per call), next to the entries it replaces - ``dosx_loss_phonon`` (one workgroup) and
  ``dosx_loss_edos`` + ``dosx_sum``.  Every side is a recorded program of ``--iters`` calls back to back, replayed from C and
  timed with device events; the sides alternate in rounds and the spread between the rounds of one side is printed.  The RMSE
  kind repeats the eDOS pair's arithmetic: at (64, 201) it should cost what the pair costs, within that spread;
* the replayed training step of Phonon-DOS L3 T2 H128 B64 and Electron-DOS L3 T2 H256 B64 with ``loss="crystal_rmse"`` against
  the default, the two trainers alternating in rounds.

usage: python tools/bench_loss.py [--iters N] [--rounds R]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dostransformer_amd import ops, synth  # noqa: E402
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


def spread(v):
    return f"best {min(v):6.2f} median {sorted(v)[len(v) // 2]:6.2f} worst {max(v):6.2f} (spread {max(v) - min(v):5.2f})"


def launches_alone(B, S, reps, rounds):
    gen = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *s: torch.randn(*s, device="cuda", generator=gen)
    y = r(B, S) * 0.8
    pg, ps = y.clamp(min=0) + 0.1 * r(B, S), y.clamp(min=0) + 0.1 * r(B, S)
    dpg, dps, per, lp, loss, sse = (torch.empty(*s, device="cuda") for s in ((B, S), (B, S), (B,), (B + 1,), (1,), (2,)))
    sides = {"loss_phonon": lambda: ops.loss_phonon(pg, ps, y, sse, 1.0, dpg, dps, loss, B * S),
             "loss_edos + sum": lambda: (ops.loss_edos(pg, ps, y, 1.0, B, S, B, dpg, dps, lp), ops.sum_to(lp, B, lp[B:]))}
    for kind in ops.LOSS_KINDS:
        sides[f"loss_rows {kind}"] = (lambda k: lambda: ops.loss_rows(pg, ps, y, k, clamp_target=True, beta=1.0, delta=0.05, dpg=dpg,
                                                                       dps=dps, per_crystal=per, loss=loss))(kind)
    progs = {}
    for key, fn in sides.items():
        with ops.recording_scope():
            ops.RECORDER.begin()
            for _ in range(reps):
                fn()
            progs[key] = ops.RECORDER.end()
    us = {k: [] for k in progs}
    for _ in range(rounds):
        for k, p in progs.items():
            us[k].append(1e3 * timeit(p.run, 5, warm=1) / reps)
    print(f"launches alone B{B} S{S} ({reps} calls back to back, {rounds} alternated rounds, us per call):")
    for k in progs:
        print(f"    {k:22s}: {spread(us[k])}")
    pair, rm = us["loss_edos + sum"], us["loss_rows crystal_rmse"]
    print(f"    loss_rows crystal_rmse - (loss_edos + sum), best - best: {min(rm) - min(pair):+.2f} us; spread of the pair's rounds "
          f"{max(pair) - min(pair):.2f} us, of loss_rows' {max(rm) - min(rm):.2f} us")


def _workload(kind, L, T, H, B):
    torch.manual_seed(0)
    if kind == "phonon":
        from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
        return (DOSTransformer_phonon(L, T, 118, 4, H, "cuda", 0.0).to("cuda"),
                synth.phonon_batch(B, seed=1, dtype=torch.float32).to("cuda"))
    from dostransformer_amd.embedder_eDOS.DOSTransformer import DOSTransformer
    return DOSTransformer(L, T, 200, 41, 2, H, "cuda", 0.0).to("cuda"), synth.edos_batch(B, seed=1, dtype=torch.float32).to("cuda")


def step_case(kind, L, T, H, B, iters, rounds):
    trainers = []
    for loss in (None, "crystal_rmse"):
        model, g = _workload(kind, L, T, H, B)
        trainers.append((loss, Trainer(model, replay=True, loss=loss), g))
    ms = {None: [], "crystal_rmse": []}
    for _ in range(rounds):
        for loss, tr, g in trainers:
            ms[loss].append(timeit(lambda: tr.step(g), iters))
    for loss in ms:
        print(f"step {kind} L{L} T{T} H{H} B{B} loss={str(loss):12s}: " + " ".join(f"{v:7.4f}" for v in ms[loss]) +
              f" ms  best {min(ms[loss]):7.4f} median {sorted(ms[loss])[len(ms[loss]) // 2]:7.4f} ms "
              f"({B / (min(ms[loss]) * 1e-3):8.0f} crystals/s)")
    a, b = min(ms[None]), min(ms["crystal_rmse"])
    print(f"     crystal_rmse / default (best of {rounds}): {b / a:.4f} ({1e3 * (b - a):+.1f} us); spread of the default's rounds "
          f"{1e3 * (max(ms[None]) - a):.1f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert args.rounds >= 3
    print(f"device: {torch.cuda.get_device_name(0)}")
    for B, S in ((64, 51), (512, 51), (64, 201)):
        launches_alone(B, S, args.iters, args.rounds)
    step_case("phonon", 3, 2, 128, 64, args.iters, args.rounds)
    step_case("edos", 3, 2, 256, 64, args.iters, args.rounds)


if __name__ == "__main__":
    main()
