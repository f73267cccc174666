#!/usr/bin/env python3
"""Timing of the fp32 training step behind the gradient guard (Trainer(max_grad_norm=..., skip_nonfinite=True), replay) next to the
same step without it, in one process.  Report only - not an acceptance bar.

* cfg2: DOSTransformer_phonon L3 T2 H128, 64 crystals (the headline shape);
* an Electron-DOS batch: DOSTransformer L3 T2 H256, 64 crystals.

The guard adds one statistics launch over the flat gradient and swaps the AdamW kernel for the one that reads its verdict; the
max_grad_norm used here (1e30) never clips, so both trainers walk the same trajectory.  The two trainers alternate in rounds so
that a drift of the clocks shows in both columns.  Last, the optimizer's launches alone at the two flat sizes, replayed back to
back from C: the device time the guard adds, without the host's share.

usage: python tools/bench_step_guard.py [--iters N] [--rounds R]"""
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


def case(name, kind, L, T, H, B, iters, rounds):
    trainers = []
    for guard in (False, True):
        torch.manual_seed(0)
        if kind == "phonon":
            from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
            model = DOSTransformer_phonon(L, T, 118, 4, H, "cuda", 0.0).to("cuda")
            g = synth.phonon_batch(B, seed=1, dtype=torch.float32).to("cuda")
        else:
            from dostransformer_amd.embedder_eDOS.DOSTransformer import DOSTransformer
            model = DOSTransformer(L, T, 200, 41, 2, H, "cuda", 0.0).to("cuda")
            g = synth.edos_batch(B, seed=1, dtype=torch.float32).to("cuda")
        kw = {"max_grad_norm": 1e30, "skip_nonfinite": True} if guard else {}
        trainers.append((guard, Trainer(model, replay=True, **kw), g))
    ms = {False: [], True: []}
    for _ in range(rounds):
        for guard, tr, g in trainers:
            ms[guard].append(timeit(lambda: tr.step(g), iters))
    for guard in (False, True):
        best, med = min(ms[guard]), sorted(ms[guard])[len(ms[guard]) // 2]
        print(f"step {name} {kind} L{L} T{T} H{H} B{B} guard={str(guard):5s}: " + " ".join(f"{v:7.4f}" for v in ms[guard]) +
              f" ms  best {best:7.4f} median {med:7.4f} ms ({B / (best * 1e-3):8.0f} crystals/s)")
    rep = trainers[1][1].guard_report()
    total = trainers[1][1]._fp.total
    print(f"     {total} flat parameters ({4 * total / 1e6:.2f} MB of gradient); guard record: {rep.applied} applied, {rep.skipped} skipped, "
          f"norm {rep.norm:.4g}; guarded / unguarded (best of {rounds}): {min(ms[True]) / min(ms[False]):.4f} "
          f"(+{1e3 * (min(ms[True]) - min(ms[False])):.1f} us)")


def launches_alone(name, n, reps, rounds):
    """The optimizer's launches alone on flat buffers of n floats: `reps` of them recorded and replayed back to back from C
    (ops.Program), so the figure is device time and not the host's cost of issuing them."""
    gen = torch.Generator(device="cuda").manual_seed(0)
    p, g, m, v = (torch.randn(n, device="cuda", generator=gen) for _ in range(4))
    v.abs_()
    rec, ws = ops.guard_buffers("cuda")
    status = ops.exchange_status_address("cuda")
    hyper = (1e-4, 0.9, 0.999)

    def plain():
        ops.adamw(p, g, m, v, n, *hyper, 1e-8, 1e-2, 1, 1.0)

    def guarded():
        ops.grad_guard(g, n, rec, ws, 1e30, *hyper, 1, status)
        ops.adamw_guarded(p, g, m, v, n, *hyper, 1e-8, 1e-2, rec)

    progs = {}
    for key, fn in (("adamw", plain), ("grad_guard + adamw_guarded", guarded)):
        with ops.recording_scope():
            ops.RECORDER.begin()
            for _ in range(reps):
                fn()
            progs[key] = ops.RECORDER.end()
    us = {k: [] for k in progs}
    for _ in range(rounds):
        for k, prog in progs.items():
            us[k].append(1e3 * timeit(prog.run, 5, warm=1) / reps)
    a, b = min(us["adamw"]), min(us["grad_guard + adamw_guarded"])
    print(f"launches alone {name} ({n} floats, {reps} back to back, best of {rounds}): adamw {a:.2f} us, grad_guard + adamw_guarded "
          f"{b:.2f} us (+{b - a:.2f} us)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name(0)}")
    case("cfg2", "phonon", 3, 2, 128, 64, args.iters, args.rounds)
    case("edos", "edos", 3, 2, 256, 64, args.iters, args.rounds)
    launches_alone("cfg2", 1634688, args.iters, args.rounds)
    launches_alone("edos", 6664704, args.iters, args.rounds)


if __name__ == "__main__":
    main()
