#!/usr/bin/env python3
"""What gradient accumulation (Trainer.step_accumulate, csrc/grad_accumulate.hip) costs, in one process.  Report only - not a speed
feature and not an acceptance bar.  By bytes the accumulate launch moves 12 B (fp32) / 24 B (float64) per element (8 / 16 for
the copy that opens a window) against AdamW's 28 / 56; the expectation for a window of K micro-batches is the sum of its K plain
steps minus K - 1 AdamW launches plus K accumulate launches.

* the launch alone, fp32 and float64, at the two flat sizes - Phonon-DOS L3 T2 H128 (1634688 elements) and Electron-DOS L3 T2 H256
  (6664704): copy and add forms replayed back to back from C (device time), next to ``torch.add(a, b, out=dst)`` of the same size
  replayed from a captured graph of as many launches, for scale;
* a replayed window of 4 x 16 crystals against 4 plain replayed steps of 16 and against one replayed step of the 64 - Phonon-DOS
  H128 with ``loss="crystal_rmse"`` and Electron-DOS H256 with its default loss; the three alternate in rounds, so that a drift
  of the clocks shows in every column.

usage: python tools/bench_accumulate.py [--iters N] [--rounds R]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dostransformer_amd import ops, synth  # noqa: E402
from dostransformer_amd.batch import collate  # noqa: E402
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
    return f"best {min(v):.2f} median {sorted(v)[len(v) // 2]:.2f} worst {max(v):.2f}"


def launches_alone(name, n, reps, rounds):
    for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        gen = torch.Generator(device="cuda").manual_seed(0)
        dst, a, b = (torch.randn(n, device="cuda", generator=gen, dtype=dtype) * 1e-3 for _ in range(3))
        sd, sa = torch.zeros(1, device="cuda", dtype=dtype), torch.ones(1, device="cuda", dtype=dtype)
        acc = ops.grad_accumulate if dtype == torch.float32 else ops.grad_accumulate64
        forms = {"copy": lambda: acc(dst, a, None, n, sdst=sd, sa=sa), "add": lambda: acc(dst, a, b, n, sdst=sd, sa=sd, sb=sa),
                 "add in place": lambda: acc(b, a, b, n, sdst=sd, sa=sd, sb=sa)}
        runs = {}
        for key, fn in forms.items():
            with ops.recording_scope():
                ops.RECORDER.begin()
                for _ in range(reps):
                    fn()
                runs[key] = ops.RECORDER.end().run
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            torch.add(a, b, out=dst)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(reps):
                torch.add(a, b, out=dst)
        runs["torch.add(out=)"] = graph.replay
        us = {k: [] for k in runs}
        for _ in range(rounds):
            for k, fn in runs.items():
                us[k].append(1e3 * timeit(fn, 5, warm=1) / reps)
        eb = 4 if dtype == torch.float32 else 8
        print(f"launches alone {name} {tag} ({n} elements, {reps} back to back, {rounds} rounds, us per launch):")
        for k in runs:
            moved = (2 if k == "copy" else 3) * eb * n
            print(f"    {k:16s}: {spread(us[k])}   ({moved / (min(us[k]) * 1e-6) / 1e12:.2f} TB/s at the best)")


def _workload(kind, L, T, H, B, parts):
    torch.manual_seed(0)
    if kind == "phonon":
        from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
        mk = lambda: DOSTransformer_phonon(L, T, 118, 4, H, "cuda", 0.0).to("cuda")
        cs = synth.phonon_crystals(B, seed=1, dtype=torch.float32)
    else:
        from dostransformer_amd.embedder_eDOS.DOSTransformer import DOSTransformer
        mk = lambda: DOSTransformer(L, T, 200, 41, 2, H, "cuda", 0.0).to("cuda")
        cs = synth.edos_crystals(B, seed=1, dtype=torch.float32)
    k = B // parts
    return mk, collate(cs).to("cuda"), [collate(cs[i:i + k]).to("cuda") for i in range(0, B, k)]


def window_case(name, kind, L, T, H, B, parts, iters, rounds, **kw):
    mk, whole, micro = _workload(kind, L, T, H, B, parts)
    window, plain, big = (Trainer(mk(), replay=True, **kw) for _ in range(3))

    def small_steps():
        for g in micro:
            plain.step(g)

    sides = {f"window of {parts} x {B // parts}": lambda: window.step_accumulate(micro),
             f"{parts} plain steps of {B // parts}": small_steps, f"one step of {B}": lambda: big.step(whole)}
    ms = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            ms[k].append(timeit(fn, iters))
    print(f"window {name} {kind} L{L} T{T} H{H} {kw or 'default loss'}, {window._fp.total} flat parameters, ms per optimizer step "
          f"({parts} for the plain steps), {rounds} rounds of {iters}:")
    for k, v in ms.items():
        print(f"    {k:22s}: " + " ".join(f"{x:7.4f}" for x in v) + f"  best {min(v):7.4f} median {sorted(v)[len(v) // 2]:7.4f}")
    w, p, o = (min(ms[k]) for k in sides)
    print(f"    window - {parts} plain steps: {1e3 * (w - p):+.1f} us ({w / p:.4f}); window / one step of {B}: {w / o:.3f}; "
          f"slots {window.slot_misses} recorded, {window.slot_hits} replayed")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert args.rounds >= 3
    print(f"device: {torch.cuda.get_device_name(0)}")
    launches_alone("cfg2", 1634688, args.iters, args.rounds)
    launches_alone("edos", 6664704, args.iters, args.rounds)
    window_case("cfg2", "phonon", 3, 2, 128, 64, 4, args.iters, args.rounds, loss="crystal_rmse")
    window_case("edos", "edos", 3, 2, 256, 64, 4, args.iters, args.rounds)


if __name__ == "__main__":
    main()
