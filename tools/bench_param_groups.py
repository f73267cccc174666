#!/usr/bin/env python3
"""Timing of the AdamW launch with parameter groups (Trainer(param_groups=...)) next to the ungrouped one, in one process.
Report only - not an acceptance bar.

* launches alone: dosx_adamw against dosx_adamw_grouped with 1, 4 and 16 groups at the two flat sizes - Phonon-DOS L3 T2 H128
  (1634688 floats) and Electron-DOS L3 T2 H256 (6664704 floats) - replayed back to back from C, so the figure is device time.
  The chunk map changes group every 37 chunks (2368 elements: about a bias-sized parameter), cycling through the groups;
* --launches: nothing but the eight AdamW launches alone - plain, guarded, grouped (4 groups), grouped guarded, each in fp32 and
  float64 - at the same two sizes and in the same way: the table two builds of the library are compared by (DOSX_LIB);
* the replayed training step of the same two models with and without the ``no_decay`` group (weight_decay = 0 for biases,
  norms, slopes, embeddings and prompt tokens).  The two trainers alternate in rounds so that a drift of the clocks shows in
  both columns.

usage: python tools/bench_param_groups.py [--iters N] [--rounds R] [--launches]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dostransformer_amd import ops, param_groups, synth  # noqa: E402
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
    for grouped in (False, True):
        torch.manual_seed(0)
        if kind == "phonon":
            from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
            model = DOSTransformer_phonon(L, T, 118, 4, H, "cuda", 0.0).to("cuda")
            g = synth.phonon_batch(B, seed=1, dtype=torch.float32).to("cuda")
        else:
            from dostransformer_amd.embedder_eDOS.DOSTransformer import DOSTransformer
            model = DOSTransformer(L, T, 200, 41, 2, H, "cuda", 0.0).to("cuda")
            g = synth.edos_batch(B, seed=1, dtype=torch.float32).to("cuda")
        kw = {"param_groups": [{"params": param_groups.no_decay(model), "weight_decay": 0.0}]} if grouped else {}
        trainers.append((grouped, Trainer(model, replay=True, **kw), g))
    ms = {False: [], True: []}
    for _ in range(rounds):
        for grouped, tr, g in trainers:
            ms[grouped].append(timeit(lambda: tr.step(g), iters))
    for grouped in (False, True):
        best, med = min(ms[grouped]), sorted(ms[grouped])[len(ms[grouped]) // 2]
        print(f"step {name} {kind} L{L} T{T} H{H} B{B} no_decay groups={str(grouped):5s}: " + " ".join(f"{v:7.4f}" for v in ms[grouped]) +
              f" ms  best {best:7.4f} median {med:7.4f} ms ({B / (best * 1e-3):8.0f} crystals/s)")
    tr = trainers[1][1]
    runs = int((tr._chunk_group[1:] != tr._chunk_group[:-1]).sum()) + 1
    print(f"     {tr._fp.total} flat parameters, {tr._chunk_group.numel()} chunks in {runs} runs, {len(tr.param_groups[1]['names'])} of "
          f"{len(tr._fp.names)} tensors without decay; grouped / ungrouped (best of {rounds}): {min(ms[True]) / min(ms[False]):.4f} "
          f"({1e3 * (min(ms[True]) - min(ms[False])):+.1f} us)")


def launches_alone(name, n, reps, rounds):
    """The optimizer's launch alone on flat buffers of n floats: `reps` of them recorded and replayed back to back from C
    (ops.Program), so the figure is device time and not the host's cost of issuing them."""
    gen = torch.Generator(device="cuda").manual_seed(0)
    p, g, m, v = (torch.randn(n, device="cuda", generator=gen) for _ in range(4))
    v.abs_()
    hyper = (0.9, 0.999, 1e-8)
    fns = {"adamw": lambda: ops.adamw(p, g, m, v, n, 1e-4, *hyper[:2], hyper[2], 1e-2, 1, 1.0)}
    keep = []
    for G in (1, 4, 16):
        chunk = ((torch.arange(n // 64) // 37) % G).to(torch.uint8).to("cuda")
        st = ops.adamw_groups([(1e-4 * (k + 1) / G, 1e-2 * (k % 2)) for k in range(G)])
        keep.append((chunk, st))
        fns[f"grouped[{G}]"] = lambda chunk=chunk, st=st: ops.adamw_grouped(p, g, m, v, n, chunk, st, *hyper, 1, 1.0)
    progs = {}
    for key, fn in fns.items():
        with ops.recording_scope():
            ops.RECORDER.begin()
            for _ in range(reps):
                fn()
            progs[key] = ops.RECORDER.end()
    us = {k: [] for k in progs}
    for _ in range(rounds):
        for k, prog in progs.items():
            us[k].append(1e3 * timeit(prog.run, 5, warm=1) / reps)
    a = min(us["adamw"])
    print(f"launches alone {name} ({n} floats, {reps} back to back, best of {rounds}): adamw {a:.2f} us, " +
          ", ".join(f"{k} {min(v):.2f} us ({min(v) - a:+.2f})" for k, v in us.items() if k != "adamw"))


def eight_launches(name, n, reps, rounds):
    """Every AdamW entry alone on flat buffers of n elements, `reps` launches replayed back to back from C, best of `rounds`.  The
    guarded forms read a record one grad_guard call wrote before the recording (nothing skipped, no clipping)."""
    hyper, G = (0.9, 0.999, 1e-8), 4
    chunk = ((torch.arange(n // 64) // 37) % G).to(torch.uint8).to("cuda")
    st = ops.adamw_groups([(1e-4 * (k + 1) / G, 1e-2 * (k % 2)) for k in range(G)])
    progs, keep = {}, []
    for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        gen = torch.Generator(device="cuda").manual_seed(0)
        p, g, m, v = (torch.randn(n, device="cuda", generator=gen, dtype=dtype) for _ in range(4))
        v.abs_()
        rec, ws = ops.guard_buffers("cuda")
        ops.grad_guard(g, n, rec, ws, None, 1e-4, *hyper[:2], 1)
        keep.append((p, g, m, v, rec, ws))
        f32 = dtype == torch.float32
        fns = {
            "plain": lambda: ops.adamw(p, g, m, v, n, 1e-4, *hyper, 1e-2, 1, 1.0) if f32 else ops.adamw64(p, g, m, v, n, 1e-4, *hyper, 1e-2, 1),
            "guarded": lambda: (ops.adamw_guarded if f32 else ops.adamw64_guarded)(p, g, m, v, n, 1e-4, *hyper, 1e-2, rec),
            "grouped": lambda: (ops.adamw_grouped if f32 else ops.adamw64_grouped)(p, g, m, v, n, chunk, st, *hyper, 1),
            "grouped_guarded": lambda: (ops.adamw_grouped_guarded if f32 else ops.adamw64_grouped_guarded)(p, g, m, v, n, chunk, st, *hyper, 1, rec),
        }
        for key, fn in fns.items():
            with ops.recording_scope():
                ops.RECORDER.begin()
                for _ in range(reps):
                    fn()
                progs[f"{key}_{tag}"] = ops.RECORDER.end()
    us = {k: [] for k in progs}
    for _ in range(rounds):
        for k, prog in progs.items():
            us[k].append(1e3 * timeit(prog.run, 5, warm=1) / reps)
    print(f"eight launches {name} ({n} elements, {reps} back to back, best of {rounds}): " + ", ".join(f"{k} {min(v):.2f}" for k, v in us.items()) + " us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", action="store_true", help="only the eight AdamW launches alone")
    args = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name(0)}")
    if args.launches:
        eight_launches("cfg2", 1634688, args.iters, args.rounds)
        eight_launches("edos", 6664704, args.iters, args.rounds)
        return
    launches_alone("cfg2", 1634688, args.iters, args.rounds)
    launches_alone("edos", 6664704, args.iters, args.rounds)
    case("cfg2", "phonon", 3, 2, 128, 64, args.iters, args.rounds)
    case("edos", "edos", 3, 2, 256, 64, args.iters, args.rounds)


if __name__ == "__main__":
    main()
