#!/usr/bin/env python3
"""What linear functionals of the DOS in the per-crystal losses cost (dosx_loss_rows_fn, csrc/loss_functional.hip; DESIGN.md
9.12).  Report only - not an acceptance bar: this is not a speed feature.

* the launch alone: ``dosx_loss_rows_fn`` (RMSE kind, two outputs with per_crystal - the trainers' form, two launches per call)
  with a cumulative table and SQ, with ABS, and with sample weights on top, at (B, S, K) = (64, 51, 51), (64, 201, 201) and
  (64, 201, 3), next to ``dosx_loss_rows_w`` (sample weights) and ``dosx_loss_rows`` at the same (B, S) - the kernels the parent
  commit has, whose device code this tree keeps.  Every side is a recorded program of ``--iters`` calls back to back, replayed
  from C and timed with device events; the sides alternate in rounds; best, median and spread per side;
* the replayed training step of Phonon-DOS L3 T2 H128 B64 and Electron-DOS L3 T2 H256 B64 with ``loss="crystal_rmse"``, without
  and with the cumulative term (SQ and ABS), the trainers alternating in rounds.

Not timed here: the float64 entries, the one-workgroup form (per_crystal == NULL), the other three pointwise kinds,
dosx_eval_functionals, and the parent commit's own library in a process of its own.

usage: python tools/bench_loss_functional.py [--iters N] [--rounds R]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from dostransformer_amd import functionals, ops, synth  # noqa: E402
from dostransformer_amd.train import Trainer  # noqa: E402

SHAPES = ((64, 51, 51), (64, 201, 201), (64, 201, 3))


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


def launch_sides(B, S, K):
    gen = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *s: torch.randn(*s, device="cuda", generator=gen)
    y = r(B, S) * 0.8
    pg, ps = y.clamp(min=0) + 0.1 * r(B, S), y.clamp(min=0) + 0.1 * r(B, S)
    dpg, dps, per, loss = (torch.empty(*s, device="cuda") for s in ((B, S), (B, S), (B,), (1,)))
    kw = dict(clamp_target=True, beta=1.0, dpg=dpg, dps=dps, per_crystal=per, loss=loss)
    w = 0.25 + 3.75 * torch.rand(B, device="cuda", generator=gen)
    # K == S: the cumulative table; fewer rows: the cumulative DOS at K evenly spaced bins
    rows = torch.linspace(0, S - 1, K).round().long()
    tab = functionals.cumulative(S, 1.0 / S).table[rows].float().cuda().contiguous()
    fn = lambda kind, **more: (lambda: ops.loss_rows(pg, ps, y, "crystal_rmse", functionals=tab, functional_kind=kind,
                                                     functional_weight=0.5, **more, **kw))
    return {"loss_rows": lambda: ops.loss_rows(pg, ps, y, "crystal_rmse", **kw),
            "loss_rows_w  w": lambda: ops.loss_rows(pg, ps, y, "crystal_rmse", weights=w, **kw),
            "loss_rows_fn sq": fn("sq"), "loss_rows_fn abs": fn("abs"), "loss_rows_fn sq, w": fn("sq", weights=w)}


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
    base = us["loss_rows_w  w"]
    for k, v in us.items():
        if k.startswith("loss_rows_fn"):
            print(f"    {k:22s} - loss_rows_w, best - best: {min(v) - min(base):+.2f} us (spread of loss_rows_w's rounds "
                  f"{max(base) - min(base):.2f} us, of its own {max(v) - min(v):.2f} us)")


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
    for name, fk in (("crystal_rmse", None), ("+ cumulative sq", "sq"), ("+ cumulative abs", "abs")):
        model, g = _workload(kind, L, T, H, B)
        S = int(model._cfg.S)
        kw = {} if fk is None else dict(functionals=functionals.cumulative(S, 1.0 / S), functional_kind=fk, functional_weight=0.5)
        trainers.append((name, Trainer(model, replay=True, loss="crystal_rmse", **kw), g))
    ms = {name: [] for name, _, _ in trainers}
    for _ in range(rounds):
        for name, tr, g in trainers:
            ms[name].append(timeit(lambda: tr.step(g), iters))
    for name in ms:
        print(f"step {kind} L{L} T{T} H{H} B{B} {name:18s}: " + " ".join(f"{v:7.4f}" for v in ms[name]) +
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
