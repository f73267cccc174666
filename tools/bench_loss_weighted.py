#!/usr/bin/env python3
"""What sample weights and energy-bin weights in the per-crystal losses cost (dosx_loss_rows_w, csrc/loss_rows.hip; DESIGN.md
9.10).  Report only - not an acceptance bar: this is not a speed feature.

* the launch alone: ``dosx_loss_rows_w`` in three forms - ``w`` only, ``w`` gathered through ``w_index`` out of a 4096-entry
  table, ``w`` with ``bin_w`` - next to the unweighted ``dosx_loss_rows`` at (B, S) = (64, 51), (64, 201), (512, 51); RMSE kind,
  two outputs with per_crystal (the trainers' form: two launches per call).  Every side is a recorded program of ``--iters``
  calls back to back, replayed from C and timed with device events; the sides alternate in rounds; best and spread per side.
  Expectation to confirm or refute: the differences are inside the rounds' spread (launch-bound; B + S more elements read);
* ``--parent DIR`` (a checkout of the parent commit with its library built): the unweighted entry of THAT library, measured by
  the same code in child processes that alternate with child processes on this tree, ``--rounds`` times each;
* the replayed training step of Phonon-DOS L3 T2 H128 B64 and Electron-DOS L3 T2 H256 B64 with ``loss="crystal_rmse"``, with
  and without ``sample_weights=True`` (and with ``bin_weights`` on top), the trainers alternating in rounds.

Not timed here: the float64 entries, the one-workgroup form (per_crystal == NULL), the other three kinds.

usage: python tools/bench_loss_weighted.py [--iters N] [--rounds R] [--parent DIR]"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.abspath(__file__)
SHAPES = ((64, 51), (64, 201), (512, 51))


def _tree(argv):
    """--tree DIR: the package is imported from DIR (the parent's checkout) instead of from this file's repository"""
    if "--tree" in argv:
        return os.path.abspath(argv[argv.index("--tree") + 1])
    return os.path.dirname(os.path.dirname(HERE))


sys.path.insert(0, _tree(sys.argv))
import torch  # noqa: E402
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


def launch_sides(B, S, weighted=True):
    gen = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *s: torch.randn(*s, device="cuda", generator=gen)
    y = r(B, S) * 0.8
    pg, ps = y.clamp(min=0) + 0.1 * r(B, S), y.clamp(min=0) + 0.1 * r(B, S)
    dpg, dps, per, loss = (torch.empty(*s, device="cuda") for s in ((B, S), (B, S), (B,), (1,)))
    kw = dict(clamp_target=True, beta=1.0, dpg=dpg, dps=dps, per_crystal=per, loss=loss)
    sides = {"loss_rows": lambda: ops.loss_rows(pg, ps, y, "crystal_rmse", **kw)}
    if weighted:
        w = 0.25 + 3.75 * torch.rand(B, device="cuda", generator=gen)
        table = 0.25 + 3.75 * torch.rand(4096, device="cuda", generator=gen)
        sel = torch.randint(0, 4096, (B,), device="cuda", generator=gen).to(torch.int32)
        v = 2.0 * torch.rand(S, device="cuda", generator=gen)
        sides["loss_rows_w  w"] = lambda: ops.loss_rows(pg, ps, y, "crystal_rmse", weights=w, **kw)
        sides["loss_rows_w  w[w_index]"] = lambda: ops.loss_rows(pg, ps, y, "crystal_rmse", weights=table, weight_index=sel, **kw)
        sides["loss_rows_w  w, bin_w"] = lambda: ops.loss_rows(pg, ps, y, "crystal_rmse", weights=w, bin_weights=v, **kw)
    return sides


def launches_alone(B, S, reps, rounds, weighted=True):
    """-> {side: [us per call, one per round]}"""
    progs = {}
    for key, fn in launch_sides(B, S, weighted).items():
        with ops.recording_scope():
            ops.RECORDER.begin()
            for _ in range(reps):
                fn()
            progs[key] = ops.RECORDER.end()
    us = {k: [] for k in progs}
    for _ in range(rounds):
        for k, p in progs.items():
            us[k].append(1e3 * timeit(p.run, 5, warm=1) / reps)
    return us


def report_launches(B, S, reps, rounds):
    us = launches_alone(B, S, reps, rounds)
    print(f"launches alone B{B} S{S} ({reps} calls back to back, {rounds} alternated rounds, us per call):")
    for k, v in us.items():
        print(f"    {k:26s}: {spread(v)}")
    base = us["loss_rows"]
    for k, v in us.items():
        if k != "loss_rows":
            print(f"    {k:26s} - loss_rows, best - best: {min(v) - min(base):+.2f} us (spread of loss_rows' rounds "
                  f"{max(base) - min(base):.2f} us, of its own {max(v) - min(v):.2f} us)")


def against_parent(parent, reps, rounds):
    """The unweighted entry of the parent's library against this tree's, child processes alternating."""
    res = {"parent": {s: [] for s in SHAPES}, "this": {s: [] for s in SHAPES}}
    for _ in range(rounds):
        for side, tree in (("parent", os.path.abspath(parent)), ("this", _tree([]))):
            out = subprocess.run([sys.executable, HERE, "--tree", tree, "--child", "--iters", str(reps)], check=True,
                                 capture_output=True, text=True, timeout=300).stdout
            row = json.loads(out.strip().splitlines()[-1])
            for s in SHAPES:
                res[side][s].append(row[f"{s[0]}x{s[1]}"])
    print(f"unweighted dosx_loss_rows, the parent's library against this one ({rounds} alternated processes each, best of 3 "
          f"rounds inside a process, us per call):")
    for s in SHAPES:
        a, b = res["parent"][s], res["this"][s]
        print(f"    B{s[0]} S{s[1]}: parent {spread(a)}")
        print(f"    {'':{len(f'B{s[0]} S{s[1]}')}}  this   {spread(b)}   best - best {min(b) - min(a):+.2f} us")


def _workload(kind, L, T, H, B):
    torch.manual_seed(0)
    if kind == "phonon":
        from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
        return (DOSTransformer_phonon(L, T, 118, 4, H, "cuda", 0.0).to("cuda"),
                synth.phonon_batch(B, seed=1, dtype=torch.float32).to("cuda"))
    from dostransformer_amd.embedder_eDOS.DOSTransformer import DOSTransformer
    return DOSTransformer(L, T, 200, 41, 2, H, "cuda", 0.0).to("cuda"), synth.edos_batch(B, seed=1, dtype=torch.float32).to("cuda")


def step_case(kind, L, T, H, B, iters, rounds):
    gen = torch.Generator().manual_seed(3)
    trainers = []
    for name, kw in (("crystal_rmse", {}), ("+ sample_weights", dict(sample_weights=True)),
                     ("+ sample_weights, bin_weights", dict(sample_weights=True, bin_weights=True))):
        model, g = _workload(kind, L, T, H, B)
        if kw.get("bin_weights"):
            kw = dict(kw, bin_weights=2.0 * torch.rand(int(model._cfg.S), generator=gen, dtype=torch.float64) + 1e-3)
        if kw.get("sample_weights"):
            g.weight = (0.25 + 3.75 * torch.rand(B, generator=gen)).to("cuda")
        trainers.append((name, Trainer(model, replay=True, loss="crystal_rmse", **kw), g))
    ms = {name: [] for name, _, _ in trainers}
    for _ in range(rounds):
        for name, tr, g in trainers:
            ms[name].append(timeit(lambda: tr.step(g), iters))
    for name in ms:
        print(f"step {kind} L{L} T{T} H{H} B{B} {name:30s}: " + " ".join(f"{v:7.4f}" for v in ms[name]) +
              f" ms  best {min(ms[name]):7.4f} median {sorted(ms[name])[len(ms[name]) // 2]:7.4f} ms")
    a = min(ms["crystal_rmse"])
    for name in list(ms)[1:]:
        b = min(ms[name])
        print(f"     {name} / crystal_rmse (best of {rounds}): {b / a:.4f} ({1e3 * (b - a):+.1f} us); spread of the unweighted "
              f"trainer's rounds {1e3 * (max(ms['crystal_rmse']) - a):.1f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent", default=None, help="checkout of the parent commit with dostransformer_amd/csrc/libdosx.so built")
    ap.add_argument("--tree", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:                        # one process of against_parent(): the unweighted entry of --tree's library, JSON
        row = {f"{B}x{S}": min(launches_alone(B, S, args.iters, 3, weighted=False)["loss_rows"]) for B, S in SHAPES}
        print(json.dumps(row))
        return
    assert args.rounds >= 3
    print(f"device: {torch.cuda.get_device_name(0)}")
    for B, S in SHAPES:
        report_launches(B, S, args.iters, args.rounds)
    if args.parent:
        against_parent(args.parent, args.iters, args.rounds)
    step_case("phonon", 3, 2, 128, 64, args.iters, args.rounds)
    step_case("edos", 3, 2, 256, 64, args.iters, args.rounds)


if __name__ == "__main__":
    main()
