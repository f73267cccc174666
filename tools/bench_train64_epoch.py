#!/usr/bin/env python3
"""A SHUFFLED float64 training epoch of DOSTransformer_phonon, three ways.  Report only - not an acceptance bar.

  exact   train64.Trainer64(model, replay=True).step(ds.collate(sel))          one slot per exact batch shape
  bucket  train64.Trainer64(model, replay=True, bucket=(8, 128), promote=0.05).step_dataset(ds, sel, n_max=dataset's)
  eager   train64.Trainer64(model).step(ds.collate(sel))

Setup: L3 T2 H128, per-crystal keys on, 2048 synthetic crystals (synth.phonon_crystals(2048, seed=1)) on a float64
loader.DeviceDataset, batches of 64 in a freshly shuffled order every epoch (32 steps per epoch).  Per process: a first epoch
(untimed: it warms up, and fills what slots it can), then the SECOND epoch between two device events.  Reported: ms per step over
that second epoch, slot_hits / (slot_hits + slot_misses) over both epochs, and the number of live slots.  Without --mode the
script is the driver: every mode runs in a child process of its own under its own time limit, the three alternated, ``--rounds``
rounds, every exit status checked (the driver stops at the first child that fails); one JSON line per process and a summary with
the ratio bucket / exact (written to --log as well).

usage: python tools/bench_train64_epoch.py [--rounds 2] [--log profiles/f64_trainer_epoch_bench.log]
       python tools/bench_train64_epoch.py --mode bucket"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("exact", "bucket", "eager")
L, T, H, B, CRYSTALS = 3, 2, 128, 64, 2048


def run_mode(mode: str, crystals: int, epochs: int) -> dict:
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from dostransformer_amd import synth
    from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
    from dostransformer_amd.loader import DeviceDataset
    from dostransformer_amd.train64 import Trainer64
    torch.manual_seed(0)
    model = DOSTransformer_phonon(L, T, 118, 4, H, "cuda", 0.0).double().set_program_dtype(torch.float64)
    model = model.set_per_crystal_keys(True).to("cuda").train()
    ds = DeviceDataset(synth.phonon_crystals(crystals, seed=1), "cuda", dtype=torch.float64)
    n_max = int(ds.n_nodes.max())
    if mode == "bucket":
        tr = Trainer64(model, lr=1e-4, replay=True, bucket=(8, 128), promote=0.05)
        step = lambda sel: tr.step_dataset(ds, sel, n_max=n_max)
    else:
        tr = Trainer64(model, lr=1e-4, replay=(mode == "exact"))
        step = lambda sel: tr.step(ds.collate(sel))
    ms, steps, loss = None, 0, None
    for epoch in range(epochs):
        order = np.random.default_rng(100 + epoch).permutation(len(ds))
        sels = [order[i:i + B] for i in range(0, len(order), B)]
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        for sel in sels:
            loss = step(sel)
        e.record()
        torch.cuda.synchronize()
        ms, steps = s.elapsed_time(e) / len(sels), len(sels)        # (the last epoch's figure is the one reported)
    total = tr.slot_hits + tr.slot_misses
    return {"mode": mode, "ms_per_step": round(ms, 4), "steps_per_epoch": steps, "epochs": epochs,
            "slot_hits": tr.slot_hits, "slot_misses": tr.slot_misses, "slot_promoted": tr.slot_promoted,
            "hit_rate": round(tr.slot_hits / total, 4) if total else None, "live_slots": len(tr._slots),
            "loss": float(loss), "crystals": crystals, "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=MODES, default=None)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--crystals", type=int, default=CRYSTALS)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--child-timeout", type=int, default=240, help="seconds one child process may take")
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    if args.mode is not None:
        print(json.dumps(run_mode(args.mode, args.crystals, args.epochs)), flush=True)
        return 0
    lines, per_mode, recs = [], {m: [] for m in MODES}, {}

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# float64 DOSTransformer_phonon L{L} T{T} H{H}, per-crystal keys, {args.crystals} synthetic crystals, shuffled epochs of "
         f"{B}-crystal batches; ms per step over epoch {args.epochs} of {args.epochs}; {args.rounds} rounds, one process per mode, alternated")
    for r in range(args.rounds):
        for m in MODES:
            cmd = ["timeout", "-k", "10", str(args.child_timeout), sys.executable, os.path.abspath(__file__), "--mode", m,
                   "--crystals", str(args.crystals), "--epochs", str(args.epochs)]
            out = subprocess.run(cmd, capture_output=True, text=True)
            if out.returncode != 0:                    # a failed child ends the run: nothing more is started on the GPU
                emit(f"# mode {m} round {r}: exit status {out.returncode}; stderr tail: {out.stderr[-2000:]}")
                if args.log:
                    with open(args.log, "w") as f:
                        f.write("\n".join(lines) + "\n")
                return out.returncode
            rec = json.loads(out.stdout.strip().splitlines()[-1])
            rec["round"] = r
            per_mode[m].append(rec["ms_per_step"])
            recs[m] = rec
            emit(json.dumps(rec))
    best = {m: statistics.median(v) for m, v in per_mode.items()}
    emit(json.dumps({"summary_ms_per_step": {m: round(best[m], 4) for m in MODES}, "per_process": per_mode,
                     "hit_rate": {m: recs[m]["hit_rate"] for m in MODES}, "live_slots": {m: recs[m]["live_slots"] for m in MODES},
                     "bucket_over_exact": round(best["bucket"] / best["exact"], 4),
                     "bucket_over_eager": round(best["bucket"] / best["eager"], 4)}))
    if args.log:
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
