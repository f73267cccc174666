#!/usr/bin/env python3
"""Timing of one evaluation pass over a device-resident split, three ways, in one process.  Report only - not an acceptance bar.

  (a) evaluate.test / test_phonon over ds.batches(1) through Predictor(model): what the reference's metrics (batch_size = 1,
      main_eDOS.py:55-56 / main_phDOS.py:52-55) cost before evaluate.test_per_crystal;
  (b) the same loops over ds.batches(B) through Predictor(model, per_crystal_keys=True): per-BATCH metrics - a different
      quantity (one R2 per flattened batch, a short last batch weighted like a full one); timed only;
  (c) evaluate.test_per_crystal(Predictor(model, per_crystal_keys=True), ds, batch_size=B): the numbers of (a) from batched
      passes - device collate into the bucket, replayed forward, dosx_eval_metrics, one host read at the end.

* phonon: DOSTransformer_phonon L3 T2 H128, 1024 synthetic crystals;
* eDOS:   DOSTransformer L3 T2 H256, 512 synthetic crystals.

Every shape is recorded in a warm-up pass; the three alternate for --rounds rounds so that a drift of the clocks shows in all
columns.  Times are host-clock times around a pass that ends in a synchronise.  Also printed: the largest difference between the
four metrics of (c) and of (a).

usage: python tools/bench_eval.py [--rounds R] [--batch-size B] [--phonon-crystals N] [--edos-crystals N]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dostransformer_amd import evaluate, synth  # noqa: E402
from dostransformer_amd.loader import DeviceDataset  # noqa: E402
from dostransformer_amd.predict import Predictor  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def case(kind, L, T, H, count, B, rounds):
    torch.manual_seed(0)
    if kind == "phonon":
        from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
        model = DOSTransformer_phonon(L, T, 118, 4, H, "cuda", 0.0).to("cuda").eval()
        crystals, loop = synth.phonon_crystals(count, 11, torch.float32), evaluate.test_phonon
    else:
        from dostransformer_amd.embedder_eDOS.DOSTransformer import DOSTransformer
        model = DOSTransformer(L, T, 200, 41, 2, H, "cuda", 0.0).to("cuda").eval()
        crystals, loop = synth.edos_crystals(count, 12, torch.float32), evaluate.test
    ds = DeviceDataset(crystals, "cuda")
    plain, keyed = Predictor(model), Predictor(model, per_crystal_keys=True)
    ways = {"a": lambda: loop(plain, ds.batches(1))[:4],
            "b": lambda: loop(keyed, ds.batches(B))[:4],
            "c": lambda: evaluate.test_per_crystal(keyed, ds, batch_size=B).as_reference()[:4]}
    warm = {k: timed(fn) for k, fn in ways.items()}                      # records every shape
    secs = {k: [] for k in ways}
    for _ in range(rounds):
        for k, fn in ways.items():
            secs[k].append(timed(fn)[0])
    best = {k: min(v) for k, v in secs.items()}
    names = {"a": "test over batches(1)", "b": f"test over batches({B}), per-crystal keys", "c": f"test_per_crystal(batch_size={B})"}
    for k in ways:
        print(f"eval {kind} L{L} T{T} H{H} C{count} ({k}) {names[k]:42s}: warm {warm[k][0] * 1e3:8.2f} ms | " +
              " ".join(f"{v * 1e3:8.2f}" for v in secs[k]) + f" ms  best {best[k] * 1e3:8.2f} ms ({count / best[k]:9.0f} crystals/s)")
    ma, mc = warm["a"][1], warm["c"][1]
    diff = max(abs(float(u) - float(v)) for u, v in zip(ma, mc))
    print(f"     (a) rmse {ma[0]:.6f} mse {ma[1]:.6f} mae {ma[2]:.6f} r2 {ma[3]:.6f}\n"
          f"     (c) rmse {mc[0]:.6f} mse {mc[1]:.6f} mae {mc[2]:.6f} r2 {mc[3]:.6f}   largest |(c) - (a)| {diff:.3e}\n"
          f"     (b) r2 {warm['b'][1][3]:.6f} (per-batch metrics: another quantity)   (c) / (a) rate: {best['a'] / best['c']:.1f}x, "
          f"(c) / (b) rate: {best['b'] / best['c']:.2f}x; buckets recorded by (c): {sum(k[-1] == 'dataset' for k in keyed._slots)}")
    return {"kind": kind, "crystals": count, "batch_size": B, "crystals_per_s": {k: round(count / best[k]) for k in ways},
            "ms": {k: round(best[k] * 1e3, 3) for k in ways}, "c_over_a": round(best["a"] / best["c"], 2), "max_metric_diff_c_a": diff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--phonon-crystals", type=int, default=1024)
    ap.add_argument("--edos-crystals", type=int, default=512)
    args = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name(0)}")
    out = [case("phonon", 3, 2, 128, args.phonon_crystals, args.batch_size, args.rounds),
           case("edos", 3, 2, 256, args.edos_crystals, args.batch_size, args.rounds)]
    print(json.dumps({"bench_eval": out}))


if __name__ == "__main__":
    main()
