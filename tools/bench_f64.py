#!/usr/bin/env python3
"""Timing of the float64 program (csrc/f64.hip, functional64.py).  Report only - not an acceptance bar.

* the fp64 GEMM and weight gradient alone at a roofline-scale shape, as TFLOP/s against the public fp64 matrix peak of the
  MI355X (78.6 TF/s, vendor specification, not measured here);
* a full eager Graphnetwork_phonon training step in float64 (forward, sqrt-MSE loss, backward, torch.optim.AdamW) at the
  cfg1 (L3 H64 B8) and cfg2 (L3 H128 B64) sizes, with the same step of the fp32 module next to it;
* the float64 attention (csrc/f64_attention.hip) forward + backward alone at the cfg2 cross shape (Sq 51, Bq 128, Bk 64,
  H 128, Nk = the batch's nmax) and self shape (Nk 51, Bk 128), in TF/s of its five matrix products;
* a float64 DOSTransformer_phonon step (set_program_dtype(torch.float64): autograd, the phonon loss, torch.optim.AdamW) at
  cfg1 (L3 T1 H64 B8) and cfg2 (L3 T2 H128 B64), next to the same eager step of the fp32 module.  The host float64 reference
  takes 35.8 ms (cfg1) and 409 ms (cfg2) per step on 8 threads.

usage: python tools/bench_f64.py [--iters N] [--dt-cfg2-f64]"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dostransformer_amd import ops, synth  # noqa: E402
from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon  # noqa: E402
from dostransformer_amd.embedder_phDOS.graphnetwork_phonon import Graphnetwork_phonon  # noqa: E402

F64_PEAK_TFLOPS = 78.6


def timeit(fn, iters, warm=3):
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


def gemm_cases(iters):
    dev = "cuda"
    for M, N, K in [(16384, 1024, 1024), (12800, 256, 384)]:
        a = torch.randn(M, K, dtype=torch.float64, device=dev)
        w = torch.randn(N, K, dtype=torch.float64, device=dev)
        out = torch.empty(M, N, dtype=torch.float64, device=dev)
        ms = timeit(lambda: ops.gemm64(M, N, [ops.seg64(a)], w, out), iters)
        tf = 2.0 * M * N * K / (ms * 1e-3) / 1e12
        print(f"gemm64   M={M:6d} N={N:5d} K={K:5d}: {ms * 1e3:9.1f} us  {tf:6.2f} TF/s  ({100 * tf / F64_PEAK_TFLOPS:5.1f} % of "
              f"{F64_PEAK_TFLOPS} peak)")
        dy = torch.randn(M, N, dtype=torch.float64, device=dev)
        dw = torch.empty(N, K, dtype=torch.float64, device=dev)
        ms = timeit(lambda: ops.wgrad64(M, dy, [ops.seg64(a)], dw), iters)
        tf = 2.0 * M * N * K / (ms * 1e-3) / 1e12
        print(f"wgrad64  M={M:6d} N={N:5d} K={K:5d}: {ms * 1e3:9.1f} us  {tf:6.2f} TF/s  ({100 * tf / F64_PEAK_TFLOPS:5.1f} % of "
              f"{F64_PEAK_TFLOPS} peak)")


def step_case(name, L, H, B, dtype, iters):
    torch.manual_seed(0)
    model = Graphnetwork_phonon(L, 118, 4, H, 51, "cuda").to(dtype).to("cuda")
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=1e-2)
    g = synth.phonon_batch(B, seed=1, dtype=dtype).to("cuda")

    def step():
        opt.zero_grad()
        loss = torch.sqrt(F.mse_loss(model(g), g.phdos))
        loss.backward()
        opt.step()
    ms = timeit(step, iters)
    print(f"step {name} Graphnetwork_phonon L{L} H{H} B{B} {str(dtype)[6:]:8s}: {ms:8.3f} ms  "
          f"({B / (ms * 1e-3):9.0f} crystals/s)  N={g.x.shape[0]} E={g.edge_index.shape[1]}")


def attention_cases(iters):
    dev = "cuda"
    nmax = int(torch.bincount(synth.phonon_batch(64, seed=1).batch).max())
    for name, Sq, Bq, Nk, Bk, H in [("cross", 51, 128, nmax, 64, 128), ("self", 51, 128, 51, 128, 128)]:
        q, x = torch.randn(Bq * Sq, H, dtype=torch.float64, device=dev), torch.randn(Bq * Sq, H, dtype=torch.float64, device=dev)
        kv = torch.randn(Bk * Nk, H, dtype=torch.float64, device=dev)
        g0, b0 = torch.ones(H, dtype=torch.float64, device=dev), torch.zeros(H, dtype=torch.float64, device=dev)
        dkv = torch.empty_like(kv)
        _, probs = ops.attention64(q, x, kv, g0, b0, Sq, Bq, Nk, Bk)

        def fb():
            ops.attention64(q, x, kv, g0, b0, Sq, Bq, Nk, Bk)
            ops.attention_bwd64(x, q, kv, g0, b0, probs, Sq, Bq, Nk, Bk, dkv)
        ms = timeit(fb, iters)
        tf = 5 * 2.0 * Bq * Sq * Nk * H / (ms * 1e-3) / 1e12      # q.k, p.v | dout.v, ds.k, (ds^T q + p^T dout)
        print(f"attn64 fwd+bwd {name:5s} Sq={Sq} Bq={Bq} Nk={Nk:3d} Bk={Bk:3d} H={H}: {ms * 1e3:8.1f} us  {tf:6.2f} TF/s  "
              f"({100 * tf / F64_PEAK_TFLOPS:5.1f} % of {F64_PEAK_TFLOPS} peak)")


def dt_step_case(name, L, T, H, B, dtype, iters):
    from oracle.dos_oracle import loss_phonon
    torch.manual_seed(0)
    model = DOSTransformer_phonon(L, T, 118, 4, H, "cuda", 0.0).to(dtype)
    if dtype == torch.float64:
        model.set_program_dtype(torch.float64)
    model = model.to("cuda")
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=1e-2)
    g = synth.phonon_batch(B, seed=1, dtype=dtype).to("cuda")

    def step():
        opt.zero_grad()
        dg, _, ds = model(g)
        loss_phonon(dg, ds, g.phdos).backward()
        opt.step()
    ms = timeit(step, iters)
    print(f"step {name} DOSTransformer_phonon L{L} T{T} H{H} B{B} {str(dtype)[6:]:8s}: {ms:8.3f} ms  "
          f"({B / (ms * 1e-3):9.0f} crystals/s)  N={g.x.shape[0]} E={g.edge_index.shape[1]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--dt-cfg2-f64", action="store_true", help="only the float64 DOSTransformer_phonon cfg2 step (for rocprofv3)")
    args = ap.parse_args()
    if args.dt_cfg2_f64:
        dt_step_case("cfg2", 3, 2, 128, 64, torch.float64, args.iters)
        return
    print(f"device: {torch.cuda.get_device_name(0)}")
    gemm_cases(args.iters)
    for name, L, H, B in [("cfg1", 3, 64, 8), ("cfg2", 3, 128, 64)]:
        for dt in (torch.float64, torch.float32):
            step_case(name, L, H, B, dt, args.iters)
    attention_cases(args.iters)
    for name, L, T, H, B in [("cfg1", 3, 1, 64, 8), ("cfg2", 3, 2, 128, 64)]:
        for dt in (torch.float64, torch.float32):
            dt_step_case(name, L, T, H, B, dt, args.iters)


if __name__ == "__main__":
    main()
