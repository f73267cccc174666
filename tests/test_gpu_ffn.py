"""The feed-forward half of the encoder layer and the row kernels around it (csrc/ffn.hip, rowops.hip; layers/transformer.py:
141-148, 76-77), with the attention half / the final LayerNorm / the output head inside the launches."""
import copy
import ctypes as C
import math
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.util import rmse  # noqa: F401
from tests.gpu_util import (DEV, TOL, _FakeDist, _Hog, _attn_ref, _descs, _fat_crystals, _fatten, _graph, _mixed_jobs, _node_block, _philox_mask_numpy, _phonon, _random_crystals, _reduce, _ref, _scratch, _sliver_case, err, ops, prelu, rnd)  # noqa: F401

pytestmark = pytest.mark.gpu


def test_layernorm_rowdot():
    o = ops()
    S, Bq, H = 51, 6, 128
    M = S * Bq
    x = rnd(M, H, seed=1).double().requires_grad_(True)
    gam = rnd(H, seed=2).double().requires_grad_(True)
    bet = rnd(H, seed=3).double().requires_grad_(True)
    w = rnd(H, seed=4).double().requires_grad_(True)
    b = rnd(1, seed=5).double().requires_grad_(True)
    y = F.layer_norm(x, (H,), gam, bet, 1e-5)
    dos_ref = (y @ w + b).reshape(S, Bq).T
    ddos = rnd(Bq, S, seed=6)
    dos_ref.backward(ddos.double())
    f = lambda t: t.detach().float().contiguous()
    xhat = torch.empty(M, H, device=DEV)
    rstd = torch.empty(M, device=DEV)
    dos = torch.empty(Bq, S, device=DEV)
    o.ln_rowdot(f(x), f(gam), f(bet), f(w), f(b), xhat, rstd, dos, S, Bq, H)
    assert err(dos, dos_ref) < 2e-5
    dx = torch.empty(M, H, device=DEV)
    rows = (M + 31) // 32
    part = torch.empty(rows, 3 * H + 1, device=DEV)
    o.ln_rowdot_bwd(ddos, xhat, rstd, f(gam), f(bet), f(w), dx, part, S, Bq, H)
    ps = part.double().sum(0)
    assert err(dx, x.grad) < 5e-5
    assert err(ps[:H], gam.grad) < 5e-5 and err(ps[H:2 * H], bet.grad) < 5e-5
    assert err(ps[2 * H:3 * H], w.grad) < 5e-5 and abs(float(ps[3 * H]) - float(b.grad)) < 1e-3
    # plain LN fwd/bwd
    yout = torch.empty(M, H, device=DEV)
    o.layernorm(f(x), f(gam), f(bet), yout, xhat, rstd, M, H)
    assert err(yout, y) < 2e-5
    x.grad = None
    gam.grad = None
    bet.grad = None
    dy = rnd(M, H, seed=7)
    F.layer_norm(x, (H,), gam, bet, 1e-5).backward(dy.double())
    part = torch.empty(rows, 2 * H, device=DEV)
    o.layernorm_bwd(dy, xhat, rstd, f(gam), dx, part, M, H)
    ps = part.double().sum(0)
    assert err(dx, x.grad) < 5e-5 and err(ps[:H], gam.grad) < 5e-5 and err(ps[H:], bet.grad) < 5e-5


def test_losses_adamw_misc():
    o = ops()
    B, S = 7, 51
    pg, ps_, y = rnd(B, S, seed=1), rnd(B, S, seed=2), rnd(B, S, seed=3).abs()
    sse = torch.empty(2, device=DEV)
    o.sse2(pg, ps_, y, sse, B * S)
    a = pg.double().requires_grad_(True)
    b = ps_.double().requires_grad_(True)
    loss = torch.sqrt(F.mse_loss(a, y.double())) + 0.7 * torch.sqrt(F.mse_loss(b, y.double()))
    loss.backward()
    dpg, dps, l = torch.empty(B, S, device=DEV), torch.empty(B, S, device=DEV), torch.empty(1, device=DEV)
    o.loss_phonon_bwd(pg, ps_, y, sse, 0.7, B * S, dpg, dps, l, B * S)
    assert abs(float(l) - float(loss)) < 1e-5 and err(dpg, a.grad) < 1e-5 and err(dps, b.grad) < 1e-5
    S = 201
    pg, ps_, yft = rnd(B, S, seed=4), rnd(B, S, seed=5), rnd(B * S, seed=6)
    a = pg.double().requires_grad_(True)
    b = ps_.double().requires_grad_(True)
    yy = torch.where(yft < 0, torch.zeros_like(yft), yft).double().reshape(B, S)
    loss = torch.sqrt(((yy - a) ** 2).mean(1)).mean() + 0.5 * torch.sqrt(((yy - b) ** 2).mean(1)).mean()
    loss.backward()
    dpg, dps, lp = torch.empty(B, S, device=DEV), torch.empty(B, S, device=DEV), torch.empty(B, device=DEV)
    o.loss_edos(pg, ps_, yft, 0.5, B, S, B, dpg, dps, lp)
    assert abs(float(lp.sum()) - float(loss)) < 1e-5 and err(dpg, a.grad) < 1e-5 and err(dps, b.grad) < 1e-5
    # AdamW vs torch.optim.AdamW, 3 steps, odd length
    n = 1003
    p0 = rnd(n, seed=7)
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([p], lr=1e-3, weight_decay=1e-2)
    pf = torch.zeros(1008, device=DEV)
    pf[:n] = p0
    m, v = torch.zeros(1008, device=DEV), torch.zeros(1008, device=DEV)
    for step in range(1, 4):
        g = rnd(n, seed=10 + step)
        p.grad = g.clone()
        opt.step()
        gf = torch.zeros(1008, device=DEV)
        gf[:n] = g
        o.adamw(pf, gf, m, v, n, 1e-3, 0.9, 0.999, 1e-8, 1e-2, step)
    assert err(pf[:n], p.detach()) < 1e-6
    # embed rows / reduce rows / act bwd
    tab = rnd(7, 64, seed=20)
    idx = torch.tensor([3, 3, 0, 6, 1], dtype=torch.int32, device=DEV)
    outr = torch.empty(5, 64, device=DEV)
    o.embed_rows(tab, idx, outr, 5, 64)
    assert torch.equal(outr, tab[idx.long()])
    dtab = torch.empty(7, 64, device=DEV)
    o.embed_rows_bwd(outr.data_ptr(), 64, idx, dtab, 5, 7, 64)
    assert err(dtab, torch.zeros(7, 64, device=DEV, dtype=torch.float64).index_add_(0, idx.long(), outr.double())) < 1e-6
    S, Bb, H = 5, 4, 32
    src = rnd(S * Bb, H, seed=21)
    d1 = torch.empty(S, H, device=DEV)
    o.reduce_rows(src.data_ptr(), H, d1.data_ptr(), H, S, Bb, Bb, 1, H)
    assert err(d1, src.double().reshape(S, Bb, H).sum(1)) < 1e-6
    d2 = torch.empty(Bb, H, device=DEV)
    o.reduce_rows(src.data_ptr(), H, d2.data_ptr(), H, Bb, S, 1, Bb, H)
    assert err(d2, src.double().reshape(S, Bb, H).sum(0)) < 1e-6
    yv, dyv = rnd(100, 32, seed=22), rnd(100, 32, seed=23)
    oo = torch.empty(100, 32, device=DEV)
    o.act_bwd(dyv, yv, 0.01, oo)
    assert err(oo, torch.where(yv > 0, dyv, 0.01 * dyv)) < 1e-7


@pytest.mark.parametrize("M,H", [(7, 16), (100, 128), (3000, 256)])
def test_rownorm_bwd_act(M, H):
    """dosx_rownorm_bwd_act == autograd of  xhat = LN_noaffine(leaky_relu(pre))  plus an extra gradient on leaky_relu(pre)."""
    o = ops()
    pre = rnd(M, H, seed=1).double().requires_grad_(True)
    y = F.leaky_relu(pre, 0.01)
    xhat = F.layer_norm(y, (H,), None, None, 1e-5)
    dxhat, dy_extra = rnd(M, H, seed=2), rnd(M, H, seed=3)
    (xhat * dxhat.double()).sum().backward(retain_graph=True)
    y.backward(dy_extra.double())
    yf = y.detach().float()
    rstd = (1 / torch.sqrt(yf.double().var(1, unbiased=False) + 1e-5)).float()
    out = torch.empty(M, H, device=DEV)
    o.rownorm_bwd_act(dxhat, xhat.detach().float().contiguous(), rstd, dy_extra, yf, 0.01, out, M, H)
    assert err(out, pre.grad) < 5e-5


@pytest.mark.parametrize("M,H", [(33, 32), (100, 64), (3264, 128), (6528, 128), (1, 128)])
def test_ffn_fused_forward(M, H):
    """dosx_ffn_fwd == the two GEMMs of layers/transformer.py:141-148 (pre-norm FFN with residual)."""
    o = ops()
    assert o.ffn_supported(H)
    x = rnd(M, H, seed=1)
    g, b = rnd(H, seed=2), rnd(H, seed=3)
    w1, b1 = rnd(4 * H, H, seed=4, scale=0.2), rnd(4 * H, seed=5)
    w2, b2 = rnd(H, 4 * H, seed=6, scale=0.2), rnd(H, seed=7)
    mu = x.mean(1, keepdim=True)
    rstd = 1 / torch.sqrt(x.var(1, unbiased=False, keepdim=True) + 1e-5)
    stats = torch.cat([mu, rstd], 1).contiguous()
    h = torch.empty(M, 4 * H, device=DEV)
    out = torch.empty(M, H, device=DEV)
    o.ffn_fwd(M, H, x, stats, g, b, w1, b1, w2, b2, h, out)
    xd = x.double()
    ln = F.layer_norm(xd, (H,), g.double(), b.double(), 1e-5)
    href = torch.relu(ln @ w1.double().T + b1.double())
    assert err(h, href) < TOL
    ref = xd + href @ w2.double().T + b2.double()
    assert err(out, ref) < TOL
    # same launch with the encoder's final LayerNorm fused into the row epilogue
    fg, fb = rnd(H, seed=8), rnd(H, seed=9)
    xhat, rstd_o, y = torch.empty(M, H, device=DEV), torch.empty(M, device=DEV), torch.empty(M, H, device=DEV)
    o.ffn_fwd(M, H, x, stats, g, b, w1, b1, w2, b2, h, y, fin=o.Head(fg, fb, xhat, rstd_o))
    mu2 = ref.mean(1, keepdim=True)
    rs2 = 1 / torch.sqrt(ref.var(1, unbiased=False, keepdim=True) + 1e-5)
    assert err(xhat, (ref - mu2) * rs2) < 5e-5 and err(rstd_o, rs2[:, 0]) < 5e-5
    assert err(y, (ref - mu2) * rs2 * fg.double() + fb.double()) < 5e-5


@pytest.mark.parametrize("M,H", [(33, 32), (100, 64), (3264, 128), (6528, 128), (1, 128), (50, 96)])
def test_ffn_fused_backward(M, H):
    """dosx_ffn_bwd == autograd of the pre-norm FFN half layer: dh (masked), dx (incl. the residual path), LN1 dgamma/dbeta."""
    o = ops()
    x = rnd(M, H, seed=1).double().requires_grad_(True)
    g = rnd(H, seed=2).double().requires_grad_(True)
    b = rnd(H, seed=3).double().requires_grad_(True)
    w1, b1 = rnd(4 * H, H, seed=4, scale=0.2), rnd(4 * H, seed=5)
    w2, b2 = rnd(H, 4 * H, seed=6, scale=0.2), rnd(H, seed=7)
    dy = rnd(M, H, seed=8)
    ln = F.layer_norm(x, (H,), g, b, 1e-5)
    pre = ln @ w1.double().T + b1.double()
    pre.retain_grad()
    href = torch.relu(pre)
    out = x + href @ w2.double().T + b2.double()
    out.backward(dy.double())
    xf = x.detach().float()
    mu = xf.mean(1, keepdim=True)
    rstd = 1 / torch.sqrt(xf.var(1, unbiased=False, keepdim=True) + 1e-5)
    stats = torch.cat([mu, rstd], 1).contiguous()
    rows = o.ffn_bwd_partial_rows(M)
    dh = torch.empty(M, 4 * H, device=DEV)
    dx = torch.empty(M, H, device=DEV)
    part = torch.full((rows, 2 * H), float("nan"), device=DEV)
    o.ffn_bwd(M, H, dy, href.detach().float().contiguous(), xf, stats, g.detach().float(), w1, w2, dh, dx, part)
    assert err(dh, pre.grad) < TOL
    assert err(dx, x.grad) < 5e-5
    ps = part.double().sum(0)
    assert err(ps[:H], g.grad) < 5e-5 and err(ps[H:], b.grad) < 5e-5


@pytest.mark.parametrize("H,S,B", [(128, 51, 8), (64, 51, 3), (128, 7, 1)])
@pytest.mark.parametrize("mode", ["cross", "self"])
def test_final_layernorm_backward_inside_ffn_bwd(H, S, B, mode):
    """The encoder's final LayerNorm backward (layers/transformer.py:76-77) fused into the last layer's ffn_bwd launch
    against the stand-alone dosx_layernorm_bwd launch it replaces and against torch autograd on the same module math."""
    from dostransformer_amd import functional as Fn
    from dostransformer_amd.layers import TransformerEncoder
    torch.manual_seed(3)
    enc = TransformerEncoder(embed_dim=H, num_heads=1, layers=2, attn_dropout=0.0).to(DEV)
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if "layer_norm" in n:
                p.add_(0.2 * torch.randn_like(p))
    gen = torch.Generator().manual_seed(11)
    x0 = torch.randn(S, B, H, generator=gen).to(DEV)
    kv0 = torch.randn(9, B, H, generator=gen).to(DEV)
    w = torch.randn(S, B, H, generator=gen).to(DEV)

    def run(fused):
        enc.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        kv = kv0.clone().requires_grad_(True)
        with Fn.forms(_FUSED_FIN_BWD=fused):
            y = enc(x, kv, kv) if mode == "cross" else enc(x, x, x)
            (y * w).sum().backward()
            torch.cuda.synchronize()
        g = {n: p.grad.clone() for n, p in enc.named_parameters() if p.grad is not None}
        return y.detach().clone(), x.grad.clone(), (kv.grad.clone() if mode == "cross" else None), g

    y1, dx1, dkv1, g1 = run(True)
    y0, dx0, dkv0, g0 = run(False)
    sc = lambda t: float(t.abs().max()) + 1e-30
    assert torch.equal(y1, y0)
    assert float((dx1 - dx0).abs().max()) <= 2e-6 * sc(dx0)
    if dkv0 is not None:
        assert float((dkv1 - dkv0).abs().max()) <= 2e-6 * sc(dkv0)
    assert set(g1) == set(g0) and "layer_norm.weight" in g1
    for k in g0:
        assert float((g1[k] - g0[k]).abs().max()) <= 5e-6 * sc(g0[k]), k


@pytest.mark.parametrize("H,S,B", [(128, 51, 4), (64, 51, 3)])
def test_head_inside_ffn_kernels_matches_standalone_launches(H, S, B):
    """Final LayerNorm + out_layer in the last ffn_fwd epilogue / first ffn_bwd prologue of the source encoder against the
    ln_rowdot(_bwd) launches they replace: same DOS, same gradients (fp32 rounding of a different summation tree only)."""
    from dostransformer_amd import functional as Fn
    from dostransformer_amd.batch import collate
    from dostransformer_amd import synth
    from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
    torch.manual_seed(1)
    model = DOSTransformer_phonon(2, 2, 118, 4, H, DEV, 0.0).to(DEV)
    g = collate(synth.phonon_crystals(B, 77, torch.float32)).to(DEV)

    def run(fused):
        model.zero_grad(set_to_none=True)
        with Fn.forms(_FUSED_HEAD_FWD=fused, _FUSED_FIN_BWD=fused):
            out = model(g)
            loss = (out[0] ** 2).sum() + 0.5 * (out[2] ** 2).sum()
            loss.backward()
            torch.cuda.synchronize()
        return [o.detach().clone() for o in (out[0], out[2])], {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}

    o1, g1 = run(True)
    o0, g0 = run(False)
    sc = lambda t: float(t.abs().max()) + 1e-30
    for a, b in zip(o1, o0):
        assert float((a - b).abs().max()) <= 2e-6 * sc(b)
    assert set(g1) == set(g0)
    for k in g0:
        assert float((g1[k] - g0[k]).abs().max()) <= 1e-5 * sc(g0[k]), k


@pytest.mark.parametrize("M,W", [(100, 768), (33, 1024), (5, 260), (70, 512)])
def test_wide_row_kernels_match_float64_autograd(M, W):
    """The one-wave-per-row backward kernels for rows of up to 1024 floats: LayerNorm -> PReLU backward (dosx_ln_prelu_bwd),
    LayerNorm backward (dosx_layernorm_bwd beyond 256) and the LayerNorm + H -> 1 output layer backward (dosx_ln_rowdot_bwd
    beyond 256), against float64 autograd - dx and the column sums of the partial rows."""
    o = ops()
    z = rnd(M, W, seed=1).double().requires_grad_(True)
    gam = rnd(W, seed=2).double().requires_grad_(True)
    bet = (0.3 * rnd(W, seed=3)).double().requires_grad_(True)
    alpha = torch.tensor([0.25], dtype=torch.float64, device=DEV, requires_grad=True)
    dy = rnd(M, W, seed=4)
    mean, var = z.mean(1, keepdim=True), z.var(1, unbiased=False, keepdim=True)
    rstd64 = (var + 1e-5).rsqrt()
    xhat64 = (z - mean) * rstd64
    ln = xhat64 * gam + bet
    act = torch.where(ln >= 0, ln, alpha * ln)
    act.backward(dy.double())
    xhat, rstd = xhat64.detach().float().contiguous(), rstd64.detach().float().reshape(-1).contiguous()
    rows = o.ln_prelu_bwd_partial_rows(M)
    part = torch.full((rows, 2 * W + 4), float("nan"), device=DEV)
    dz = torch.full((M, W), float("nan"), device=DEV)
    o.ln_prelu_bwd(dy, xhat, rstd, gam.detach().float(), bet.detach().float(), alpha.detach().float(), dz, part, M, W)
    torch.cuda.synchronize()
    assert err(dz, z.grad) < TOL
    ps = part.double().sum(0)
    assert err(ps[:W], gam.grad) < TOL and err(ps[W:2 * W], bet.grad) < TOL
    assert abs(float(ps[2 * W + 3]) - float(alpha.grad)) < TOL * max(1.0, abs(float(alpha.grad)))
    # plain LayerNorm backward on the same rows
    z.grad = gam.grad = bet.grad = None
    ln2 = ((z - z.mean(1, keepdim=True)) * (z.var(1, unbiased=False, keepdim=True) + 1e-5).rsqrt()) * gam + bet
    ln2.backward(dy.double())
    part2 = torch.full(((M + 31) // 32, 2 * W), float("nan"), device=DEV)
    dx = torch.full((M, W), float("nan"), device=DEV)
    o.layernorm_bwd(dy, xhat, rstd, gam.detach().float(), dx, part2, M, W)
    torch.cuda.synchronize()
    assert err(dx, z.grad) < TOL
    assert err(part2.double().sum(0)[:W], gam.grad) < TOL and err(part2.double().sum(0)[W:], bet.grad) < TOL
    # LayerNorm + output layer: rows are (s, bq), ddos is [Bq, S]
    S, Bq = (M // 3, 3) if M % 3 == 0 else (M, 1)
    if S * Bq == M:
        z.grad = gam.grad = bet.grad = None
        wv = rnd(W, seed=6).double().requires_grad_(True)
        ddos = rnd(Bq, S, seed=7)
        ln3 = ((z - z.mean(1, keepdim=True)) * (z.var(1, unbiased=False, keepdim=True) + 1e-5).rsqrt()) * gam + bet
        y = (ln3 @ wv).reshape(S, Bq).T
        y.backward(ddos.double())
        part3 = torch.full(((M + 31) // 32, 3 * W + 1), float("nan"), device=DEV)
        dx3 = torch.full((M, W), float("nan"), device=DEV)
        o.ln_rowdot_bwd(ddos, xhat, rstd, gam.detach().float(), bet.detach().float(), wv.detach().float(), dx3, part3, S, Bq, W)
        torch.cuda.synchronize()
        p3 = part3.double().sum(0)
        assert err(dx3, z.grad) < TOL and err(p3[:W], gam.grad) < TOL and err(p3[W:2 * W], bet.grad) < TOL
        assert err(p3[2 * W:3 * W], wv.grad) < TOL and abs(float(p3[3 * W]) - float(ddos.double().sum())) < 1e-4


@pytest.mark.parametrize("form", ["rows", "aligned"])
@pytest.mark.parametrize("Sq,Bq,Nk,Bk,H,bcast,drop", [(51, 64, 12, 64, 128, True, 0.0), (51, 128, 12, 64, 128, False, 0.0),
                                                      (51, 4, 9, 2, 128, False, 0.0), (51, 6, 16, 3, 64, False, 0.3),
                                                      (7, 3, 1, 3, 32, True, 0.0), (201, 8, 5, 8, 96, False, 0.25),
                                                      (51, 128, 12, 64, 128, False, 0.2),
                                                      # more than 16 keys: the crystal-aligned form only (self attention: 51 keys)
                                                      (51, 128, 51, 128, 128, False, 0.0), (51, 64, 51, 64, 128, False, 0.3),
                                                      (40, 5, 64, 5, 64, False, 0.0), (33, 3, 17, 3, 32, False, 0.0)])
def test_encoder_layer_with_attention_inside_the_ffn_launch(Sq, Bq, Nk, Bk, H, bcast, drop, form):
    """DosxFfn.att_*: <= 16-key cross attention in the prologue of dosx_ffn_fwd == dosx_attention_fwd + dosx_ffn_fwd: encoder
    output and every tensor the backward reads (x1, softmax weights, both LayerNorm statistics, h), T = 2 layers, broadcast
    query rows (the energy embeddings: stride 0 over the batch) and dense ones, 16- and 32-row workgroups, dropout masks; and
    the gradients through the (unchanged) backward agree."""
    from dostransformer_amd import functional as Fn
    o = ops()
    # the per-row form takes at most 16 keys: beyond them the policy must fall back to the attention kernel + dosx_ffn_fwd
    assert form != "rows" or Nk <= 16 or not o.ffn_att_supported(H, Nk)
    T = 2
    gen = torch.Generator().manual_seed(Sq * 7 + Nk)
    P, G = {}, {}
    for t in range(T):
        lp = f"e.layers.{t}"
        for k, shp, sc in ((".layer_norms.0.weight", (H,), 1.0), (".layer_norms.0.bias", (H,), 0.3), (".layer_norms.1.weight", (H,), 1.0),
                           (".layer_norms.1.bias", (H,), 0.3), (".fc1.weight", (4 * H, H), H ** -0.5), (".fc1.bias", (4 * H,), 0.1),
                           (".fc2.weight", (H, 4 * H), (4 * H) ** -0.5), (".fc2.bias", (H,), 0.1)):
            P[lp + k] = (torch.randn(*shp, generator=gen) * sc + (1.0 if k.endswith("norms.0.weight") or k.endswith("norms.1.weight") else 0.0)).to(DEV)
    P["e.layer_norm.weight"], P["e.layer_norm.bias"] = (1 + 0.1 * torch.randn(H, generator=gen)).to(DEV), (0.1 * torch.randn(H, generator=gen)).to(DEV)
    P = Fn.pack_params(P)
    x = torch.randn(Sq if bcast else Sq * Bq, H, generator=gen).to(DEV)
    kv = torch.randn(Nk * Bk, H, generator=gen)
    kv[::5] = 0.0                                       # padded key slots: exact zero rows
    kvhat = kv.to(DEV)
    qs, qb = (1, 0) if bcast else (Bq, 1)
    seed = torch.tensor([1234], dtype=torch.int64, device=DEV)
    res = {}
    for fused in (False, True):
        # (the shipped policy fuses by shape; the kernels take any: force the form under test)
        with Fn.forms(_FUSED_ATT_FFN=fused, _ATT_FFN_MAX_ROWS=(1 << 30) if form == "rows" else 0, _ATT_ALIGNED=form == "aligned",
                      _ATT_ALIGNED_MAX_WGS=1 << 30, _ATT_ROWS_FIRST=form == "rows",
                      _FUSED_ATT_BWD=fused and form == "aligned"):      # (round 5: ... and the attention half's backward inside dosx_ffn_bwd)
            o.KERNEL_TIMER.reset(enabled=False)
            y, ctx = Fn.encoder_fwd(P, "e", x, Sq, Bq, qs, qb, kvhat, Nk, Bk, H, T, drop=(drop, seed, 0) if drop > 0 else None)
            G = {k: torch.zeros_like(v) for k, v in P.items()}
            dkv = torch.zeros(Nk * Bk, H, device=DEV)
            sink = o.GradSink(DEV)
            dy = torch.randn(Sq * Bq, H, generator=torch.Generator().manual_seed(5)).to(DEV)
            dx = Fn.encoder_bwd(P, G, "e", ctx, dy, dkv, sink)
            sink.flush()
            torch.cuda.synchronize()
            res[fused] = (y, ctx.layers, dx, dkv, {k: v.clone() for k, v in G.items()})
    (y0, lay0, dx0, dkv0, G0), (y1, lay1, dx1, dkv1, G1) = res[False], res[True]
    rel = lambda a, b: float((a - b).abs().max() / (b.abs().max() + 1e-12))
    assert rel(y1, y0) < 5e-6
    for t in range(T):
        for name in ("x1", "probs", "qstats", "st1", "h"):
            a1, a0 = getattr(lay1[t], name), getattr(lay0[t], name)
            assert not torch.isnan(a1).any(), (t, name)
            assert rel(a1, a0) < 1e-5, (t, name, rel(a1, a0))
        if drop > 0:
            assert torch.equal(lay1[t].mask, lay0[t].mask)                  # same Philox draws
    # A ReLU gate whose pre-activation is below fp32 resolution may flip between the two forms (their sums run in another order:
    # the aligned form multiplies on the MFMA) - ~1e-6 of the 4H x rows gates: one flip moves ONE row of the gradients by O(1e-3)
    # of their maximum.  Without a flip the gradients agree to rounding; with flips, everywhere but in those rows.
    flips = sum(int(((lay1[t].h > 0) != (lay0[t].h > 0)).sum()) for t in range(T))
    if flips == 0:
        assert rel(dx1, dx0) < 2e-5 and rel(dkv1, dkv0) < 2e-5
        for k in G0:
            assert rel(G1[k], G0[k]) < 5e-5, k
    else:
        assert flips <= 8, flips

        def typical(a, b):
            e = ((a - b).abs() / (b.abs().max() + 1e-12)).flatten()
            return float(torch.quantile(e[:4_000_000].double(), 0.95)), float(e.max())     # (a flip reaches one row of dx, one row of fc1's gradient, the key rows of one crystal)
        for name, (a, b) in [("dx", (dx1, dx0)), ("dkv", (dkv1, dkv0))] + [(k, (G1[k], G0[k])) for k in G0]:
            q, mx = typical(a, b)
            assert mx < 0.2 and (q < 2e-4 or a.numel() < 2000), (name, q, mx, flips)     # (weight gradients: sums over thousands of rows of the 1e-6 forward differences)


@pytest.mark.parametrize("mode", ["graph", "replay"])
def test_concurrent_feed_forward_tail_is_bitwise_in_every_launch_mode(mode):
    """The tail rows of the unfused feed-forward layers run as a concurrent chain on the side stream (functional._ffn_tail_start,
    ops.concurrent): an Electron-DOS model with hidden 256 and 21 crystals has 2 * 21 * 201 = 8442 rows = one full round of
    8192 + 250.  Recorded replay and HIP-graph capture (stream fork / join recorded resp. captured) against the eagerly issued
    step on the same ghost-padded batch (one stream, the two chains one after the other): the same bits after 3 steps."""
    import copy
    from dostransformer_amd import functional as Fn, synth
    from dostransformer_amd.batch import bucket_sizes, pad_batch
    from dostransformer_amd.embedder_eDOS.DOSTransformer import DOSTransformer
    from dostransformer_amd.train import Trainer
    assert Fn._ffn_tail_start(2 * 21 * 201, 256) == 8192
    torch.manual_seed(0)
    b = synth.edos_batch(21, seed=77, dtype=torch.float32).to(DEV)
    bp = pad_batch(b, *bucket_sizes(b.meta.num_nodes, b.meta.num_edges))
    mk = lambda: DOSTransformer(3, 1, 200, 41, 2, 256, DEV, 0.0)
    m_e = mk().to(DEV)
    m_r = mk()
    m_r.load_state_dict(copy.deepcopy(m_e.state_dict()))
    m_r = m_r.to(DEV)
    te = Trainer(m_e, lr=1e-3)
    tr = Trainer(m_r, lr=1e-3, graph=(mode == "graph"), replay=(mode == "replay"))
    for i in range(3):
        le, lr_ = te.step(bp), tr.step(b)
        assert float(le) == float(lr_), i
    torch.cuda.synchronize()
    for (k, a), (_, c) in zip(m_e.state_dict().items(), m_r.state_dict().items()):
        if a.is_floating_point():
            assert torch.equal(a, c), k


@pytest.mark.parametrize("Sq,Bq,Nk,Bk,H,T,bcast,final", [(51, 64, 12, 64, 128, 2, True, True), (51, 128, 51, 128, 128, 2, False, True),
                                                         (51, 128, 12, 64, 128, 2, False, False), (51, 6, 9, 3, 64, 3, False, True),
                                                         (51, 8, 51, 8, 64, 1, False, True)])
def test_encoder_stack_layers_in_one_launch(Sq, Bq, Nk, Bk, H, T, bcast, final):
    """dosx_ffn_fwd_multi (round 6): the layers of one encoder stack - each attending over the ORIGINAL keys, transformer.py:72-73,
    so row-local per tile once the attention half is inside the launch - run back to back in ONE launch (two per launch): output,
    every saved tensor of every layer (x1, P, statistics, h) and the final LayerNorm's xhat / rstd BITWISE the per-layer launches."""
    from dostransformer_amd import functional as Fn
    gen = torch.Generator().manual_seed(Sq + Bq + Nk + H)
    P = {}
    for t in range(T):
        lp = f"e.layers.{t}"
        for k, shp in ((".layer_norms.0.weight", (H,)), (".layer_norms.0.bias", (H,)), (".layer_norms.1.weight", (H,)), (".layer_norms.1.bias", (H,)),
                       (".fc1.weight", (4 * H, H)), (".fc1.bias", (4 * H,)), (".fc2.weight", (H, 4 * H)), (".fc2.bias", (H,))):
            v = torch.randn(*shp, generator=gen) * (0.1 if "bias" in k else (shp[-1] ** -0.5 if len(shp) == 2 else 1.0))
            P[lp + k] = (1.0 + 0.1 * v if "layer_norms" in k and "weight" in k else v)
    P["e.layer_norm.weight"], P["e.layer_norm.bias"] = 1 + 0.1 * torch.randn(H, generator=gen), 0.1 * torch.randn(H, generator=gen)
    P = Fn.pack_params({k: v.to(DEV) for k, v in P.items()})
    x = (torch.randn(Sq, H, generator=gen) if bcast else torch.randn(Sq * Bq, H, generator=gen)).to(DEV)
    kvhat = torch.randn(Nk * Bk, H, generator=gen).to(DEV)
    qs, qb = (1, 0) if bcast else (Bq, 1)
    res = {}
    for multi in (False, True):
        with Fn.forms(_FFN_MULTI=multi):
            y, ctx = Fn.encoder_fwd(P, "e", x, Sq, Bq, qs, qb, kvhat, Nk, Bk, H, T, final_ln=final)
            torch.cuda.synchronize()
        res[multi] = (y, ctx)
    (y0, c0), (y1, c1) = res[False], res[True]
    assert bool(torch.isfinite(y1).all()) and torch.equal(y0, y1)
    for l0, l1 in zip(c0.layers, c1.layers):
        for name in ("x1", "probs", "qstats", "st1", "h"):
            assert torch.equal(getattr(l0, name), getattr(l1, name)), name
    if final:
        assert torch.equal(c0.fin.xhat, c1.fin.xhat) and torch.equal(c0.fin.rstd, c1.fin.rstd)


_FWD_ONE = ["dosx_ffn_fwd_multi"]
_FWD_ATT = ["dosx_attention_fwd", "dosx_ffn_fwd"] * 2
_FWD_DROPOUT = ["dosx_dropout_mask", "dosx_attention_fwd", "dosx_mask_residual", "dosx_gemm", "dosx_mask_residual", "dosx_gemm",
                "dosx_mask_residual"] * 2 + ["dosx_layernorm"]
_BWD_DROPOUT = ["dosx_layernorm_bwd"] + ["dosx_gemm", "dosx_mask_residual", "dosx_gemm", "dosx_mask_residual", "dosx_attention_bwd",
                                         "dosx_mask_residual"] * 2


@pytest.mark.parametrize("form,H,Nk,relu_drop,fwd,bwd", [
    ("IN_FFN", 64, 12, 0.0, _FWD_ONE, ["dosx_ffn_bwd"] * 2),
    ("ONE_LAUNCH", 32, 12, 0.0, _FWD_ONE, ["dosx_ffn_bwd", "dosx_attention_bwd"] * 2),
    ("SPLIT", 64, 70, 0.0, _FWD_ATT, ["dosx_ffn_bwd", "dosx_attention_bwd", "dosx_attention_bwd"] * 2),
    ("DROPOUT", 64, 12, 0.3, _FWD_DROPOUT, _BWD_DROPOUT)])
def test_each_named_form_issues_its_entries(form, H, Nk, relu_drop, fwd, bwd):
    """functional.ffn_form / attention_form_bwd name the program: a two-layer encoder (Sq 51, Bq 4, Bk 2), forward and backward
    under ops.call_log(), at the smallest shapes that reach each form - the form is named beforehand, then the entries are the
    form's.  Numerics are the oracle tests'; this pins name <-> launch list."""
    from dostransformer_amd import functional as Fn
    Sq, Bq, Bk, T = 51, 4, 2, 2
    fdrop = relu_drop > 0.0
    want_ffn = Fn.FfnForm.DROPOUT if fdrop else Fn.FfnForm.ONE_LAUNCH
    want_att = Fn.AttBwdForm.ONE_LAUNCH if fdrop else Fn.AttBwdForm[form]
    assert Fn.ffn_form(H, fdrop) is want_ffn and Fn.attention_form_bwd(Sq, Bq, Nk, H, fdrop) is want_att
    assert Fn.attention_bwd_in_ffn(Sq, Bq, Nk, H, fdrop) == (form == "IN_FFN")
    gen = torch.Generator().manual_seed(H + Nk)
    P = {}
    for t in range(T):
        for k, shp in ((".layer_norms.0.weight", (H,)), (".layer_norms.0.bias", (H,)), (".layer_norms.1.weight", (H,)), (".layer_norms.1.bias", (H,)),
                       (".fc1.weight", (4 * H, H)), (".fc1.bias", (4 * H,)), (".fc2.weight", (H, 4 * H)), (".fc2.bias", (H,))):
            v = torch.randn(*shp, generator=gen) * (0.1 if "bias" in k else (shp[-1] ** -0.5 if len(shp) == 2 else 1.0))
            P[f"e.layers.{t}" + k] = (1.0 + 0.1 * v if "layer_norms" in k and "weight" in k else v)
    P["e.layer_norm.weight"], P["e.layer_norm.bias"] = 1 + 0.1 * torch.randn(H, generator=gen), 0.1 * torch.randn(H, generator=gen)
    P = Fn.pack_params({k: v.to(DEV) for k, v in P.items()})
    G = {k: torch.zeros_like(v) for k, v in P.items()}
    x, dy = torch.randn(Sq * Bq, H, generator=gen).to(DEV), torch.randn(Sq * Bq, H, generator=gen).to(DEV)
    kvhat = torch.randn(Nk * Bk, H, generator=gen).to(DEV)
    dkv = torch.zeros(Nk * Bk, H, device=DEV)
    seed = torch.tensor([11], dtype=torch.int64, device=DEV)
    o = ops()
    with o.call_log() as names_fwd:
        y, ctx = Fn.encoder_fwd(P, "e", x, Sq, Bq, Bq, 1, kvhat, Nk, Bk, H, T, fdrop=(relu_drop, 0.0, seed, 1000) if fdrop else None)
    sink = o.GradSink(x.device)
    with o.call_log() as names_bwd:
        dx = Fn.encoder_bwd(P, G, "e", ctx, dy, dkv, sink)
    sink.flush()
    sink.release()
    torch.cuda.synchronize()
    assert names_fwd == fwd and names_bwd == bwd, (names_fwd, names_bwd)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(dx).all()) and bool(dkv.abs().sum() > 0)
    assert all(bool(G[k].abs().sum() > 0) for k in G), [k for k in G if not bool(G[k].abs().sum() > 0)]
