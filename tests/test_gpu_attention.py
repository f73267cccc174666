"""Attention on the GPU (csrc/attention*.hip; layers/multihead_attention.py:49-76, layers/transformer.py:120-157): forward,
backward forms, dropout, K != V, key counts beyond the MFMA kernels."""
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


@pytest.mark.parametrize("Sq,Bq,Nk,Bk,H,bcast", [(51, 4, 12, 4, 128, False), (51, 6, 9, 3, 64, False),
                                                   (201, 2, 41, 2, 256, False), (70, 3, 70, 3, 128, False),
                                                   (51, 5, 7, 5, 128, True), (201, 2, 201, 2, 256, False),
                                                   (7, 3, 5, 3, 16, False),
                                                   # more than 320 keys: the general kernels behind the same contract
                                                   (51, 4, 330, 2, 128, False), (20, 3, 700, 3, 64, False),
                                                   (51, 4, 321, 4, 128, True), (9, 2, 400, 2, 256, False)])
@pytest.mark.parametrize("drop", [0.0, 0.35])
@pytest.mark.parametrize("pkv", [False, True])
def test_attention_fwd_bwd(Sq, Bq, Nk, Bk, H, bcast, pkv, drop):
    """pkv: the dq kernel also produces the per-tile dK + dV partials and a reduction kernel finishes the key gradient
    (Nk <= 64; DosxAttn.dkv_part) instead of the streamed dkv kernel behind the dscores round trip.  Beyond the shapes that
    path covers, a given dkv_part is left alone and the streamed dkv kernel runs (include/dosx.h)."""
    _attention_case(Sq, Bq, Nk, Bk, H, bcast, pkv, drop)


# Template boundaries of dosx_attention_fwd / _bwd (csrc/attention.hip), checked from both sides.  With the crystal-aligned
# kernels off (aligned mode 0): keys per lane of the row phases NJ = 1 (Nk <= 16), 3 (17..48), 4 (49..64), 13 (65..208),
# 20 (209..320), the general kernels beyond 320; the streamed dkv kernel's key group kg = 2 above 32 keys; QT = 32 query rows
# per workgroup (Sq 1 / 32 / 33).  LDS residency (fwd_smem / dq_smem against 160 KiB): the forward keeps every key chunk
# resident for all Nk <= 64 up to H 256 (H 256, Nk 64: 131 KiB) and never beyond 64 keys; the partial-dK/dV path fits for
# all Nk <= 64 up to H 256 (H 256, Nk 64: 147 KiB: pkv_supported) and never beyond; the dq kernel with it keeps the keys
# resident at H 128 (Nk 64: 104 KiB) and at H 256 up to 32 keys (157 KiB) but not from 33 keys (172 KiB); without it at every
# Nk <= 64.  Default mode: the forward of Nk <= 64 at H 64 / 128 / 256 runs csrc/attention_aligned.hip instead (keys padded to
# 16, 32 query rows per tile), and with pkv the one-launch backward (dkv_cnt) runs there too; elsewhere attention.hip's.
BOUNDARY_SHAPES = [
    (51, 4, 16, 4, 128, False),    # NJ 1, last
    (51, 4, 17, 4, 128, False),    # NJ 3, first
    (33, 3, 32, 3, 256, False),    # NJ 3, kg 1 (last), pkv dq resident at H 256 (last)
    (33, 3, 33, 3, 256, False),    # NJ 3, kg 2 (first), pkv dq NOT resident at H 256 (first)
    (32, 2, 48, 2, 64, False),     # NJ 3, last; one full query tile
    (51, 2, 49, 2, 64, False),     # NJ 4, first
    (70, 3, 64, 3, 128, False),    # NJ 4, last; pkv dq resident at H 128
    (70, 3, 64, 3, 256, False),    # NJ 4, last; pkv dq not resident at H 256
    (51, 2, 65, 2, 128, False),    # NJ 13, first: no pkv, no resident forward
    (20, 3, 208, 3, 64, False),    # NJ 13, last
    (20, 3, 209, 3, 64, False),    # NJ 20, first
    (9, 2, 320, 2, 128, False),    # NJ 20, last fused shape (MAX_FUSED_NK)
    (1, 4, 16, 2, 128, False),     # one query row, Bq = 2 Bk
    (1, 3, 64, 3, 256, False),     # one query row at H 256
    (32, 2, 33, 2, 128, False),    # exactly one query tile
    (33, 2, 48, 2, 16, False),     # H 16: never aligned
    (33, 2, 17, 1, 64, True),      # broadcast query rows, two query tiles
    (51, 6, 64, 3, 64, True),      # broadcast, Bq = 2 Bk, 64 keys
]


@pytest.mark.parametrize("Sq,Bq,Nk,Bk,H,bcast", BOUNDARY_SHAPES)
@pytest.mark.parametrize("drop", [0.0, 0.35])
@pytest.mark.parametrize("pkv", [False, True])
@pytest.mark.parametrize("mode", ["streamed", "default"])
def test_attention_fwd_bwd_at_template_boundaries(Sq, Bq, Nk, Bk, H, bcast, pkv, drop, mode):
    """test_attention_fwd_bwd's assertions at each side of the template boundaries: aligned mode 0 (attention.hip's streamed
    templates at every shape) and the default mode (the crystal-aligned kernels where they take the shape)."""
    from dostransformer_amd import _lib
    lib = _lib.load()
    assert bool(lib.dosx_attention_pkv_supported(Nk, H)) == (Nk <= 64)
    prev = lib.dosx_attention_aligned_mode(0 if mode == "streamed" else -1)
    try:
        _attention_case(Sq, Bq, Nk, Bk, H, bcast, pkv, drop, one_launch=(mode == "default"))
    finally:
        lib.dosx_attention_aligned_mode(prev)


def _attention_case(Sq, Bq, Nk, Bk, H, bcast, pkv, drop, one_launch=False):
    """one_launch: with the partial-dK/dV path, also hand the backward its crystal counters (DosxAttn.dkv_cnt)."""
    from dostransformer_amd import _lib
    pkv_path = pkv and bool(_lib.load().dosx_attention_pkv_supported(Nk, H))
    assert pkv_path or not pkv or Nk > 64
    o = ops()
    from dostransformer_amd._lib import Attn
    qs, qb = (1, 0) if bcast else (Bq, 1)
    xrows = Sq if bcast else Sq * Bq
    x = rnd(xrows, H, seed=1).double().requires_grad_(True)
    kv = rnd(Nk * Bk, H, seed=2)
    kv[-Bk:] = 0            # zero-padded atoms: LN gives beta on them
    kv = kv.double().requires_grad_(True)
    gam = rnd(H, seed=3).double().requires_grad_(True)
    bet = (0.3 * rnd(H, seed=4)).double().requires_grad_(True)
    mask = None
    if drop > 0:          # an arbitrary Bernoulli multiplier: the kernels take the mask as an operand
        mask = (torch.rand(Bq, Sq, Nk, generator=torch.Generator().manual_seed(9)) >= drop).float().to(DEV) / (1 - drop)
    ref, pref = _attn_ref(x, kv, gam, bet, Sq, Bq, Nk, Bk, H, qs, qb, None if mask is None else mask.double())
    dout = rnd(Sq * Bq, H, seed=5)
    ref.backward(dout.double())
    f = lambda t: t.detach().float().contiguous()
    a = Attn()
    a.Sq, a.Bq, a.Nk, a.Bk, a.H, a.q_stride_s, a.q_stride_b = Sq, Bq, Nk, Bk, H, qs, qb
    xf, kvf, gf, bf = f(x), f(kv), f(gam), f(bet)
    out = torch.empty(Sq * Bq, H, device=DEV)
    probs = torch.empty(Bq, Sq, Nk, device=DEV)
    qstats = torch.empty(Sq * Bq, 2, device=DEV)
    ostats = torch.empty(Sq * Bq, 2, device=DEV)
    a.x, a.kvhat, a.gamma0, a.beta0 = xf.data_ptr(), kvf.data_ptr(), gf.data_ptr(), bf.data_ptr()
    a.out, a.probs, a.qstats, a.out_stats = out.data_ptr(), probs.data_ptr(), qstats.data_ptr(), ostats.data_ptr()
    a.drop_mask = mask.data_ptr() if mask is not None else None
    o.attention_fwd(a)
    assert err(out, ref) < 3e-5
    assert err(probs, pref) < 3e-5
    assert err(ostats[:, 0], ref.detach().mean(1)) < 5e-5
    assert err(ostats[:, 1], 1 / torch.sqrt(ref.detach().var(1, unbiased=False) + 1e-5)) < 5e-5
    dx = torch.empty(Sq * Bq, H, device=DEV)
    dsc = torch.empty(Bq, Sq, Nk, device=DEV)
    dkv = torch.zeros(Nk * Bk, H, device=DEV)
    nqt, nkt = (Sq + 31) // 32, ((Nk + 15) // 16 if pkv_path else (Nk + 31) // 32)
    part = torch.empty(Bq * nqt + Bk * nkt, 2 * H, device=DEV)
    a.dout, a.dx, a.dscores, a.dkvhat, a.dkv_accumulate = dout.data_ptr(), dx.data_ptr(), dsc.data_ptr(), dkv.data_ptr(), 1
    a.partials_q = part.data_ptr()
    a.partials_kv = part.data_ptr() + 4 * Bq * nqt * 2 * H
    if pkv:
        kvp = torch.full((Bq * nqt * Nk, H), float("nan"), device=DEV)
        a.dkv_part = kvp.data_ptr()
    if pkv_path:
        a.dscores = None
        dkv += 0.5                           # accumulate flag: the reduction adds onto what is there
        if one_launch:
            a.dkv_cnt = o.COUNTERS.take(DEV, Bk)
    o.attention_bwd(a)
    if pkv_path:
        dkv -= 0.5
    elif pkv:
        torch.cuda.synchronize()
        assert bool(torch.isnan(kvp).all())  # the streamed dkv kernel ran: the partial-dKV scratch is untouched
    ps = part.double().sum(0)
    if bcast:
        dxr = dx.double().reshape(Sq, Bq, H).sum(1)
    else:
        dxr = dx
    assert err(dxr, x.grad) < 5e-5
    assert err(dkv, kv.grad) < 5e-5
    assert err(ps[:H], gam.grad) < 5e-5 and err(ps[H:], bet.grad) < 5e-5


def test_dropout_mask_kernel():
    from dostransformer_amd import ops
    n, p = 100003, 0.3
    seed = torch.tensor([0x1234567 + (5 << 40)], dtype=torch.int64, device=DEV)
    m = torch.empty(n, device=DEV)
    ops.dropout_mask(m, p, seed, 7)
    ref = _philox_mask_numpy(n, p, int(seed.item()), 7)
    assert np.array_equal(m.cpu().numpy(), ref)
    keep = float((m > 0).float().mean())
    assert abs(keep - (1 - p)) < 4 * (p * (1 - p) / n) ** 0.5 + 1e-3          # keep rate
    assert abs(float(m.mean()) - 1.0) < 0.01                                    # unbiased multiplier
    m2 = torch.empty(n, device=DEV)
    ops.dropout_mask(m2, p, seed, 7)
    assert torch.equal(m, m2)                                                   # same (seed, stream) -> same mask
    ops.dropout_mask(m2, p, seed, 8)
    assert not torch.equal(m, m2)                                               # another stream id -> another mask
    seed.add_(1)
    ops.dropout_mask(m2, p, seed, 7)
    assert not torch.equal(m, m2)                                               # bumped seed -> another mask
    z = torch.empty(1000, device=DEV)
    ops.dropout_mask(z, 0.0, seed, 0)
    assert bool((z == 1).all())


@pytest.mark.parametrize("mode", ["cross", "self"])
def test_transformer_encoder_attention_dropout_matches_oracle(mode):
    """TransformerEncoder(attn_dropout=0.3) in training mode: outputs and gradients equal the oracle's with the SAME
    Bernoulli draws (the masks the kernels used, captured per layer); eval mode ignores dropout; p = 0 is untouched."""
    from oracle import dos_oracle as O
    from dostransformer_amd import functional as Fn
    from dostransformer_amd.layers import TransformerEncoder
    torch.manual_seed(0)
    Hh, S, Bq, Nk, T = 32, 51, 5, 9, 2
    enc = TransformerEncoder(embed_dim=Hh, num_heads=1, layers=T, attn_dropout=0.3).to(DEV)
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(S, Bq, Hh, generator=gen).to(DEV).requires_grad_(True)
    kv = torch.randn(Nk, Bq, Hh, generator=gen).to(DEV).requires_grad_(True)
    w = torch.randn(S, Bq, Hh, generator=gen).to(DEV)
    Fn.DROP_MASK_LOG = []
    try:
        enc.train()
        y = enc(x, kv, kv) if mode == "cross" else enc(x, x, x)
        masks = [m.clone() for _, _, m in Fn.DROP_MASK_LOG]
    finally:
        Fn.DROP_MASK_LOG = None
    assert len(masks) == T and all(0.5 < float((m > 0).float().mean()) < 0.9 for m in masks)
    (y * w).sum().backward()
    p64 = {"e." + k: v.detach().double().cpu() for k, v in enc.state_dict().items() if v.is_floating_point()}
    x64 = x.detach().double().cpu().requires_grad_(True)
    kv64 = kv.detach().double().cpu().requires_grad_(True)
    m64 = [m.double().cpu() for m in masks]
    yr = O.transformer_encoder(p64, "e", x64, kv64 if mode == "cross" else x64, kv64 if mode == "cross" else x64, T, m64)
    (yr * w.double().cpu()).sum().backward()
    assert float((y.detach().cpu().double() - yr.detach()).abs().max()) < 2e-5
    assert float((x.grad.cpu().double() - x64.grad).abs().max() / x64.grad.abs().max()) < 1e-4
    if mode == "cross":
        assert float((kv.grad.cpu().double() - kv64.grad).abs().max() / kv64.grad.abs().max()) < 1e-4
    # a second training forward draws different masks; eval mode is deterministic and equals the p = 0 oracle
    y2 = enc(x, kv, kv) if mode == "cross" else enc(x, x, x)
    assert not torch.equal(y.detach(), y2.detach())
    enc.eval()
    with torch.no_grad():
        ye = enc(x, kv, kv) if mode == "cross" else enc(x, x, x)
        y0 = O.transformer_encoder(p64, "e", x64, kv64 if mode == "cross" else x64, kv64 if mode == "cross" else x64, T)
    assert float((ye.cpu().double() - y0.detach()).abs().max()) < 2e-5


@pytest.mark.parametrize("Sq,Bq,Nk,Bk,H", [(51, 4, 12, 4, 128), (51, 6, 9, 3, 64), (70, 3, 64, 3, 128), (51, 128, 51, 128, 128),
                                            (51, 128, 12, 64, 128), (201, 4, 41, 2, 256), (7, 3, 5, 3, 16)])
@pytest.mark.parametrize("drop", [0.0, 0.3])
def test_attention_backward_in_one_launch(Sq, Bq, Nk, Bk, H, drop):
    """DosxAttn.dkv_cnt: the key gradient finished by the last arriving query-tile workgroup of each crystal, inside the dq
    launch == the dq launch + attn_dkv_reduce_kernel, BITWISE (dx, dkvhat with the accumulate flag, both partial-sum
    blocks); repeated launches on the same counters reproduce it (the counters are back at zero)."""
    from dostransformer_amd import _lib
    from dostransformer_amd._lib import Attn
    if not _lib.load().dosx_attention_pkv_supported(Nk, H):
        pytest.skip("partial-dKV path covers Nk <= 64 where its tiles fit the LDS")
    o = ops()
    x, kv = rnd(Sq * Bq, H, seed=1), rnd(Nk * Bk, H, seed=2)
    gam, bet = rnd(H, seed=3), 0.3 * rnd(H, seed=4)
    mask = None
    if drop > 0:
        mask = (torch.rand(Bq, Sq, Nk, generator=torch.Generator().manual_seed(9)) >= drop).float().to(DEV) / (1 - drop)
    a = Attn()
    a.Sq, a.Bq, a.Nk, a.Bk, a.H, a.q_stride_s, a.q_stride_b = Sq, Bq, Nk, Bk, H, Bq, 1
    out, probs = torch.empty(Sq * Bq, H, device=DEV), torch.empty(Bq, Sq, Nk, device=DEV)
    qstats, ostats = torch.empty(Sq * Bq, 2, device=DEV), torch.empty(Sq * Bq, 2, device=DEV)
    a.x, a.kvhat, a.gamma0, a.beta0 = x.data_ptr(), kv.data_ptr(), gam.data_ptr(), bet.data_ptr()
    a.out, a.probs, a.qstats, a.out_stats = out.data_ptr(), probs.data_ptr(), qstats.data_ptr(), ostats.data_ptr()
    a.drop_mask = mask.data_ptr() if mask is not None else None
    o.attention_fwd(a)
    dout = rnd(Sq * Bq, H, seed=5)
    nqt, nkt = (Sq + 31) // 32, (Nk + 15) // 16
    base = rnd(Nk * Bk, H, seed=6)

    def run(fused):
        dx = torch.full((Sq * Bq, H), float("nan"), device=DEV)
        dkv = base.clone()
        part = torch.full((Bq * nqt + Bk * nkt, 2 * H), float("nan"), device=DEV)
        kvp = torch.full((Bq * nqt * Nk, H), float("nan"), device=DEV)
        a.dout, a.dx, a.dscores, a.dkvhat, a.dkv_accumulate = dout.data_ptr(), dx.data_ptr(), None, dkv.data_ptr(), 1
        a.partials_q, a.partials_kv = part.data_ptr(), part.data_ptr() + 4 * Bq * nqt * 2 * H
        a.dkv_part = kvp.data_ptr()
        a.dkv_cnt = o.COUNTERS.take(DEV, Bk) if fused else None
        reps = 3 if fused else 1
        outs = []
        for _ in range(reps):
            dkv.copy_(base)
            o.attention_bwd(a)
            torch.cuda.synchronize()
            outs.append((dx.clone(), dkv.clone(), part.clone()))
        for r in outs[1:]:
            assert all(torch.equal(u, v) for u, v in zip(r, outs[0]))
        return outs[0]

    # (round 5: hidden 256 with <= 64 keys takes csrc/attention_aligned.hip in the one-launch form - other tiles, other summation
    #  orders; this test is about attention.hip's two forms: keep both on those kernels)
    prev = _lib.load().dosx_attention_aligned_mode(0)
    try:
        two, one = run(False), run(True)
    finally:
        _lib.load().dosx_attention_aligned_mode(prev)
    for name, u, v in zip(("dx", "dkvhat", "partials"), two, one):
        assert not torch.isnan(v).any(), name
        assert torch.equal(u, v), name


@pytest.mark.parametrize("mode", ["cross", "self"])
@pytest.mark.parametrize("p_attn,p_relu,p_res", [(0.0, 0.3, 0.0), (0.0, 0.0, 0.2), (0.25, 0.3, 0.2)])
def test_transformer_encoder_relu_and_res_dropout_match_oracle(mode, p_attn, p_relu, p_res):
    """TransformerEncoder(relu_dropout, res_dropout) (`transformer.py:137,145-147`) in training mode: outputs and every
    gradient equal the oracle's with the SAME Bernoulli draws (the masks the kernels used, captured per layer and site);
    eval mode ignores them."""
    from oracle import dos_oracle as O
    from dostransformer_amd import functional as Fn
    from dostransformer_amd.layers import TransformerEncoder
    torch.manual_seed(0)
    Hh, S, Bq, Nk, T = 32, 51, 5, 9, 2
    enc = TransformerEncoder(embed_dim=Hh, num_heads=1, layers=T, attn_dropout=p_attn, relu_dropout=p_relu, res_dropout=p_res).to(DEV)
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if "layer_norm" in n or "bias" in n:
                p.add_(0.1 * torch.randn_like(p))
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(S, Bq, Hh, generator=gen).to(DEV).requires_grad_(True)
    kv = torch.randn(Nk, Bq, Hh, generator=gen).to(DEV).requires_grad_(True)
    w = torch.randn(S, Bq, Hh, generator=gen).to(DEV)
    Fn.DROP_MASK_LOG, Fn.FDROP_MASK_LOG = [], []
    try:
        enc.train()
        y = enc(x, kv, kv) if mode == "cross" else enc(x, x, x)
        amasks = [m.clone() for _, _, m in Fn.DROP_MASK_LOG]
        fmasks = [(t, k, m.clone()) for _, t, k, m in Fn.FDROP_MASK_LOG]
    finally:
        Fn.DROP_MASK_LOG = Fn.FDROP_MASK_LOG = None
    assert len(amasks) == (T if p_attn > 0 else 0)
    assert len(fmasks) == T * ((1 if p_relu > 0 else 0) + (2 if p_res > 0 else 0))
    (y * w).sum().backward()
    masks = [dict() for _ in range(T)]
    for t, m in enumerate(amasks):
        masks[t]["attn"] = m.double().cpu()
    for t, k, m in fmasks:
        assert 0.4 < float((m > 0).float().mean()) < 0.95
        masks[t][k] = m.double().cpu()
    p64 = {"e." + k: v.detach().double().cpu().requires_grad_(True) for k, v in enc.state_dict().items() if v.is_floating_point()}
    x64 = x.detach().double().cpu().requires_grad_(True)
    kv64 = kv.detach().double().cpu().requires_grad_(True)
    src = kv64 if mode == "cross" else x64
    yr = O.transformer_encoder(p64, "e", x64, src, src, T, masks)
    (yr * w.double().cpu()).sum().backward()
    assert float((y.detach().cpu().double() - yr.detach()).abs().max()) < 3e-5
    assert float((x.grad.cpu().double() - x64.grad).abs().max() / x64.grad.abs().max()) < 1e-4
    if mode == "cross":
        assert float((kv.grad.cpu().double() - kv64.grad).abs().max() / kv64.grad.abs().max()) < 1e-4
    for n, p in enc.named_parameters():
        if ".self_attn." in n:
            assert p.grad is None
            continue
        gr = p64["e." + n].grad
        assert float((p.grad.cpu().double() - gr).abs().max() / (gr.abs().max() + 1e-12)) < 2e-4, n
    y2 = enc(x, kv, kv) if mode == "cross" else enc(x, x, x)
    assert not torch.equal(y.detach(), y2.detach())                          # a new call draws new masks
    enc.eval()
    with torch.no_grad():
        ye = enc(x, kv, kv) if mode == "cross" else enc(x, x, x)
        y0 = O.transformer_encoder({k: v.detach() for k, v in p64.items()}, "e", x64.detach(), src.detach(), src.detach(), T)
    assert float((ye.cpu().double() - y0).abs().max()) < 3e-5


def test_multihead_attention_with_key_is_not_value():
    """`MultiheadAttention.forward(query, key, value)` with a value tensor that is not the key (`multihead_attention.py:49-76`
    takes any pair of equal shape; no reference call site does): outputs and the three input gradients against float64
    autograd of the same expression, with and without attention dropout (the mask the kernels used)."""
    from dostransformer_amd.layers.multihead_attention import MultiheadAttention
    torch.manual_seed(0)
    for H, S, B, Nk, p in ((32, 51, 4, 9, 0.0), (128, 20, 3, 70, 0.3), (16, 7, 2, 5, 0.0)):
        mha = MultiheadAttention(H, 1, attn_dropout=p).to(DEV).train()
        gen = torch.Generator().manual_seed(3)
        q = torch.randn(S, B, H, generator=gen).to(DEV).requires_grad_(True)
        k = torch.randn(Nk, B, H, generator=gen).to(DEV).requires_grad_(True)
        v = torch.randn(Nk, B, H, generator=gen).to(DEV).requires_grad_(True)
        w = torch.randn(S, B, H, generator=gen).to(DEV)
        out = mha(q, k, v)
        (out * w).sum().backward()
        m = mha.last_drop_mask.double() if p > 0 else None
        q2, k2, v2 = (t.detach().double().requires_grad_(True) for t in (q, k, v))
        a = torch.softmax(torch.bmm(q2.transpose(0, 1), k2.permute(1, 2, 0)) * H ** -0.5, -1)
        if m is not None:
            a = a * m
        ref = torch.bmm(a, v2.transpose(0, 1)).transpose(0, 1)
        (ref * w.double()).sum().backward()
        assert err(out.detach(), ref.detach()) < 3e-5
        for g_, r_ in ((q.grad, q2.grad), (k.grad, k2.grad), (v.grad, v2.grad)):
            assert err(g_, r_) < 5e-5
        assert mha.in_proj_weight.grad is None


@pytest.mark.parametrize("H,S,B,Nk", [(32, 51, 2, 400), (32, 20, 3, 1000), (256, 10, 2, 330), (128, 12, 3, 700), (512, 12, 2, 9)])
def test_layers_take_any_number_of_keys_and_wide_embeddings(H, S, B, Nk):
    """`layers.MultiheadAttention` and `layers.TransformerEncoder` called with the SAME tensor for keys and values (every
    reference call site) on shapes beyond the fused kernels - more than 320 keys (both modules), embed_dim 512 (attention module):
    the general path (scores by dosx_attn_dp, dosx_softmax_fwd, the K != V building blocks) against float64 autograd of
    `multihead_attention.py:62-74` and against the oracle's encoder, outputs and every gradient."""
    from oracle import dos_oracle as O
    from dostransformer_amd.layers import TransformerEncoder
    from dostransformer_amd.layers.multihead_attention import MultiheadAttention
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(5)
    mha = MultiheadAttention(H, 1).to(DEV)
    q = torch.randn(S, B, H, generator=gen).to(DEV).requires_grad_(True)
    kv = torch.randn(Nk, B, H, generator=gen).to(DEV).requires_grad_(True)
    w = torch.randn(S, B, H, generator=gen).to(DEV)
    out = mha(q, kv, kv)
    (out * w).sum().backward()
    q2, k2 = (t.detach().double().requires_grad_(True) for t in (q, kv))
    a = torch.softmax(torch.bmm(q2.transpose(0, 1), k2.permute(1, 2, 0)) * H ** -0.5, -1)
    ref = torch.bmm(a, k2.transpose(0, 1)).transpose(0, 1)
    (ref * w.double()).sum().backward()
    assert err(out.detach(), ref.detach()) < 3e-5
    assert err(q.grad, q2.grad) < 5e-5 and err(kv.grad, k2.grad) < 5e-5
    if H > 256:
        return                                             # (the encoder's row kernels stop at 256 columns: DESIGN.md §7)
    T = 2
    enc = TransformerEncoder(embed_dim=H, num_heads=1, layers=T).to(DEV)
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if "layer_norm" in n or "bias" in n:
                p.add_(0.1 * torch.randn_like(p))
    x = torch.randn(S, B, H, generator=gen).to(DEV).requires_grad_(True)
    k = torch.randn(Nk, B, H, generator=gen).to(DEV).requires_grad_(True)
    y = enc(x, k, k)
    (y * w).sum().backward()
    p64 = {"e." + n: t_.detach().double().cpu().requires_grad_(True) for n, t_ in enc.state_dict().items() if t_.is_floating_point()}
    x64, k64 = x.detach().double().cpu().requires_grad_(True), k.detach().double().cpu().requires_grad_(True)
    yr = O.transformer_encoder(p64, "e", x64, k64, k64, T)
    (yr * w.double().cpu()).sum().backward()
    assert float((y.detach().cpu().double() - yr.detach()).abs().max()) < 5e-5
    rel = lambda a_, b_: float((a_.cpu().double() - b_).abs().max() / (b_.abs().max() + 1e-12))
    assert rel(x.grad, x64.grad) < 1e-4 and rel(k.grad, k64.grad) < 1e-4
    for n, p in enc.named_parameters():
        if ".self_attn." in n:
            assert p.grad is None
        else:
            assert rel(p.grad, p64["e." + n].grad) < 2e-4, n


@pytest.mark.parametrize("case", ["kv_differ", "embed_dropout", "everything"])
def test_transformer_encoder_with_k_not_v_matches_oracle(case):
    """TransformerEncoder with x_in_k is not x_in_v, and with embed dropout (`transformer.py:61-68`: independent masks on the
    queries, keys and values - so K != V even when one tensor is passed for both): outputs and every gradient against the
    oracle with the same draws.  `everything`: all four dropouts at once on different key / value tensors."""
    from oracle import dos_oracle as O
    from dostransformer_amd import functional as Fn
    from dostransformer_amd.layers import TransformerEncoder
    torch.manual_seed(0)
    Hh, S, Bq, Nk, T = 32, 51, 4, 9, 2
    kw = {"kv_differ": {}, "embed_dropout": dict(embed_dropout=0.2),
          "everything": dict(embed_dropout=0.2, attn_dropout=0.25, relu_dropout=0.3, res_dropout=0.2)}[case]
    enc = TransformerEncoder(embed_dim=Hh, num_heads=1, layers=T, **kw).to(DEV).train()
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if "layer_norm" in n or "bias" in n:
                p.add_(0.1 * torch.randn_like(p))
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(S, Bq, Hh, generator=gen).to(DEV).requires_grad_(True)
    k = torch.randn(Nk, Bq, Hh, generator=gen).to(DEV).requires_grad_(True)
    v = torch.randn(Nk, Bq, Hh, generator=gen).to(DEV).requires_grad_(True)
    w = torch.randn(S, Bq, Hh, generator=gen).to(DEV)
    same = case == "embed_dropout"
    Fn.DROP_MASK_LOG, Fn.FDROP_MASK_LOG, Fn.EDROP_MASK_LOG = [], [], []
    try:
        y = enc(x, k, k) if same else enc(x, k, v)
        amasks = [m.clone() for _, _, m in Fn.DROP_MASK_LOG]
        fmasks = [(t, kk, m.clone()) for _, t, kk, m in Fn.FDROP_MASK_LOG]
        emasks = {n: m.clone() for _, n, m in Fn.EDROP_MASK_LOG}
    finally:
        Fn.DROP_MASK_LOG = Fn.FDROP_MASK_LOG = Fn.EDROP_MASK_LOG = None
    (y * w).sum().backward()
    assert (len(emasks) == 3) == ("embed_dropout" in kw)
    masks = [dict() for _ in range(T)]
    for t, m in enumerate(amasks):
        masks[t]["attn"] = m.double().cpu()
    for t, kk, m in fmasks:
        masks[t][kk] = m.double().cpu()
    p64 = {"e." + n: t_.detach().double().cpu().requires_grad_(True) for n, t_ in enc.state_dict().items() if t_.is_floating_point()}
    x64 = x.detach().double().cpu().requires_grad_(True)
    k64 = k.detach().double().cpu().requires_grad_(True)
    v64 = k64 if same else v.detach().double().cpu().requires_grad_(True)
    em = lambda t, n: t if n not in emasks else t * emasks[n].double().cpu().reshape(t.shape)
    yr = O.transformer_encoder(p64, "e", em(x64, "x"), em(k64, "k"), em(v64, "v"), T, masks)
    (yr * w.double().cpu()).sum().backward()
    assert float((y.detach().cpu().double() - yr.detach()).abs().max()) < 3e-5
    rel = lambda a, b: float((a.cpu().double() - b).abs().max() / (b.abs().max() + 1e-12))
    assert rel(x.grad, x64.grad) < 1e-4 and rel(k.grad, k64.grad) < 1e-4
    if not same:
        assert rel(v.grad, v64.grad) < 1e-4
    for n, p in enc.named_parameters():
        if ".self_attn." in n:
            assert p.grad is None
        else:
            assert rel(p.grad, p64["e." + n].grad) < 2e-4, n
    enc.eval()                                             # eval mode: no dropout anywhere; K != V still honoured
    with torch.no_grad():
        ye = enc(x, k, k) if same else enc(x, k, v)
        y0 = O.transformer_encoder({n: t_.detach() for n, t_ in p64.items()}, "e", x64.detach(), k64.detach(), v64.detach(), T)
    assert float((ye.cpu().double() - y0).abs().max()) < 3e-5


@pytest.mark.parametrize("Sq,Bq,Nk,Bk,H,bcast", [(201, 6, 41, 3, 256, False), (201, 5, 64, 5, 256, False), (51, 4, 12, 4, 128, False),
                                                   (51, 6, 9, 3, 64, False), (70, 3, 48, 3, 128, False), (33, 300, 17, 150, 64, False),
                                                   (201, 140, 16, 70, 128, False), (7, 3, 1, 3, 256, False), (51, 5, 7, 5, 128, True),
                                                   (64, 9, 33, 9, 256, True)])
@pytest.mark.parametrize("drop", [0.0, 0.35])
def test_attention_on_crystal_aligned_tiles(Sq, Bq, Nk, Bk, H, bcast, drop):
    """csrc/attention_aligned.hip behind dosx_attention_fwd / dosx_attention_bwd (one-launch form): <= 64 keys, hidden 64 / 128 /
    256, workgroups that own one, several (Bq = 140: 2 per crystal) or all (Bq = 300) query tiles of a crystal, broadcast query
    rows, dropout masks - against the float64 reference of multihead_attention.py:49-76 + the LayerNorm / residual around it;
    repeated launches bitwise equal (counters back at zero); with the mode switched off the same call takes attention.hip's
    kernels and agrees to rounding."""
    from tests.gpu_util import _attn_ref
    from dostransformer_amd import _lib
    from dostransformer_amd._lib import Attn
    o = ops()
    lib = _lib.load()
    qs, qb = (1, 0) if bcast else (Bq, 1)
    x = rnd(Sq if bcast else Sq * Bq, H, seed=1).double().requires_grad_(True)
    kv = rnd(Nk * Bk, H, seed=2)
    kv[-Bk:] = 0                        # zero-padded atoms
    kv = kv.double().requires_grad_(True)
    gam, bet = rnd(H, seed=3).double().requires_grad_(True), (0.3 * rnd(H, seed=4)).double().requires_grad_(True)
    mask = None
    if drop > 0:
        mask = (torch.rand(Bq, Sq, Nk, generator=torch.Generator().manual_seed(9)) >= drop).float().to(DEV) / (1 - drop)
    ref, pref = _attn_ref(x, kv, gam, bet, Sq, Bq, Nk, Bk, H, qs, qb, None if mask is None else mask.double())
    dout = rnd(Sq * Bq, H, seed=5)
    ref.backward(dout.double())
    f = lambda t: t.detach().float().contiguous()
    xf, kvf, gf, bf = f(x), f(kv), f(gam), f(bet)
    nqt, nkt = (Sq + 31) // 32, (Nk + 15) // 16
    base = rnd(Nk * Bk, H, seed=6)
    g1, b1 = 1 + 0.2 * rnd(H, seed=7), 0.3 * rnd(H, seed=8)

    def run(mode):
        prev = lib.dosx_attention_aligned_mode(mode)
        try:
            a = Attn()
            a.Sq, a.Bq, a.Nk, a.Bk, a.H, a.q_stride_s, a.q_stride_b = Sq, Bq, Nk, Bk, H, qs, qb
            out, probs = torch.full((Sq * Bq, H), float("nan"), device=DEV), torch.full((Bq, Sq, Nk), float("nan"), device=DEV)
            qstats, ostats = torch.full((Sq * Bq, 2), float("nan"), device=DEV), torch.full((Sq * Bq, 2), float("nan"), device=DEV)
            a.x, a.kvhat, a.gamma0, a.beta0 = xf.data_ptr(), kvf.data_ptr(), gf.data_ptr(), bf.data_ptr()
            a.out, a.probs, a.qstats, a.out_stats = out.data_ptr(), probs.data_ptr(), qstats.data_ptr(), ostats.data_ptr()
            a.drop_mask = mask.data_ptr() if mask is not None else None
            ln1 = torch.full((Sq * Bq, H), float("nan"), device=DEV)      # DosxAttn.ln1_*: the layer's next LayerNorm on the output rows
            a.ln1_gamma, a.ln1_beta, a.ln1_out = g1.data_ptr(), b1.data_ptr(), ln1.data_ptr()
            o.attention_fwd(a)
            assert err(ln1, torch.nn.functional.layer_norm(ref.detach(), (H,), g1.double(), b1.double(), 1e-5)) < 5e-5
            dx = torch.full((Sq * Bq, H), float("nan"), device=DEV)
            dkv = base.clone()
            part = torch.full((Bq * nqt + Bk * nkt, 2 * H), float("nan"), device=DEV)
            kvp = torch.full((Bq * nqt * Nk, H), float("nan"), device=DEV)
            a.dout, a.dx, a.dscores, a.dkvhat, a.dkv_accumulate = dout.data_ptr(), dx.data_ptr(), None, dkv.data_ptr(), 1
            a.partials_q, a.partials_kv = part.data_ptr(), part.data_ptr() + 4 * Bq * nqt * 2 * H
            a.dkv_part, a.dkv_cnt = kvp.data_ptr(), o.COUNTERS.take(DEV, Bk)
            outs = []
            for _ in range(2):
                dkv.copy_(base)
                o.attention_bwd(a)
                torch.cuda.synchronize()
                outs.append((dx.clone(), dkv.clone(), part.clone()))
            assert all(torch.equal(u, v) for u, v in zip(*outs))
            return out, probs, qstats, ostats, dx, dkv - base, part
        finally:
            lib.dosx_attention_aligned_mode(prev)

    new, old = run(2), run(0)
    for out, probs, qstats, ostats, dx, dkv, part in (new, old):
        assert err(out, ref) < 3e-5 and err(probs, pref) < 3e-5
        assert err(ostats[:, 0], ref.detach().mean(1)) < 5e-5
        assert err(ostats[:, 1], 1 / torch.sqrt(ref.detach().var(1, unbiased=False) + 1e-5)) < 5e-5
        ps = part.double().sum(0)
        dxr = dx.double().reshape(Sq, Bq, H).sum(1) if bcast else dx
        assert err(dxr, x.grad) < 5e-5 and err(dkv, kv.grad) < 5e-5
        assert err(ps[:H], gam.grad) < 5e-5 and err(ps[H:], bet.grad) < 5e-5
    assert err(new[2], old[2]) < 1e-5               # the LayerNorm-0 statistics of the query rows


@pytest.mark.parametrize("Sq,Bq,Nk,H", [(201, 3, 201, 256), (70, 3, 70, 128), (51, 4, 12, 128)])
def test_attention_forward_also_writes_the_next_layernorm(Sq, Bq, Nk, H):
    """DosxAttn.ln1_out on attention.hip's kernels (more than 64 keys: the 201-key Electron-DOS self attention; mode 0 for the
    small shape): LN1 of the output rows == F.layer_norm of the rows the same call writes; refused beyond 320 keys."""
    from dostransformer_amd import _lib
    from dostransformer_amd._lib import Attn, DosxError
    o = ops()
    lib = _lib.load()
    x, kv, gam, bet = rnd(Sq * Bq, H, seed=1), rnd(Nk * Bq, H, seed=2), rnd(H, seed=3), 0.3 * rnd(H, seed=4)
    g1, b1 = 1 + 0.2 * rnd(H, seed=7), 0.3 * rnd(H, seed=8)
    a = Attn()
    a.Sq, a.Bq, a.Nk, a.Bk, a.H, a.q_stride_s, a.q_stride_b = Sq, Bq, Nk, Bq, H, Bq, 1
    out, probs = torch.empty(Sq * Bq, H, device=DEV), torch.empty(Bq, Sq, Nk, device=DEV)
    qstats, ostats = torch.empty(Sq * Bq, 2, device=DEV), torch.empty(Sq * Bq, 2, device=DEV)
    ln1 = torch.full((Sq * Bq, H), float("nan"), device=DEV)
    a.x, a.kvhat, a.gamma0, a.beta0 = x.data_ptr(), kv.data_ptr(), gam.data_ptr(), bet.data_ptr()
    a.out, a.probs, a.qstats, a.out_stats = out.data_ptr(), probs.data_ptr(), qstats.data_ptr(), ostats.data_ptr()
    a.ln1_gamma, a.ln1_beta, a.ln1_out = g1.data_ptr(), b1.data_ptr(), ln1.data_ptr()
    prev = lib.dosx_attention_aligned_mode(0)
    try:
        o.attention_fwd(a)
    finally:
        lib.dosx_attention_aligned_mode(prev)
    assert err(ln1, torch.nn.functional.layer_norm(out.double(), (H,), g1.double(), b1.double(), 1e-5)) < 2e-5
    a.Nk = 330
    big_kv, big_p = rnd(330 * Bq, H, seed=2), torch.empty(Bq, Sq, 330, device=DEV)
    a.kvhat, a.probs = big_kv.data_ptr(), big_p.data_ptr()
    with pytest.raises(DosxError, match="ln1_out"):
        o.attention_fwd(a)


# (Sq, Bq, Nk, Bk, H) and the forms that take the shape: "two" = attention.hip, dq launch + attn_dkv_reduce_kernel; "one" =
# attention.hip, the dq launch's last arriver; "aligned" = csrc/attention_aligned.hip (hidden 64 / 128 / 256 only).  64 is the
# largest Nk <= 64 with dosx_attention_pkv_supported(Nk, 256), so attention.hip's forms run the last shape as it stands.
_DKV_REDUCE_SHAPES = [
    ((33, 3, 1, 3, 32), ("two", "one")),               # one key; lanes with c >= H
    ((70, 6, 17, 2, 96), ("two", "one")),              # 9 shares: a ragged last round; second row group with one row; half a column block
    ((7, 4, 16, 1, 64), ("two", "one", "aligned")),    # 4 shares: exactly one round
    ((40, 2, 33, 2, 128), ("two", "one", "aligned")),  # first row of the second row-per-slot
    ((65, 150, 64, 5, 64), ("two", "one", "aligned")),  # aligned: 1 workgroup for 3 tiles per query batch entry, 30 of them per crystal
    ((65, 5, 64, 5, 256), ("two", "one", "aligned")),  # aligned: NG 4, two shares per round, odd share count
]


@pytest.mark.parametrize("per_crystal", [False, True], ids=["all_keys", "key_ptr"])
@pytest.mark.parametrize("accumulate", [0, 1], ids=["fresh", "accumulate"])
@pytest.mark.parametrize("shape,form", [(s, f) for s, fs in _DKV_REDUCE_SHAPES for f in fs],
                         ids=[f"{'x'.join(map(str, s))}-{f}" for s, fs in _DKV_REDUCE_SHAPES for f in fs])
def test_key_gradient_is_the_sum_of_the_published_shares(shape, form, accumulate, per_crystal):
    """The key-gradient reduction alone (csrc/dkv_reduce.h), apart from the tile arithmetic: dkv_part starts as NaN, so after
    dosx_attention_bwd a [Nk, H] slot that is still all NaN was not published, and with key_ptr the rows >= n of a published
    slot are still NaN.  In float64, d[j] = sum of the published shares of key row j; then
        dkvhat[j] = base * accumulate + d[j] * gamma0,   partials_kv[bk][g] = [sum_{j in g} d[j] * k^[j] | sum_{j in g} d[j]],
    each element within (n_addends + 2) * 2^-23 * sum |addends| (n_addends fp32 values are summed into it: sequential fp32
    sums of n terms are off by at most (n - 1) 2^-24 sum |terms|, one more rounding each for the product and the base), and the
    rows >= n exactly 0.0 (fresh) or exactly base (accumulate)."""
    from dostransformer_amd import _lib
    from dostransformer_amd._lib import Attn
    Sq, Bq, Nk, Bk, H = shape
    lib, o = _lib.load(), ops()
    assert lib.dosx_attention_pkv_supported(Nk, H)
    x, kv = rnd(Sq * Bq, H, seed=1), rnd(Nk * Bk, H, seed=2)
    gam, bet = rnd(H, seed=3), 0.3 * rnd(H, seed=4)
    dout, base = rnd(Sq * Bq, H, seed=5), rnd(Nk * Bk, H, seed=6)
    counts = [Nk] * Bk
    kp = None
    if per_crystal:
        choices = sorted({min(c, Nk) for c in (0, 1, 16, 17, Nk)})
        counts = [choices[(len(choices) - 2 - bk) % len(choices)] for bk in range(Bk)]
        kp = torch.tensor([0] + list(np.cumsum(counts)), dtype=torch.int32, device=DEV)
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    nqt, ng = (Sq + 31) // 32, (Nk + 15) // 16
    a = Attn()
    a.Sq, a.Bq, a.Nk, a.Bk, a.H, a.q_stride_s, a.q_stride_b = Sq, Bq, Nk, Bk, H, Bq, 1
    out, probs, qstats, ostats = nan(Sq * Bq, H), nan(Bq, Sq, Nk), nan(Sq * Bq, 2), nan(Sq * Bq, 2)
    a.x, a.kvhat, a.gamma0, a.beta0 = x.data_ptr(), kv.data_ptr(), gam.data_ptr(), bet.data_ptr()
    a.out, a.probs, a.qstats, a.out_stats = out.data_ptr(), probs.data_ptr(), qstats.data_ptr(), ostats.data_ptr()
    a.key_ptr = kp.data_ptr() if kp is not None else None
    dx, dkv, part, kvp = nan(Sq * Bq, H), (base.clone() if accumulate else nan(Nk * Bk, H)), nan(Bq * nqt + Bk * ng, 2 * H), nan(Bq * nqt * Nk, H)
    a.dout, a.dx, a.dscores, a.dkvhat, a.dkv_accumulate = dout.data_ptr(), dx.data_ptr(), None, dkv.data_ptr(), accumulate
    a.partials_q, a.partials_kv = part.data_ptr(), part.data_ptr() + 4 * Bq * nqt * 2 * H
    a.dkv_part = kvp.data_ptr()
    a.dkv_cnt = None if form == "two" else o.COUNTERS.take(DEV, Bk)
    prev = lib.dosx_attention_aligned_mode(2 if form == "aligned" else 0)
    try:
        o.attention_fwd(a)
        o.attention_bwd(a)
        torch.cuda.synchronize()
    finally:
        lib.dosx_attention_aligned_mode(prev)
    # ---- the shares the launch published ----
    rep = Bq // Bk
    S = kvp.reshape(Bq, nqt, Nk, H).double()
    blank = torch.isnan(S)
    pub = ~blank.all(3).all(2)                                              # [Bq, nqt]
    n_q = torch.tensor(counts, device=DEV).repeat(rep)                      # keys of query batch entry bq = bk + i Bk
    live = torch.arange(Nk, device=DEV)[None, :] < n_q[:, None]             # [Bq, Nk]
    assert torch.equal(~blank, (pub[:, :, None, None] & live[:, None, :, None]).expand_as(blank))
    assert bool(pub.any(1)[n_q > 0].all()) and not bool(pub[n_q == 0].any())
    if form != "aligned":
        assert bool(pub[n_q > 0].all())                                     # one share per query tile
    S = torch.where(blank, torch.zeros_like(S), S).reshape(rep, Bk, nqt, Nk, H)
    d, dabs = S.sum((0, 2)), S.abs().sum((0, 2))                            # [Bk, Nk, H]
    nsh = pub.reshape(rep, Bk, nqt).sum((0, 2)).double()                    # shares per crystal
    u = 2.0 ** -23
    # ---- dkvhat ----
    g64, b64 = gam.double(), base.reshape(Nk, Bk, H).double().transpose(0, 1)
    got = dkv.reshape(Nk, Bk, H).double().transpose(0, 1)                   # [Bk, Nk, H]
    want = b64 * accumulate + d * g64
    bound = (nsh[:, None, None] + accumulate + 2) * u * (dabs * g64.abs() + b64.abs() * accumulate)
    excess = ((got - want).abs() - bound).max().item()
    rows_past = ~live[:Bk]                                                  # [Bk, Nk]
    print(f"dkvhat: max |err| {float((got - want).abs().max()):.3e}, max bound {float(bound.max()):.3e}, shares/crystal {nsh.tolist()}")
    assert not torch.isnan(got).any() and excess <= 0, excess
    assert torch.equal(got[rows_past], (b64 * accumulate)[rows_past])
    # ---- partials_kv ----
    k64 = kv.reshape(Nk, Bk, H).double().transpose(0, 1)
    pad = lambda t: torch.cat([t, torch.zeros(Bk, ng * 16 - Nk, H, device=DEV, dtype=torch.float64)], 1).reshape(Bk, ng, 16, H)
    want_p = torch.cat([pad(d * k64).sum(2), pad(d).sum(2)], 2)             # [Bk, ng, 2H]
    abs_p = torch.cat([pad(dabs * k64.abs()).sum(2), pad(dabs).sum(2)], 2)
    rows_g = torch.cat([live[:Bk], torch.zeros(Bk, ng * 16 - Nk, dtype=torch.bool, device=DEV)], 1).reshape(Bk, ng, 16).sum(2).double()
    bound_p = (nsh[:, None, None] * rows_g[:, :, None] + 2) * u * abs_p
    got_p = part[Bq * nqt:].reshape(Bk, ng, 2 * H).double()
    print(f"partials_kv: max |err| {float((got_p - want_p).abs().max()):.3e}, max bound {float(bound_p.max()):.3e}")
    assert not torch.isnan(got_p).any() and ((got_p - want_p).abs() - bound_p).max().item() <= 0
