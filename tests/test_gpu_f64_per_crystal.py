"""Per-crystal keys of the float64 DOSTransformer_phonon on a real MI355X (DosxAttn64.key_ptr, set_per_crystal_keys): the
attention kernels against float64 torch restricted to each crystal's own keys, and the model on a batch of crystals against
the float64 oracle run on every crystal alone - what the reference computes at batch_size = 1 (main_phDOS.py:52-55)."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.util import rmse

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
NAN = float("nan")


def _ops():
    from dostransformer_amd import ops
    return ops


def _r(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).to(DEV)


def _dy(*shape, seed=0, lo=-4, hi=5, den=4.0):
    """dyadic values: products and sums of a few of them are exact in fp64 and representable in fp32"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(lo, hi, shape, generator=g).double() / den).to(DEV)


def _mask(Bq, Sq, Nk, seed):
    g = torch.Generator().manual_seed(seed)
    keep = torch.rand(Bq, Sq, Nk, generator=g) >= 0.25
    return (keep.float() * torch.tensor(1.0 / 0.75, dtype=torch.float32)).to(DEV)


def _key_ptr(counts):
    kp = torch.zeros(len(counts) + 1, dtype=torch.int32)
    kp[1:] = torch.cumsum(torch.tensor(counts), 0)
    return kp.to(DEV)


def _dead(counts, Bq, Nk):
    """[Bq, 1, Nk] bool: key j does not exist for query crystal bq (j >= n of key crystal bq % Bk)"""
    n = torch.tensor(counts, device=DEV)[torch.arange(Bq, device=DEV) % len(counts)]
    return (torch.arange(Nk, device=DEV)[None, :] >= n[:, None])[:, None, :]


def _dead_rows(counts, Nk):
    """[Bk * Nk] bool: key row bk * Nk + j with j >= n"""
    n = torch.tensor(counts, device=DEV)
    return (torch.arange(Nk, device=DEV)[None, :] >= n[:, None]).reshape(-1)


def _all_zero(t):
    return torch.equal(t, torch.zeros_like(t))


def _ref_attention(q, x, kvhat, g0, b0, Sq, Bq, Nk, Bk, counts, mask, soft64):
    """float64 torch with the reference's numerics (multihead_attention.py:68-72), crystal by crystal over the keys [0, n) of
    its key crystal only; autograd gives the backward.  -> (out [Bq*Sq, H], p [Bq, Sq, Nk] with zeros past n)"""
    H = q.shape[1]
    kall = (kvhat * g0 + b0).view(Bk, Nk, H)
    outs, ps = [], []
    for bq in range(Bq):
        n = counts[bq % Bk]
        k = kall[bq % Bk, :n]
        qb = q.view(Bq, Sq, H)[bq]
        sc = qb @ k.t() * (H ** -0.5)
        p = F.softmax(sc, -1) if soft64 else F.softmax(sc.float(), -1).type_as(sc)
        pd = p if mask is None else p * mask[bq, :, :n].to(p.dtype)
        outs.append(x.view(Bq, Sq, H)[bq] + pd @ k)
        ps.append(F.pad(p, (0, Nk - n)))
    return torch.cat(outs), torch.stack(ps)


def _bound(got, ref, scale, k=1e-13):
    err = (got - ref).abs()
    ok = bool((err <= k * scale + 1e-300).all())
    return ok, float((err / (scale + 1e-300)).max())


# (Sq, Bq, Nk, Bk, H, counts): partial query and key tiles; a one-key crystal and a full one; counts on both sides of a 16-key
# tile edge; more than 64 keys and more than one dkv workgroup per crystal (130 keys: 9 tiles, 3 workgroups); Bq = 2 Bk
CASES = [(17, 4, 21, 2, 24, [1, 21]), (51, 6, 37, 3, 40, [16, 17, 37]), (5, 2, 130, 2, 64, [3, 129])]
IDS = ["n1_21", "n16_17_37", "n3_129"]


@pytest.mark.parametrize("Sq,Bq,Nk,Bk,H,counts", CASES, ids=IDS)
def test_attention_f64_key_ptr_exact_mode(Sq, Bq, Nk, Bk, H, counts):
    """fp64 softmax: out, probs, dq, ds, dkvhat, dgamma0 and dbeta0 within 1e-13 of their operand scale (the
    _bound rule of test_attention_f64_exact_mode, the abs-valued sums taken over the live keys only); everything past a
    crystal's keys exactly zero (dkvhat: left alone when accumulating).  Mask on / off, accumulate on / off."""
    ops = _ops()
    q, x = _r(Bq * Sq, H, seed=1), _r(Bq * Sq, H, seed=2)
    kvhat = _r(Bk * Nk, H, seed=3)                           # the rows past n hold numbers too: they must not matter
    g0, b0 = _r(H, seed=4, scale=0.5) + 1.0, _r(H, seed=5, scale=0.3)
    dout = _r(Bq * Sq, H, seed=6)
    kp = _key_ptr(counts)
    dead, dead_rows = _dead(counts, Bq, Nk), _dead_rows(counts, Nk)
    live = (~dead).double()
    c = H ** -0.5
    for use_mask in (False, True):
        mask = _mask(Bq, Sq, Nk, 7) if use_mask else None
        out, probs = ops.attention64(q, x, kvhat, g0, b0, Sq, Bq, Nk, Bk, mask, softmax64=True, key_ptr=kp)
        out2, probs2 = ops.attention64(q, x, kvhat, g0, b0, Sq, Bq, Nk, Bk, mask, softmax64=True, key_ptr=kp)
        assert torch.equal(out, out2) and torch.equal(probs, probs2)
        assert _all_zero(probs.masked_select(dead))
        qq, kk, gg, bb = (t.clone().requires_grad_(True) for t in (q, kvhat, g0, b0))
        ref, p = _ref_attention(qq, x, kk, gg, bb, Sq, Bq, Nk, Bk, counts, mask, True)
        ref.backward(dout)
        p = p.detach()
        assert _all_zero(kk.grad[dead_rows])
        # abs-valued operand scales over the live keys
        kab = (kvhat.abs() * g0.abs() + b0.abs()).view(Bk, Nk, H)[torch.arange(Bq, device=DEV) % Bk] * live.transpose(1, 2)
        m_ab = torch.ones_like(probs) if mask is None else mask.double()
        s_ab = q.abs().view(Bq, Sq, H) @ kab.transpose(1, 2) * c
        p_sc = p * (1.0 + s_ab)
        out_sc = x.abs() + ((p_sc * m_ab) @ kab).reshape(Bq * Sq, H)
        ok, worst = _bound(out, ref.detach(), out_sc)
        assert ok, ("out", worst)
        ok, worst = _bound(probs, p, p_sc)
        assert ok, ("probs", worst)
        dP_ab = dout.abs().view(Bq, Sq, H) @ kab.transpose(1, 2)
        g_ab = dP_ab * m_ab
        ds_sc = p_sc * (g_ab + (p * g_ab).sum(-1, keepdim=True)) * c
        dq_sc = (ds_sc @ kab).reshape(Bq * Sq, H)
        sel = lambda t: t.view(Bq // Bk, Bk, Sq, -1).transpose(0, 1).reshape(Bk, (Bq // Bk) * Sq, -1)
        dkv_sc = (sel(ds_sc).transpose(1, 2) @ sel(q.abs().view(Bq, Sq, H)) +
                  sel(p_sc * m_ab).transpose(1, 2) @ sel(dout.abs().view(Bq, Sq, H))).reshape(Bk * Nk, H)
        # ds against autograd of the scaled scores: dS = p (g - sum p g) c with g = (dout . k^T) o mask, live keys only
        kref = (kvhat * g0 + b0).view(Bk, Nk, H)[torch.arange(Bq, device=DEV) % Bk] * live.transpose(1, 2)
        g_ref = dout.view(Bq, Sq, H) @ kref.transpose(1, 2) * m_ab
        ds_ref = p * (g_ref - (p * g_ref).sum(-1, keepdim=True)) * c
        for acc in (False, True):
            base = _r(Bk * Nk, H, seed=8)
            dkv = base.clone()
            dq, part, ds = ops.attention_bwd64(dout, q, kvhat, g0, b0, probs, Sq, Bq, Nk, Bk, dkv, mask, softmax64=True,
                                               accumulate=acc, key_ptr=kp)
            dkv2 = base.clone()
            r2 = ops.attention_bwd64(dout, q, kvhat, g0, b0, probs, Sq, Bq, Nk, Bk, dkv2, mask, softmax64=True, accumulate=acc,
                                     key_ptr=kp)
            assert torch.equal(dq, r2[0]) and torch.equal(part, r2[1]) and torch.equal(ds, r2[2]) and torch.equal(dkv, dkv2)
            assert _all_zero(ds.masked_select(dead))
            assert _all_zero(part[dead_rows])
            if acc:
                assert torch.equal(dkv[dead_rows], base[dead_rows])
            else:
                assert _all_zero(dkv[dead_rows])
            ok, worst = _bound(dq, qq.grad, dq_sc)
            assert ok, ("dq", worst)
            ok, worst = _bound(ds, ds_ref, ds_sc)
            assert ok, ("ds", worst)
            want = kk.grad + (base if acc else 0.0)
            ok, worst = _bound(dkv, want, dkv_sc * g0.abs() + (base.abs() if acc else 0.0))
            assert ok, ("dkvhat", acc, worst)
            dg = torch.zeros(H, dtype=torch.float64, device=DEV)
            db = torch.zeros(H, dtype=torch.float64, device=DEV)
            ops.colsum64(part[:, :H], dg)
            ops.colsum64(part[:, H:], db)
            ok, worst = _bound(dg, gg.grad, (dkv_sc * kvhat.abs()).sum(0))
            assert ok, ("dgamma0", worst)
            ok, worst = _bound(db, bb.grad, dkv_sc.sum(0))
            assert ok, ("dbeta0", worst)


@pytest.mark.parametrize("Sq,Bq,Nk,Bk,H,counts", CASES, ids=IDS)
def test_attention_f64_key_ptr_reference_softmax(Sq, Bq, Nk, Bk, H, counts):
    """Reference mode with the dyadic operands and the unit counts of test_attention_f64_reference_softmax, the crystal's own
    n in the place of Nk: probs within (11 + d_gpu + n) units of 2^-24 p, ds within (4 + d_gpu + n + 1) units of
    p (|g| + sum p |g|) H^-1/2, d_gpu = ceil(n / 64) - 1 + 6.  (The dyadic dot products are exact in fp64 and both sides
    multiply them by the same double H^-1/2, so both round the same fp32 scores for every H.)"""
    ops = _ops()
    q, x = _dy(Bq * Sq, H, seed=1), _r(Bq * Sq, H, seed=2)
    kvhat = _dy(Bk * Nk, H, seed=3)
    g0, b0 = _dy(H, seed=4, lo=2, hi=5, den=2.0), _dy(H, seed=5, lo=-2, hi=3)
    dout = _dy(Bq * Sq, H, seed=6)
    kp = _key_ptr(counts)
    dead = _dead(counts, Bq, Nk)
    kall = (kvhat * g0 + b0).view(Bk, Nk, H)
    for use_mask in (False, True):
        mask = _mask(Bq, Sq, Nk, 7) if use_mask else None
        out, probs = ops.attention64(q, x, kvhat, g0, b0, Sq, Bq, Nk, Bk, mask, key_ptr=kp)
        _, p_ref = _ref_attention(q, x, kvhat, g0, b0, Sq, Bq, Nk, Bk, counts, mask, False)
        assert _all_zero(probs.masked_select(dead))
        assert torch.equal(probs, probs.float().double())                  # promoted fp32 values
        dkv = torch.zeros(Bk * Nk, H, dtype=torch.float64, device=DEV)
        dq, part, ds = ops.attention_bwd64(dout, q, kvhat, g0, b0, probs, Sq, Bq, Nk, Bk, dkv, mask, key_ptr=kp)
        assert _all_zero(ds.masked_select(dead))
        for bq in range(Bq):
            n = counts[bq % Bk]
            d_gpu = math.ceil(n / 64) - 1 + 6
            c = 11 + d_gpu + n
            ok, worst = _bound(probs[bq, :, :n], p_ref[bq, :, :n], p_ref[bq, :, :n], k=c * U)
            print(f"bq {bq} n {n} probs: worst {worst / U:.2f} units of 2^-24 p (c = {c})")
            assert ok, ("probs", bq, worst / U)
            g = dout.view(Bq, Sq, H)[bq] @ kall[bq % Bk, :n].t()
            if mask is not None:
                g = g * mask[bq, :, :n].double()
            pb = probs[bq, :, :n]
            ds_ref = torch._softmax_backward_data(g.float(), pb.float(), -1, torch.float32).double() * (H ** -0.5)
            scale = pb * (g.abs() + (pb * g.abs()).sum(-1, keepdim=True)) * (H ** -0.5)
            c = 4 + d_gpu + n + 1
            ok, worst = _bound(ds[bq, :, :n], ds_ref, scale, k=c * U)
            print(f"bq {bq} n {n} ds: worst {worst / U:.2f} units (c = {c})")
            assert ok, ("ds", bq, worst / U)


def _raw(ops, q, x, kvhat, g0, b0, dout, Sq, Bq, Nk, Bk, mask, soft64, kp, acc, base, fill):
    """Forward + backward on output buffers prefilled with ``fill`` (ops.attention64 / attention_bwd64 allocate theirs with
    torch.empty): -> out, probs, dq, ds, part, dkvhat"""
    H = q.shape[1]
    full = lambda *s: torch.full(s, fill, dtype=torch.float64, device=DEV)
    out, probs, dq = full(Bq * Sq, H), full(Bq, Sq, Nk), full(Bq * Sq, H)
    ds, part = full(Bq, Sq, Nk), full(Bk * Nk, 2 * H)
    dkv = base.clone() if acc else full(Bk * Nk, H)
    d = ops._attn64_desc(q, kvhat, g0, b0, Sq, Bq, Nk, Bk, mask, soft64, kp)
    d.x, d.out, d.probs = x.data_ptr(), out.data_ptr(), probs.data_ptr()
    ops._call("dosx_attention_f64", ops.C.byref(d), ops._stream())
    d.dout, d.dq, d.ds = dout.data_ptr(), dq.data_ptr(), ds.data_ptr()
    d.dkvhat, d.part, d.accumulate = dkv.data_ptr(), part.data_ptr(), int(acc)
    ops._call("dosx_attention_bwd_f64", ops.C.byref(d), ops._stream())
    torch.cuda.synchronize()
    return out, probs, dq, ds, part, dkv


@pytest.mark.parametrize("soft64", [True, False], ids=["exact", "reference"])
@pytest.mark.parametrize("Sq,Bq,Nk,Bk,H,counts", CASES, ids=IDS)
def test_attention_f64_key_ptr_nan_padding(Sq, Bq, Nk, Bk, H, counts, soft64):
    """Nothing past a crystal's keys is read and everything there is written: NaN in the kvhat rows >= n, in
    drop_mask[..., n:] and in every output buffer beforehand gives bitwise what zero padding gives, and no NaN anywhere."""
    ops = _ops()
    q, x = _r(Bq * Sq, H, seed=1), _r(Bq * Sq, H, seed=2)
    kvhat = _r(Bk * Nk, H, seed=3)
    g0, b0 = _r(H, seed=4, scale=0.5) + 1.0, _r(H, seed=5, scale=0.3)
    dout = _r(Bq * Sq, H, seed=6)
    base = _r(Bk * Nk, H, seed=8)
    mask = _mask(Bq, Sq, Nk, 7)
    kp = _key_ptr(counts)
    dead, dead_rows = _dead(counts, Bq, Nk), _dead_rows(counts, Nk)
    kv0, kvn = kvhat.clone(), kvhat.clone()
    kv0[dead_rows] = 0.0
    kvn[dead_rows] = NAN
    mn = torch.where(dead.expand_as(mask), torch.full_like(mask, NAN), mask).contiguous()
    for acc in (False, True):
        want = _raw(ops, q, x, kv0, g0, b0, dout, Sq, Bq, Nk, Bk, mask, soft64, kp, acc, base, 0.0)
        got = _raw(ops, q, x, kvn, g0, b0, dout, Sq, Bq, Nk, Bk, mn, soft64, kp, acc, base, NAN)
        for name, a, b in zip(("out", "probs", "dq", "ds", "part", "dkvhat"), got, want):
            assert not bool(torch.isnan(a).any()), (name, acc)
            assert torch.equal(a, b), (name, acc)
        # ... and the zero-padded call through the public wrappers is the same
        out, probs = ops.attention64(q, x, kv0, g0, b0, Sq, Bq, Nk, Bk, mask, softmax64=soft64, key_ptr=kp)
        dkv = base.clone()
        dq, part, ds = ops.attention_bwd64(dout, q, kv0, g0, b0, probs, Sq, Bq, Nk, Bk, dkv, mask, softmax64=soft64,
                                           accumulate=acc, key_ptr=kp)
        assert torch.equal(out, got[0]) and torch.equal(probs, got[1]) and torch.equal(dq, got[2])
        assert torch.equal(ds, got[3]) and torch.equal(part, got[4])
        if acc:
            assert torch.equal(dkv, got[5])
        else:
            assert torch.equal(dkv[~dead_rows], got[5][~dead_rows]) and _all_zero(dkv[dead_rows])


@pytest.mark.parametrize("soft64", [True, False], ids=["exact", "reference"])
@pytest.mark.parametrize("Sq,Bq,Nk,Bk,H,counts", CASES, ids=IDS)
def test_attention_f64_full_key_ptr_is_bitwise_no_key_ptr(Sq, Bq, Nk, Bk, H, counts, soft64):
    ops = _ops()
    q, x = _r(Bq * Sq, H, seed=1), _r(Bq * Sq, H, seed=2)
    kvhat = _r(Bk * Nk, H, seed=3)
    g0, b0 = _r(H, seed=4, scale=0.5) + 1.0, _r(H, seed=5, scale=0.3)
    dout = _r(Bq * Sq, H, seed=6)
    base = _r(Bk * Nk, H, seed=8)
    mask = _mask(Bq, Sq, Nk, 7)
    res = []
    for kp in (None, _key_ptr([Nk] * Bk)):
        out, probs = ops.attention64(q, x, kvhat, g0, b0, Sq, Bq, Nk, Bk, mask, softmax64=soft64, key_ptr=kp)
        for acc in (False, True):
            dkv = base.clone()
            dq, part, ds = ops.attention_bwd64(dout, q, kvhat, g0, b0, probs, Sq, Bq, Nk, Bk, dkv, mask, softmax64=soft64,
                                               accumulate=acc, key_ptr=kp)
            res += [dq, part, ds, dkv]
        res += [out, probs]
    half = len(res) // 2
    for a, b in zip(res[:half], res[half:]):
        assert torch.equal(a, b)


def test_attention_f64_key_ptr_empty_crystal_clamp_and_checks():
    """n = 0: out = x bitwise, zero probs / dq / ds / part / dkvhat, nothing divides by zero; a count above Nk is clamped to Nk;
    the wrappers refuse a key_ptr that is not an int32 device tensor of Bk + 1 entries."""
    ops = _ops()
    Sq, Bq, Nk, Bk, H = 5, 4, 7, 2, 16
    q, x = _r(Bq * Sq, H, seed=1), _r(Bq * Sq, H, seed=2)
    kvhat = _r(Bk * Nk, H, seed=3)
    g0, b0 = _r(H, seed=4, scale=0.5) + 1.0, _r(H, seed=5, scale=0.3)
    dout = _r(Bq * Sq, H, seed=6)
    for soft64 in (True, False):
        res = []
        for counts in ([0, 7], [0, 9]):
            kp = _key_ptr(counts)
            out, probs = ops.attention64(q, x, kvhat, g0, b0, Sq, Bq, Nk, Bk, None, softmax64=soft64, key_ptr=kp)
            dkv = torch.full((Bk * Nk, H), NAN, dtype=torch.float64, device=DEV)
            dq, part, ds = ops.attention_bwd64(dout, q, kvhat, g0, b0, probs, Sq, Bq, Nk, Bk, dkv, None, softmax64=soft64,
                                               key_ptr=kp)
            res.append((out, probs, dq, part, ds, dkv))
        for a, b in zip(*res):
            assert torch.equal(a, b) and not bool(torch.isnan(a).any())
        out, probs, dq, part, ds, dkv = res[0]
        for bq in (0, 2):                                              # the query crystals of the empty key crystal
            rows = slice(bq * Sq, (bq + 1) * Sq)
            assert torch.equal(out[rows], x[rows]) and _all_zero(probs[bq]) and _all_zero(dq[rows]) and _all_zero(ds[bq])
        assert _all_zero(part[:Nk]) and _all_zero(dkv[:Nk])
        assert float((probs[1].sum(-1) - 1.0).abs().max()) < 1e-6
    for bad in (torch.zeros(Bk + 1, dtype=torch.int64, device=DEV), torch.zeros(Bk, dtype=torch.int32, device=DEV),
                torch.zeros(Bk + 1, dtype=torch.int32), [0, 2, 5]):
        with pytest.raises(ValueError, match="key_ptr"):
            ops.attention64(q, x, kvhat, g0, b0, Sq, Bq, Nk, Bk, None, key_ptr=bad)


# ---- the model --------------------------------------------------------------------------------------------------------------
BATCHES = {"h16": dict(n_atoms=[1, 2, 17, 33], L=2, T=1, H=16, seed=31),
           "h64": dict(n_atoms=[2, 5, 16, 70], L=2, T=2, H=64, seed=32)}
S = 51


def _soft64_mha(q, k, v, drop_mask=None):
    dim = q.shape[2]
    w = torch.bmm(q.transpose(0, 1), k.transpose(0, 1).transpose(1, 2)) * (dim ** -0.5)
    w = F.softmax(w, dim=-1)
    if drop_mask is not None:
        w = w * drop_mask.to(w.dtype)
    return torch.bmm(w, v.transpose(0, 1)).transpose(0, 1)


def _crystals(name):
    from dostransformer_amd import synth
    gen = torch.Generator().manual_seed(BATCHES[name]["seed"])
    return [synth.phonon_crystal(gen, n) for n in BATCHES[name]["n_atoms"]]


def _collate(cs):
    from dostransformer_amd.batch import collate
    return collate(cs)


def _model(name, attn_drop=0.0, flag=True):
    from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
    c = BATCHES[name]
    torch.manual_seed(c["seed"])
    model = DOSTransformer_phonon(c["L"], c["T"], 118, 4, c["H"], DEV, attn_drop).double()
    p = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.set_program_dtype(torch.float64).set_per_crystal_keys(flag).to(DEV)
    assert model.per_crystal_keys is flag
    return model, p


def _weights(name):
    c = BATCHES[name]
    B, N = len(c["n_atoms"]), sum(c["n_atoms"])
    gw = torch.Generator().manual_seed(3)
    return [torch.randn(B, S, generator=gw, dtype=torch.float64), torch.randn(B, S, generator=gw, dtype=torch.float64),
            torch.randn(N, c["H"], generator=gw, dtype=torch.float64)]


def _oracle(p, g, L, T, w, drop_masks=None):
    """(dos_global, x, dos_system) and the gradients of sum(dg w0) + sum(ds w1) + sum(x w2)"""
    from oracle import dos_oracle as O
    pr = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in p.items()}
    dg, x, ds = O.dostransformer_phonon_forward(pr, g, L, T, drop_masks)
    ((dg * w[0]).sum() + (ds * w[1]).sum() + (x * w[2]).sum()).backward()
    return (dg.detach(), x.detach(), ds.detach()), {k: v.grad for k, v in pr.items()}


def _ptr(name):
    ptr = [0]
    for n in BATCHES[name]["n_atoms"]:
        ptr.append(ptr[-1] + n)
    return ptr


def _oracle_batch1(name, p, masks=None):
    """The oracle on every crystal alone (collate([c])): -> per-crystal outputs, per-crystal gradients.  masks: the
    logged [Bq, S, Nk] masks of the batched run; crystal b alone gets rows [b, B + b] (transformer: [b]) and columns [:n_b]."""
    c = BATCHES[name]
    cs, w, ptr = _crystals(name), _weights(name), _ptr(name)
    B = len(cs)
    outs, grads = [], []
    for b, cr in enumerate(cs):
        n = c["n_atoms"][b]
        wb = [w[0][b:b + 1], w[1][b:b + 1], w[2][ptr[b]:ptr[b + 1]]]
        mb = None
        if masks is not None:
            mb = {"transformer": [m[b:b + 1, :, :n] for m in masks["transformer"]],
                  "transformer_self": [m[[b, B + b]] for m in masks["transformer_self"]],
                  "transformer_source": [m[[b, B + b]][:, :, :n] for m in masks["transformer_source"]]}
        o, g = _oracle(p, _collate([cr]), c["L"], c["T"], wb, mb)
        outs.append(o)
        grads.append(g)
    return outs, grads


def _sum_grads(grads):
    return {k: (None if grads[0][k] is None else sum(g[k] for g in grads)) for k in grads[0]}


def _dead_params(p):
    from dostransformer_amd._fused import is_dead_param
    return {k for k in p if is_dead_param(k)}


def _loss(out, w):
    wd = [t.to(DEV) for t in w]
    return (out[0] * wd[0]).sum() + (out[2] * wd[1]).sum() + (out[1] * wd[2]).sum()


def _check_outputs(name, out, refs, tol=1e-12):
    ptr = _ptr(name)
    for b, (dg, x, ds) in enumerate(refs):
        e = (rmse(out[0][b].cpu(), dg[0]), rmse(out[2][b].cpu(), ds[0]), rmse(out[1][ptr[b]:ptr[b + 1]].cpu(), x))
        assert max(e) <= tol, (name, b, e)


def _check_grads(model, ref_grads, dead, tol=1e-10):
    worst = 0.0
    for k, prm in model.named_parameters():
        if k in dead:
            assert prm.grad is None, k
            continue
        assert prm.grad is not None and prm.grad.dtype == torch.float64, k
        r = ref_grads[k]
        e = float((prm.grad.cpu() - r).abs().max() / (r.abs().max() + 1e-300))
        worst = max(worst, e)
        assert e <= tol, (k, e)
    return worst


@pytest.mark.parametrize("name", list(BATCHES))
def test_per_crystal_keys_model_equals_the_batch_1_oracle(name, monkeypatch):
    """fp64 softmax on both sides.  One flagged forward + backward on the batch: every crystal's global and system DOS and its
    rows of x within 1e-12 RMSE of the oracle run on that crystal alone, every live gradient within 1e-10 relative of the sum
    over crystals of the oracle's batch-1 gradients.  Input condition (CPU): for every crystal smaller than the largest the
    oracle's batched DOS differs from its batch-1 DOS by RMSE >= 1e-3, and the unflagged model still is the batched oracle -
    so the flag cannot be ignored.  Two flagged runs are bitwise equal."""
    from oracle import dos_oracle as O
    from dostransformer_amd import functional64 as F64
    monkeypatch.setattr(O, "multihead_attention", _soft64_mha)
    monkeypatch.setattr(F64, "SOFTMAX64", True)
    c = BATCHES[name]
    cs, w = _crystals(name), _weights(name)
    model, p = _model(name)
    refs, grads1 = _oracle_batch1(name, p)
    out = model(_collate(cs).to(DEV))
    assert all(t.dtype == torch.float64 for t in out)
    _check_outputs(name, out, refs)
    _loss(out, w).backward()
    worst = _check_grads(model, _sum_grads(grads1), _dead_params(p))
    print(f"{name}: worst per-tensor gradient error {worst:.2e}")
    # the input condition, and the unflagged program against the batched oracle
    (bg, bx, bs), _ = _oracle(p, _collate(cs), c["L"], c["T"], w)
    nmax = max(c["n_atoms"])
    diffs = [min(rmse(bg[b], refs[b][0][0]), rmse(bs[b], refs[b][2][0])) for b, n in enumerate(c["n_atoms"]) if n < nmax]
    print(f"{name}: batched against batch-1 oracle, smallest RMSE of a padded crystal {min(diffs):.2e}")
    assert len(diffs) == len(cs) - 1 and min(diffs) >= 1e-3, diffs
    plain, _ = _model(name, flag=False)
    with torch.no_grad():
        po = plain(_collate(cs).to(DEV))
    for a, b in zip(po, (bg, bx, bs)):
        assert rmse(a.cpu(), b) <= 1e-12
    # reproducibility: forward and backward
    g1 = {k: v.grad.clone() for k, v in model.named_parameters() if v.grad is not None}
    model.zero_grad(set_to_none=True)
    out2 = model(_collate(cs).to(DEV))
    assert all(torch.equal(a, b) for a, b in zip(out, out2))
    _loss(out2, w).backward()
    for k, v in model.named_parameters():
        if v.grad is not None:
            assert torch.equal(v.grad, g1[k]), k


def test_per_crystal_keys_model_with_attention_dropout(monkeypatch):
    """attn_drop 0.25 in train mode: the masks are drawn on [Bq, S, nmax] as without the flag; the oracle alone on crystal b
    gets rows [b, B + b] and columns [:n_b] of each logged mask.  Same bounds."""
    from oracle import dos_oracle as O
    from dostransformer_amd import functional as Fn
    from dostransformer_amd import functional64 as F64
    monkeypatch.setattr(O, "multihead_attention", _soft64_mha)
    monkeypatch.setattr(F64, "SOFTMAX64", True)
    monkeypatch.setattr(Fn, "DROP_MASK_LOG", [])
    name = "h16"
    c = BATCHES[name]
    cs, w = _crystals(name), _weights(name)
    B, T, nmax = len(cs), c["T"], max(c["n_atoms"])
    model, p = _model(name, attn_drop=0.25)
    model.train()
    out = model(_collate(cs).to(DEV))
    log = Fn.DROP_MASK_LOG
    assert len(log) == 3 * T
    masks = {pre: [m.detach().cpu().double() for (pr, t, m) in log if pr == pre] for pre in
             ("transformer", "transformer_self", "transformer_source")}
    assert tuple(masks["transformer"][0].shape) == (B, S, nmax)
    assert tuple(masks["transformer_source"][0].shape) == (2 * B, S, nmax)
    assert tuple(masks["transformer_self"][0].shape) == (2 * B, S, S)
    assert float(masks["transformer_source"][0].min()) == 0.0            # something was dropped
    refs, grads1 = _oracle_batch1(name, p, masks)
    _check_outputs(name, out, refs)
    _loss(out, w).backward()
    worst = _check_grads(model, _sum_grads(grads1), _dead_params(p))
    print(f"dropout: worst per-tensor gradient error {worst:.2e}")


def test_per_crystal_keys_model_reference_softmax(monkeypatch):
    """The reference's fp32 softmax (no hook on either side): each crystal's DOS vectors and every gradient within
    4 D_ref + 1e-12 of the batch-1 oracle, D_ref what the oracle's fp32 softmax moves the number by against its fp64 softmax
    (per crystal and DOS vector max abs; for a gradient the sum over crystals of the per-crystal max abs) - the rule of
    _check_ref_mode with each tensor's own D_ref.  x does not pass through a softmax: 1e-12 RMSE."""
    from oracle import dos_oracle as O
    name = "h64"
    cs, w, ptr = _crystals(name), _weights(name), _ptr(name)
    model, p = _model(name)
    refs_a, grads_a = _oracle_batch1(name, p)                              # the reference: fp32 softmax
    with monkeypatch.context() as mp:
        mp.setattr(O, "multihead_attention", _soft64_mha)
        refs_b, grads_b = _oracle_batch1(name, p)
    out = model(_collate(cs).to(DEV))
    worst = 0.0
    for b in range(len(cs)):
        for tag, got, i in (("dos_global", out[0][b], 0), ("dos_system", out[2][b], 2)):
            d = float((got.detach().cpu() - refs_a[b][i][0]).abs().max())
            dref = float((refs_a[b][i][0] - refs_b[b][i][0]).abs().max())
            worst = max(worst, d / (dref + 1e-12 / 4))
            print(f"crystal {b} {tag}: d {d:.3e} D_ref {dref:.3e}")
            assert d <= 4 * dref + 1e-12, (b, tag, d, dref)
        assert rmse(out[1][ptr[b]:ptr[b + 1]].detach().cpu(), refs_a[b][1]) <= 1e-12
    _loss(out, w).backward()
    dead = _dead_params(p)
    ga = _sum_grads(grads_a)
    worst_g = 0.0
    for k, prm in model.named_parameters():
        if k in dead:
            assert prm.grad is None, k
            continue
        d = float((prm.grad.cpu() - ga[k]).abs().max())
        dref = sum(float((a[k] - b_[k]).abs().max()) for a, b_ in zip(grads_a, grads_b))
        worst_g = max(worst_g, d / (dref + 1e-12 / 4))
        print(f"{k}: d {d:.3e} D_ref {dref:.3e}")
        assert d <= 4 * dref + 1e-12, (k, d, dref)
    print(f"worst d / (D_ref + 2.5e-13): outputs {worst:.2f}, gradients {worst_g:.2f} (bound 4)")


@pytest.mark.parametrize("name", list(BATCHES))
def test_per_crystal_keys_outputs_do_not_depend_on_the_batch(name, monkeypatch):
    """Both runs on the GPU with the flag set: a crystal in the batch of four against the same crystal alone, within 1e-12 of
    the output's scale."""
    from dostransformer_amd import functional64 as F64
    monkeypatch.setattr(F64, "SOFTMAX64", True)
    cs, ptr = _crystals(name), _ptr(name)
    model, _ = _model(name)
    with torch.no_grad():
        out = [t.clone() for t in model(_collate(cs).to(DEV))]
        for b, cr in enumerate(cs):
            dg, x, ds = model(_collate([cr]).to(DEV))
            for got, ref in ((out[0][b], dg[0]), (out[2][b], ds[0]), (out[1][ptr[b]:ptr[b + 1]], x)):
                assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), (name, b)
