"""float64 DOSTransformer_phonon on a real MI355X (csrc/f64_attention.hip, functional64.dostransformer_phonon_fwd/bwd): the
attention, dense-row and index-sum kernels against float64 torch, and the model against the float64 oracle - sharply with the
softmax in fp64 on both sides, and in the reference's mode (fp32 softmax) against its G5 fixture and training loop within a
few times D_ref, what the reference's own fp32 softmax moves the numbers by."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.util import batch_from, load, rmse, sub

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24


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


def _ref_attention(q, x, kvhat, g0, b0, Sq, Bq, Nk, Bk, mask, soft64):
    """float64 torch with the reference's numerics (multihead_attention.py:68-72); autograd gives the backward"""
    H = q.shape[1]
    k = (kvhat * g0 + b0).view(Bk, Nk, H)[torch.arange(Bq, device=q.device) % Bk]
    sc = q.view(Bq, Sq, H) @ k.transpose(1, 2) * (H ** -0.5)
    p = F.softmax(sc, -1) if soft64 else F.softmax(sc.float(), -1).type_as(sc)
    pd = p if mask is None else p * mask.to(p.dtype)
    return x + (pd @ k).reshape(Bq * Sq, H), p, sc


def _bound(got, ref, scale, k=1e-13):
    err = (got - ref).abs()
    ok = bool((err <= k * scale + 1e-300).all())
    return ok, float((err / (scale + 1e-300)).max())


CASES = [(51, 3, 5, 3, 16), (51, 8, 17, 4, 64), (1, 2, 1, 2, 8), (51, 4, 51, 4, 128), (33, 2, 300, 2, 36), (51, 2, 65, 1, 512)]


@pytest.mark.parametrize("Sq,Bq,Nk,Bk,H", CASES)
def test_attention_f64_exact_mode(Sq, Bq, Nk, Bk, H):
    """fp64 softmax (DOSX_ATTN64_SOFTMAX_F64): every output within 1e-13 of its operand scale, the error bound of an fp64 sum
    propagated through abs-valued operands.  Zero (padding) key rows, mask on / off, accumulate on / off; bitwise repeatable."""
    ops = _ops()
    q, x = _r(Bq * Sq, H, seed=1), _r(Bq * Sq, H, seed=2)
    kvhat = _r(Bk * Nk, H, seed=3)
    if Nk > 1:
        kvhat.view(Bk, Nk, H)[0, Nk // 2:] = 0.0          # ghost keys of crystal 0: k = v = beta0
    g0, b0 = _r(H, seed=4, scale=0.5) + 1.0, _r(H, seed=5, scale=0.3)
    dout = _r(Bq * Sq, H, seed=6)
    c = H ** -0.5
    for use_mask in (False, True):
        mask = _mask(Bq, Sq, Nk, 7) if use_mask else None
        out, probs = ops.attention64(q, x, kvhat, g0, b0, Sq, Bq, Nk, Bk, mask, softmax64=True)
        out2, probs2 = ops.attention64(q, x, kvhat, g0, b0, Sq, Bq, Nk, Bk, mask, softmax64=True)
        assert torch.equal(out, out2) and torch.equal(probs, probs2)
        qq, kk, gg, bb = (t.clone().requires_grad_(True) for t in (q, kvhat, g0, b0))
        ref, p, _ = _ref_attention(qq, x, kk, gg, bb, Sq, Bq, Nk, Bk, mask, True)
        ref.backward(dout)
        # abs-valued operand scales
        kab = (kvhat.abs() * g0.abs() + b0.abs()).view(Bk, Nk, H)[torch.arange(Bq, device=DEV) % Bk]
        m_ab = torch.ones_like(probs) if mask is None else mask.double()
        s_ab = q.abs().view(Bq, Sq, H) @ kab.transpose(1, 2) * c
        p_sc = p.detach() * (1.0 + s_ab)
        out_sc = x.abs() + ((p_sc * m_ab) @ kab).reshape(Bq * Sq, H)
        ok, worst = _bound(out, ref.detach(), out_sc)
        assert ok, ("out", worst)
        ok, worst = _bound(probs, p.detach(), p_sc)
        assert ok, ("probs", worst)
        dP_ab = dout.abs().view(Bq, Sq, H) @ kab.transpose(1, 2)
        g_ab = dP_ab * m_ab
        ds_sc = p_sc * (g_ab + (p.detach() * g_ab).sum(-1, keepdim=True)) * c
        dq_sc = (ds_sc @ kab).reshape(Bq * Sq, H)
        sel = lambda t: t.view(Bq // Bk, Bk, Sq, -1).transpose(0, 1).reshape(Bk, (Bq // Bk) * Sq, -1)
        dkv_sc = (sel(ds_sc).transpose(1, 2) @ sel(q.abs().view(Bq, Sq, H)) +
                  sel(p_sc * m_ab).transpose(1, 2) @ sel(dout.abs().view(Bq, Sq, H))).reshape(Bk * Nk, H)
        for acc in (False, True):
            base = _r(Bk * Nk, H, seed=8)
            dkv = base.clone()
            dq, part, ds = ops.attention_bwd64(dout, q, kvhat, g0, b0, probs, Sq, Bq, Nk, Bk, dkv, mask, softmax64=True,
                                               accumulate=acc)
            dkv2 = base.clone()
            r2 = ops.attention_bwd64(dout, q, kvhat, g0, b0, probs, Sq, Bq, Nk, Bk, dkv2, mask, softmax64=True, accumulate=acc)
            assert torch.equal(dq, r2[0]) and torch.equal(part, r2[1]) and torch.equal(dkv, dkv2)
            ok, worst = _bound(dq, qq.grad, dq_sc)
            assert ok, ("dq", worst)
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


@pytest.mark.parametrize("Sq,Bq,Nk,Bk,H", [(51, 4, 17, 2, 16), (51, 6, 51, 6, 64), (33, 2, 300, 2, 64), (51, 2, 65, 1, 16)])
def test_attention_f64_reference_softmax(Sq, Bq, Nk, Bk, H):
    """Reference mode.  Dyadic operands and H in {16, 64} (H^-1/2 = 1/4, 1/8) make the fp64 scores and dP exact, so both
    sides round the same fp32 values.  Rounding count for p = e_j / sum e (each side): expf <= 1 ulp (2 units of 2^-24
    relative), the sum of the e_j <= 2 + d units (d: additions on the longest path - GPU ceil(Nk/64) - 1 per lane plus a
    6-level butterfly, torch at most Nk - 1), the division 1 (torch: a reciprocal and a multiply, 2): c = 11 + d_gpu + Nk.
    dS = p (g - sum p g) with the same p and g on both sides: products and the dot sum d + 1 units of sum |p g| each side,
    the subtraction and the product 1 each: c = 4 + d_gpu + Nk + 1 on p (|g| + sum p |g|)."""
    ops = _ops()
    q, x = _dy(Bq * Sq, H, seed=1), _r(Bq * Sq, H, seed=2)
    kvhat = _dy(Bk * Nk, H, seed=3)
    kvhat.view(Bk, Nk, H)[0, Nk // 2:] = 0.0
    g0, b0 = _dy(H, seed=4, lo=2, hi=5, den=2.0), _dy(H, seed=5, lo=-2, hi=3)
    dout = _dy(Bq * Sq, H, seed=6)
    d_gpu = math.ceil(Nk / 64) - 1 + 6
    for use_mask in (False, True):
        mask = _mask(Bq, Sq, Nk, 7) if use_mask else None
        out, probs = ops.attention64(q, x, kvhat, g0, b0, Sq, Bq, Nk, Bk, mask)
        _, p_ref, sc = _ref_attention(q, x, kvhat, g0, b0, Sq, Bq, Nk, Bk, mask, False)
        c = 11 + d_gpu + Nk
        ok, worst = _bound(probs, p_ref, p_ref, k=c * U)
        print(f"probs: worst {worst / U:.2f} units of 2^-24 p (c = {c})")
        assert ok, ("probs", worst / U)
        assert torch.equal(probs, probs.float().double())                  # promoted fp32 values
        dkv = torch.zeros(Bk * Nk, H, dtype=torch.float64, device=DEV)
        dq, part, ds = ops.attention_bwd64(dout, q, kvhat, g0, b0, probs, Sq, Bq, Nk, Bk, dkv, mask)
        k = (kvhat * g0 + b0).view(Bk, Nk, H)[torch.arange(Bq, device=DEV) % Bk]
        g = dout.view(Bq, Sq, H) @ k.transpose(1, 2)
        if mask is not None:
            g = g * mask.double()
        g32, p32 = g.float(), probs.float()
        ds_ref = torch._softmax_backward_data(g32, p32, -1, torch.float32).double() * (H ** -0.5)
        scale = probs * (g.abs() + (probs * g.abs()).sum(-1, keepdim=True)) * (H ** -0.5)
        c = 4 + d_gpu + Nk + 1
        ok, worst = _bound(ds, ds_ref, scale, k=c * U)
        print(f"ds: worst {worst / U:.2f} units (c = {c})")
        assert ok, ("ds", worst / U)


def test_dense_rows_and_index_sum_f64():
    from oracle.dos_oracle import to_dense_batch
    ops = _ops()
    counts = [3, 1, 7, 5]
    B, nmax, H = len(counts), 9, 48
    N = sum(counts)
    batch = torch.repeat_interleave(torch.arange(B), torch.tensor(counts))
    ptr = torch.zeros(B + 1, dtype=torch.int32)
    ptr[1:] = torch.cumsum(torch.tensor(counts), 0)
    x = _r(N, H, seed=1, scale=3.0) + 0.5
    xx = x.detach().cpu().clone().requires_grad_(True)
    ref = F.layer_norm(to_dense_batch(xx, batch, B, nmax), (H,), None, None, 1e-5).reshape(B * nmax, H)
    rows, rstd = ops.dense_rows64(x, ptr.to(DEV), B, nmax)
    assert float((rows.cpu() - ref.detach()).abs().max()) <= 1e-13
    assert torch.equal(rows.view(B, nmax, H)[1, 1:], torch.zeros(nmax - 1, H, dtype=torch.float64, device=DEV))
    dout = _r(B * nmax, H, seed=2)
    ref.backward(dout.cpu())
    base = _r(N, H, seed=3)
    for acc in (False, True):
        dx = base.clone()
        ops.dense_rows_bwd64(dout, rows, rstd, ptr.to(DEV), dx, B, nmax, accumulate=acc)
        want = xx.grad + (base.cpu() if acc else 0.0)
        assert float((dx.cpu() - want).abs().max()) <= 1e-12 * float(want.abs().max())
    src = _r(10, 24, seed=4)
    idx = torch.tensor([3, 0, 3, 6, 3, 1, 0, 5, 3, 2], dtype=torch.int32)
    out = torch.full((7, 24), 7.0, dtype=torch.float64, device=DEV)
    ops.index_sum64(src, idx.to(DEV), out)
    want = torch.zeros(7, 24, dtype=torch.float64).index_add(0, idx.long(), src.cpu())
    assert float((out.cpu() - want).abs().max()) <= 1e-14
    assert torch.equal(out[4], torch.zeros(24, dtype=torch.float64, device=DEV))   # no crystal of system 4


# ---- the model --------------------------------------------------------------------------------------------------------------
def _soft64_mha(q, k, v, drop_mask=None):
    dim = q.shape[2]
    w = torch.bmm(q.transpose(0, 1), k.transpose(0, 1).transpose(1, 2)) * (dim ** -0.5)
    w = F.softmax(w, dim=-1)
    if drop_mask is not None:
        w = w * drop_mask.to(w.dtype)
    return torch.bmm(w, v.transpose(0, 1)).transpose(0, 1)


def _model(L, T, H, attn_drop=0.0, seed=0, state=None):
    from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
    torch.manual_seed(seed)
    model = DOSTransformer_phonon(L, T, 118, 4, H, DEV, attn_drop).double()
    if state is not None:
        model.load_state_dict(state)
    p = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return model.set_program_dtype(torch.float64).to(DEV), p


def _oracle(p, g, L, T, w, drop_masks=None):
    from oracle import dos_oracle as O
    pr = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in p.items()}
    dg, x, ds = O.dostransformer_phonon_forward(pr, g, L, T, drop_masks)
    ((dg * w[0]).sum() + (ds * w[1]).sum() + (x * w[2]).sum()).backward()
    return (dg.detach(), x.detach(), ds.detach()), {k: v.grad for k, v in pr.items()}


def _dead(p):
    from dostransformer_amd._fused import is_dead_param
    return {k for k in p if is_dead_param(k)}


def _worst_grad(model, ref_grads, dead, tol):
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


def _big_batch():
    """crystals of 2, 5, 70 and 120 atoms: Nk = 120 > 64 keys, most of them padding for three of the crystals"""
    from dostransformer_amd import synth
    return synth.phonon_batch(4, seed=11, n_atoms=[2, 5, 70, 120])


@pytest.mark.parametrize("case", ["g5", "h64", "h128", "big", "dropout"])
def test_dostransformer_phonon_f64_exact_softmax(case, monkeypatch):
    """SOFTMAX64 on the GPU and an fp64 softmax in the oracle: everything else is float64 on both sides, so outputs agree to
    1e-12 RMSE and every live gradient to 1e-10 relative.  The loss has a term on x."""
    from oracle import dos_oracle as O
    from dostransformer_amd import functional as Fn
    from dostransformer_amd import functional64 as F64
    from dostransformer_amd import synth
    monkeypatch.setattr(O, "multihead_attention", _soft64_mha)
    monkeypatch.setattr(F64, "SOFTMAX64", True)
    drop = 0.0
    if case == "g5":
        z = load("g5_phonon.npz")
        L, T, H = 3, 1, 16
        model, p = _model(L, T, H, state=sub(z, "p0/"))
        g = batch_from(z)
    elif case == "big":
        L, T, H = 2, 2, 64
        model, p = _model(L, T, H, seed=3)
        g = _big_batch()
    else:
        L, T, H = 3, 2, (128 if case == "h128" else 64)
        drop = 0.25 if case == "dropout" else 0.0
        model, p = _model(L, T, H, attn_drop=drop, seed=1)
        g = synth.phonon_batch(8, seed=17, dtype=torch.float64)
    B = int(g.system.shape[0])
    gw = torch.Generator().manual_seed(3)
    w = [torch.randn(B, 51, generator=gw, dtype=torch.float64), None, None]
    w[1] = torch.randn(B, 51, generator=gw, dtype=torch.float64)
    w[2] = torch.randn(g.x.shape[0], H, generator=gw, dtype=torch.float64)
    masks = None
    if drop > 0.0:
        model.train()
        monkeypatch.setattr(Fn, "DROP_MASK_LOG", [])
    out = model(g.clone().to(DEV))
    if drop > 0.0:
        log = Fn.DROP_MASK_LOG
        assert len(log) == 3 * T
        masks = {pre: [m.detach().cpu().double() for (pr, t, m) in log if pr == pre] for pre in
                 ("transformer", "transformer_self", "transformer_source")}
        assert tuple(masks["transformer_source"][0].shape) == (2 * B, 51, int(torch.bincount(g.batch).max()))
        assert tuple(masks["transformer_self"][0].shape) == (2 * B, 51, 51)
    ref, rg = _oracle(p, g, L, T, w, masks)
    assert all(t.dtype == torch.float64 for t in out)
    for a, b in zip(out, ref):
        assert rmse(a.detach().cpu(), b) <= 1e-12, (case, rmse(a.detach().cpu(), b))
    wd = [t.to(DEV) for t in w]
    ((out[0] * wd[0]).sum() + (out[2] * wd[1]).sum() + (out[1] * wd[2]).sum()).backward()
    worst = _worst_grad(model, rg, _dead(p), 1e-10)
    print(f"{case}: worst per-tensor gradient error {worst:.2e}")
    assert all(v.dtype == torch.float64 for v in model.state_dict().values() if v.is_floating_point())
    if drop > 0.0:
        return
    # two runs bitwise equal; an fp32 batch is promoted once and gives what the float64 batch of the same values gives
    with torch.no_grad():
        again = model(g.clone().to(DEV))
        assert all(torch.equal(a, b) for a, b in zip(again, out))
        g32 = g.clone().to(DEV, dtype=torch.float32)
        o32 = model(g32)
        g64 = g.clone()
        g64.x, g64.edge_vec = g32.x.cpu().double(), g32.edge_vec.cpu().double()
        o64 = model(g64.to(DEV))
        assert all(a.dtype == torch.float64 and torch.equal(a, b) for a, b in zip(o32, o64))


def _d_ref(p, g, L, T, monkeypatch):
    """Oracle (fp32 softmax, the reference) and the same with an fp64 softmax: outputs, loss and gradients of each"""
    from oracle import dos_oracle as O

    def run():
        pr = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in p.items()}
        dg, x, ds = O.dostransformer_phonon_forward(pr, g, L, T)
        loss = O.loss_phonon(dg, ds, g.phdos)
        loss.backward()
        return (dg.detach(), x.detach(), ds.detach()), loss.detach(), {k: v.grad for k, v in pr.items()}

    a = run()
    with monkeypatch.context() as mp:
        mp.setattr(O, "multihead_attention", _soft64_mha)
        b = run()
    return a, b


def _check_ref_mode(out, loss, model, a, b, dead, tag):
    """Each DOS vector and gradient within 4 D_ref + 1e-12 of the reference (D_ref: the reference against its fp64-softmax
    variant, per tensor max abs); returns the noise floor of every gradient tensor.

    For a gradient tensor D_ref can be a single draw of zero-mean noise: a PReLU weight or out_layer.bias is one sum over every
    node / edge / energy row of terms that each carry an independent fp32-softmax rounding (~2^-24 relative, either sign), and
    a final LayerNorm bias is the out_layer weight times one such sum.  The GPU's deviation (its expf and summation order
    round differently from torch-CPU's) is another draw of the same noise, and the ratio of two draws is Cauchy-like: above 4
    in about one case in six.  The floor of a tensor is therefore 4 max(D_ref, rel |g|max), rel the largest relative D_ref of
    the model (the measure of the issue's table: 5.4e-8 for G5)."""
    (ra, la, ga), (rb, lb, gb) = a, b
    worst = 0.0
    for name, got, r, r2 in (("dos_global", out[0], ra[0], rb[0]), ("dos_system", out[2], ra[2], rb[2])):
        d = float((got.detach().cpu() - r).abs().max())
        dref = float((r - r2).abs().max())
        worst = max(worst, d / (dref + 1e-300))
        assert d <= 4 * dref + 1e-12, (tag, name, d, dref)
    assert rmse(out[1].detach().cpu(), ra[1]) <= 1e-12, (tag, "x")
    assert abs(float(loss.detach()) - float(la)) <= 1e-8, (tag, float(loss.detach()), float(la))
    live = [k for k, _ in model.named_parameters() if k not in dead]
    dref = {k: float((ga[k] - gb[k]).abs().max()) for k in live}
    rel = max(dref[k] / (float(ga[k].abs().max()) + 1e-300) for k in live)
    floors = {}
    worst_t = 0.0
    for k, prm in model.named_parameters():
        if k in dead:
            assert prm.grad is None, k
            continue
        d = float((prm.grad.cpu() - ga[k]).abs().max())
        worst_t = max(worst_t, d / (dref[k] + 1e-300))
        dr = max(dref[k], rel * float(ga[k].abs().max()))
        floors[k] = 4 * dr + 1e-12
        worst = max(worst, d / (dr + 1e-300))
        assert d <= floors[k], (tag, k, d, dref[k], dr)
    print(f"{tag}: worst ratio to the floor / 4: {worst:.2f}; worst ratio to the tensor's own D_ref {worst_t:.2f}; "
          f"largest relative D_ref {rel:.2e}")
    return floors


def _check_params(model, ref, grads, floors, tol, tag, lr=1e-4, eps=1e-8, sticky=None, state=None):
    """Parameters after AdamW steps within tol.  Exempt (and print) the entries whose gradient sits so close to the noise
    floor that AdamW's step moves by more than tol / 4 when the gradient moves by the floor.  The step is
    lr m^ / (sqrt(v^) + eps); its derivative with respect to the step's gradient is at most
    lr (1 - b1) / (1 - b1^t) / (sqrt(v^) + eps) (v^ from the oracle's AdamW state; after one step sqrt(v^) = |g|).
    sticky (a loop): an entry exempted once stays exempted, its parameter keeps the difference of that step."""
    sd = model.state_dict()
    for k, v in ref.items():
        if not v.is_floating_point():
            continue
        d = (sd[k].cpu() - v).abs()
        gk = grads.get(k)
        if gk is not None:
            if state is not None:
                t = state[k]["step"]
                vh = (state[k]["v"] / (1 - 0.999 ** t)).sqrt()
                gain = (1 - 0.9) / (1 - 0.9 ** t)
            else:
                vh, gain = gk.abs(), 1.0
            exempt = (gk.abs() < floors[k]) | (lr * gain * floors[k] / (vh + eps) > tol / 4)
            if sticky is not None:
                exempt = exempt | sticky.get(k, torch.zeros_like(exempt))
                sticky[k] = exempt
            for i in (exempt & (d > tol)).nonzero().tolist():
                print("exempt", tag, k, i, float(d[tuple(i)]), float(gk[tuple(i)]))
            d = torch.where(exempt, torch.zeros_like(d), d)
        assert float(d.max()) <= tol, (tag, k, float(d.max()))


def test_dostransformer_phonon_f64_g5_reference_mode(monkeypatch):
    """The reference's own float64 numbers (G5, fp32 softmax) and its AdamW trajectory (lr 1e-4, wd 1e-2)."""
    from oracle import dos_oracle as O
    z = load("g5_phonon.npz")
    L, T, H = 3, 1, 16
    model, p = _model(L, T, H, state=sub(z, "p0/"))
    g = batch_from(z)
    a, b = _d_ref(p, g, L, T, monkeypatch)
    assert float((a[0][0] - torch.from_numpy(z["dos_global"])).abs().max()) <= 1e-12      # the oracle is the fixture
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=1e-2)
    gd = g.clone().to(DEV)
    out = model(gd)
    assert rmse(out[1].detach().cpu(), z["x_nodes"]) <= 1e-12
    loss = O.loss_phonon(out[0], out[2], gd.phdos)
    assert abs(float(loss.detach()) - float(z["loss"])) <= 1e-8
    loss.backward()
    dead = set(str(s) for s in z["dead_params"])
    floors = _check_ref_mode(out, loss, model, a, b, dead, "g5")
    fixture = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("g/")}
    for k, prm in model.named_parameters():
        if k not in dead:
            assert float((prm.grad.cpu() - fixture[k]).abs().max()) <= floors[k], k
    grads = {k: prm.grad.detach().cpu().clone() for k, prm in model.named_parameters() if k not in dead}
    opt.step()
    _check_params(model, sub(z, "p1/"), grads, floors, 1e-9, "p1")
    for _ in range(2):
        opt.zero_grad()
        out = model(gd)
        O.loss_phonon(out[0], out[2], gd.phdos).backward()
        opt.step()
    _check_params(model, sub(z, "p3/"), grads, floors, 1e-9, "p3")


def test_dostransformer_phonon_f64_reference_loop(monkeypatch):
    """The reference's loop in float64 (default dtype float64, L3 T2 H64 B8, 3 steps of torch.optim.AdamW) against the oracle's
    autograd + adamw_step, with the bounds of the G5 test."""
    from oracle import dos_oracle as O
    from dostransformer_amd import synth
    from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
    L, T, H, B = 3, 2, 64, 8
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        torch.manual_seed(0)
        model = DOSTransformer_phonon(L, T, 118, 4, H, DEV, 0.0).set_program_dtype(torch.float64)
        params = {k: v.detach().clone() for k, v in model.state_dict().items()}
        model = model.to(DEV)
        opt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=1e-2)
        g = synth.phonon_batch(B, seed=5)
        gd = g.clone().to(DEV)
        dead = _dead(params)
        state, sticky = {}, {}
        for step in range(3):
            # this step's numbers against the oracle at the module's own current parameters (x then runs on equal inputs) ...
            here = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
            opt.zero_grad()
            out = model(gd)
            loss = O.loss_phonon(out[0], out[2], gd.phdos)
            loss.backward()
            a, b = _d_ref(here, g, L, T, monkeypatch)
            floors = _check_ref_mode(out, loss, model, a, b, dead, f"step {step}")
            opt.step()
            # ... and the trajectory against the oracle's own autograd + adamw_step from the same start
            ao, _ = _d_ref(params, g, L, T, monkeypatch) if step else (a, None)
            O.adamw_step(params, ao[2], state, 1e-4)
            _check_params(model, params, ao[2], floors, 1e-9, f"step {step}", sticky=sticky, state=state)
    finally:
        torch.set_default_dtype(old)
