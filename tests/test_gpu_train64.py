"""The fused float64 training step on a real MI355X: dosx_loss_phonon_f64 (csrc/f64_train.hip) and dosx_adamw_f64 (csrc/adamw.hip) against
float64 torch / a long-double host reference, and train64.Trainer64 - eager against the hand-written loop (model(batch), torch
loss, loss.backward(), torch.optim.AdamW) and against the float64 oracle run crystal by crystal, replay against eager (bitwise),
checkpoint and resume (bitwise).  Bounds: the project's float64 bars (tests/test_gpu_f64.py): losses 1e-12 relative, gradients
1e-10 relative per tensor, parameters after AdamW steps 1e-9."""
import copy
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 12345.0
U64 = 2.0 ** -53


def _ops():
    from dostransformer_amd import ops
    return ops


def _relmax(got, ref):
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-300))


# =====================================================================================================================
# 1. the loss kernel
# =====================================================================================================================
def _loss_inputs(count, seed):
    """targets whose magnitudes span 1e-3 .. 1e3, predictions off by 1 % .. 100 % of the target's magnitude"""
    gen = torch.Generator().manual_seed(seed)
    r = lambda: torch.randn(count, generator=gen, dtype=torch.float64)
    mag = 10.0 ** (torch.rand(count, generator=gen, dtype=torch.float64) * 6 - 3)
    y = r() * mag
    pg = y + r() * mag * 10.0 ** (torch.rand(count, generator=gen, dtype=torch.float64) * 2 - 2)
    ps = y + r() * mag * 0.3
    return pg.to(DEV), ps.to(DEV), y.to(DEV)


def _run_loss(pg, ps, y, beta, with_sse=True):
    """-> (loss [1], dpg, dps, sse or None, the three padded output buffers)"""
    count = pg.numel()
    bufs = [torch.full((count + 8,), SENT, dtype=torch.float64, device=DEV) for _ in range(2)]
    dpg, dps = bufs[0][4:4 + count], bufs[1][4:4 + count]
    lbuf = torch.full((9,), SENT, dtype=torch.float64, device=DEV)
    sbuf = torch.full((10,), SENT, dtype=torch.float64, device=DEV)
    _ops().loss_phonon64(pg, ps, y, beta, dpg, dps, lbuf[4:5], sbuf[4:6] if with_sse else None)
    torch.cuda.synchronize()
    for b in bufs:
        assert bool((b[:4] == SENT).all()) and bool((b[4 + count:] == SENT).all()), "written outside the gradient"
    assert bool((lbuf[:4] == SENT).all()) and bool((lbuf[5:] == SENT).all())
    assert bool((sbuf[:4] == SENT).all()) and bool((sbuf[6:] == SENT).all()) and (with_sse or bool((sbuf == SENT).all()))
    return lbuf[4:5].clone(), dpg.clone(), dps.clone(), (sbuf[4:6].clone() if with_sse else None)


@pytest.mark.parametrize("beta", [0.0, 1.0, 0.3])
@pytest.mark.parametrize("count", [1, 51, 1024, 1025, 3264])
def test_loss_phonon_f64_against_float64_torch(count, beta):
    """loss within 1e-12 relative, each gradient within 1e-10 relative of its tensor's largest entry, the SSE pair within 1e-12;
    with and without sse the same numbers; two runs bitwise equal."""
    pg, ps, y = _loss_inputs(count, 100 + count)
    a, b = pg.clone().requires_grad_(True), ps.clone().requires_grad_(True)
    ref = torch.sqrt(F.mse_loss(a, y)) + beta * torch.sqrt(F.mse_loss(b, y))
    ref.backward()
    ref = ref.detach()
    loss, dpg, dps, sse = _run_loss(pg, ps, y, beta)
    e = (abs(float(loss) - float(ref)) / abs(float(ref)), _relmax(dpg, a.grad), _relmax(dps, b.grad))
    s_ref = torch.stack([((pg - y) ** 2).sum(), ((ps - y) ** 2).sum()])
    e_sse = float(((sse - s_ref).abs() / s_ref).max())
    print(f"loss_phonon64[count{count},beta{beta:g}]: loss {e[0]:.2e}  dpg {e[1]:.2e}  dps {e[2]:.2e}  sse {e_sse:.2e}")
    assert e[0] <= 1e-12 and e[1] <= 1e-10 and e[2] <= 1e-10 and e_sse <= 1e-12, (e, e_sse)
    if beta == 0.0:
        assert bool((dps == 0).all())
    again = _run_loss(pg, ps, y, beta)
    nosse = _run_loss(pg, ps, y, beta, with_sse=False)
    for x, x2, x3 in zip((loss, dpg, dps), again, nosse):
        assert torch.equal(x, x2) and torch.equal(x, x3)
    assert torch.equal(sse, again[3]) and nosse[3] is None


@pytest.mark.parametrize("count", [1, 51, 1025])
def test_loss_phonon_f64_zero_rmse_gives_zero_gradients(count):
    """pg == y: that branch's RMSE is exactly 0 and its gradient is written as finite zeros (autograd gives NaN there); the
    other branch is unchanged.  Both branches exact: loss 0, all gradients 0."""
    pg, ps, y = _loss_inputs(count, 200 + count)
    loss, dpg, dps, sse = _run_loss(y.clone(), ps, y, 0.7)
    b = ps.clone().requires_grad_(True)
    ref = 0.7 * torch.sqrt(F.mse_loss(b, y))
    ref.backward()
    ref = ref.detach()
    assert bool(torch.isfinite(dpg).all()) and bool((dpg == 0).all()) and float(sse[0]) == 0.0
    assert abs(float(loss) - float(ref)) <= 1e-12 * abs(float(ref)) and _relmax(dps, b.grad) <= 1e-10
    loss, dpg, dps, sse = _run_loss(y.clone(), y.clone(), y, 0.7)
    assert float(loss) == 0.0 and bool((dpg == 0).all()) and bool((dps == 0).all()) and bool((sse == 0).all())
    loss, dpg, dps, _ = _run_loss(pg, y.clone(), y, 0.7)
    assert bool((dps == 0).all()) and bool(torch.isfinite(dpg).all()) and float(dpg.abs().max()) > 0 and float(loss) > 0


def test_loss_phonon64_wrapper_checks_dtype_and_layout():
    o = _ops()
    pg, ps, y = _loss_inputs(51, 1)
    out = lambda: torch.empty(51, dtype=torch.float64, device=DEV)
    loss = torch.empty(1, dtype=torch.float64, device=DEV)
    with pytest.raises(TypeError):
        o.loss_phonon64(pg.float(), ps, y, 1.0, out(), out(), loss)
    with pytest.raises((TypeError, ValueError)):
        o.loss_phonon64(pg, ps, y, 1.0, torch.empty(51, 2, dtype=torch.float64, device=DEV)[:, 0], out(), loss)
    with pytest.raises(ValueError):
        o.loss_phonon64(pg, ps[:50], y, 1.0, out(), out(), loss)
    p = torch.zeros(8, dtype=torch.float64, device=DEV)
    with pytest.raises(TypeError):
        o.adamw64(p, p.float(), p.clone(), p.clone(), 8, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1)
    with pytest.raises(ValueError):
        o.adamw64(p, p.clone(), p.clone(), p.clone(), 9, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1)


# =====================================================================================================================
# 2. the AdamW kernel
# =====================================================================================================================
# One step in float64, u = 2^-53 (division and square root are correctly rounded: no fast-math in the build).  The host scalars
# decay = 1 - lr wd, 1 - b1, 1 - b2, step_size = lr / bc1, sqrt(bc2) with bc_k = 1 - b_k^step are computed in double on both sides
# with the same IEEE operations, as torch computes them in Python; the reference then takes them to long double.  Counted like
# the fp32 kernel (tests/test_gpu_tail.py, section C), whose arithmetic this is without the gradient scale:
#   m' = m + (g - m)(1 - b1)                the difference, the product (x 0.1), the sum: <= 3, held to 4 against |m| + |g|
#   v' = v b2 + (1 - b2) g g                three products and the sum, all terms >= 0: <= 4, held to 6 against v' itself
#   denom = sqrt(v') / sqrt(bc2) + eps      half of v' (3), sqrt, the division, the sum, 1 for the host's sqrt(bc2): 7
#   p' = p decay - step_size (m' / denom)   p decay: 1 against |p|; the final difference: 1 on both terms.
#                                           update term: m' 4 + denom 7 + division + product + 1 for the host's step_size +
#                                           difference: 15.  Together <= 16 against |p| + step_size (|m| + |g|) / denom
C_ADAM_M, C_ADAM_V, C_ADAM_P = 4, 6, 16
B1, B2, EPS = 0.9, 0.999, 1e-8
ADAM64_SWEEP = 2048 * 256 * 2               # doubles one sweep of the capped grid covers (csrc/adamw.hip)


def _adam_ref(p, g, m, v, step, lr, wd):
    """long-double update in torch's operation order from the double state; -> (p', m', v') and their scales"""
    L = np.longdouble
    assert np.finfo(L).eps <= 2.0 ** -63, "the host reference needs a long double wider than double"
    decay, step_size, bc2_sqrt = 1 - lr * wd, lr / (1 - B1 ** step), math.sqrt(1 - B2 ** step)
    p, g, m, v = (t.cpu().numpy().astype(L) for t in (p, g, m, v))
    p1 = p * L(decay)
    m1 = m + (g - m) * L(1 - B1)
    v1 = v * L(B2) + L(1 - B2) * g * g
    denom = np.sqrt(v1) / L(bc2_sqrt) + L(EPS)
    p2 = p1 - L(step_size) * (m1 / denom)
    return (p2, m1, v1), (np.abs(p) + L(step_size) * (np.abs(m) + np.abs(g)) / denom, np.abs(m) + np.abs(g), v1)


def _adam_state(n, step, seed):
    """Flat buffers of n + 8 doubles, sentinel-filled behind n: |p| over 1e-4 .. 10, |g| over 1e-8 .. 100 with gradients of
    exactly 0 and of 1e-30 among them; zero moments at step 1, moments of the gradients' own magnitude otherwise."""
    gen = torch.Generator().manual_seed(seed)
    u = lambda: torch.rand(n, generator=gen, dtype=torch.float64)
    r = lambda: torch.randn(n, generator=gen, dtype=torch.float64)
    gmag = 10.0 ** (u() * 10 - 8)
    g = r() * gmag
    perm = torch.randperm(n, generator=gen)
    g[perm[:max(1, min(100, n // 4))]] = 0.0
    if n >= 2:
        g[perm[n // 4 + 1:n // 4 + 1 + max(1, min(100, n // 4))]] = 1e-30
    vals = [r() * 10.0 ** (u() * 5 - 4), g]
    vals += [torch.zeros(n, dtype=torch.float64)] * 2 if step == 1 else [0.5 * r() * gmag, (r() * gmag) ** 2 * u()]
    out = []
    for t in vals:
        b = torch.full((n + 8,), SENT, dtype=torch.float64, device=DEV)
        b[:n] = t.to(DEV)
        out.append(b)
    return out


def _adam_check(n, p, g, m, v, step, lr, wd, tag):
    p0, g0, m0, v0 = p.clone(), g.clone(), m.clone(), v.clone()
    _ops().adamw64(p, g, m, v, n, lr, B1, B2, EPS, wd, step)
    torch.cuda.synchronize()
    refs, scales = _adam_ref(p0[:n], g0[:n], m0[:n], v0[:n], step, lr, wd)
    for name, got, ref, sc, c in zip("pmv", (p, m, v), refs, scales, (C_ADAM_P, C_ADAM_M, C_ADAM_V)):
        err = np.abs(got[:n].cpu().numpy().astype(np.longdouble) - ref)
        bound = np.longdouble(c * U64) * sc
        worst = float(np.max(err / np.maximum(bound, np.finfo(np.longdouble).tiny)))
        assert bool(np.all(err <= bound)), (tag, name, worst)
        assert bool((got[n:] == SENT).all()), tag + ": written behind n"
    assert torch.equal(g, g0), tag + ": gradient changed"
    zero = (g0[:n] == 0) & (m0[:n] == 0) & (v0[:n] == 0)          # 0 / eps = 0: exactly the product p decay
    if bool(zero.any()):
        assert torch.equal(p[:n][zero], p0[:n][zero] * (1 - lr * wd)) and bool((m[:n][zero] == 0).all()) and bool((v[:n][zero] == 0).all())


@pytest.mark.parametrize("step,wd,lr", [(1, 1e-2, 1e-3), (1000, 1e-2, 1e-4), (1000, 0.0, 1e-3)])
@pytest.mark.parametrize("n", [1, 2, 3, 255, 1025, 2 * ADAM64_SWEEP + 2 * 256 * 3 + 1])
def test_adamw_f64_step(n, step, wd, lr):
    """One element (the scalar tail alone), one pair, pair + tail, a partial workgroup, 256 k + 1, and two full grid-stride
    sweeps of the capped launch + a partial third + the tail."""
    p, g, m, v = _adam_state(n, step, 301 + n % 1000)
    _adam_check(n, p, g, m, v, step, lr, wd, f"adamw64[n{n},step{step},wd{wd:g},lr{lr:g}]")


def test_adamw_f64_three_steps_against_torch_adamw():
    n = 1003
    gen = torch.Generator().manual_seed(7)
    p0 = torch.randn(n, generator=gen, dtype=torch.float64)
    grads = [torch.randn(n, generator=gen, dtype=torch.float64) * 10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 6 - 4)
             for _ in range(3)]
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([ref], lr=1e-3, betas=(B1, B2), eps=EPS, weight_decay=1e-2)
    bufs = [torch.zeros(n + 1, dtype=torch.float64, device=DEV) for _ in range(4)]
    p, g, m, v = bufs
    p[:n] = p0.to(DEV)
    for step, gr in enumerate(grads, 1):
        ref.grad = gr.clone()
        opt.step()
        g[:n] = gr.to(DEV)
        _ops().adamw64(p, g, m, v, n, 1e-3, B1, B2, EPS, 1e-2, step)
    st = opt.state[ref]
    assert float((p[:n].cpu() - ref.detach()).abs().max()) <= 1e-9
    assert _relmax(m[:n].cpu(), st["exp_avg"]) <= 1e-12 and _relmax(v[:n].cpu(), st["exp_avg_sq"]) <= 1e-12


# =====================================================================================================================
# 3 - 6. Trainer64
# =====================================================================================================================
L_, T_, H_, S_ = 2, 2, 32, 51
ATOMS_A = [3, 7, 19, 12]           # one crystal's keys cross a 16-key tile
ATOMS_B = [5, 2, 18]


def _crystals(n_atoms, seed):
    from dostransformer_amd import synth
    gen = torch.Generator().manual_seed(seed)
    return [synth.phonon_crystal(gen, n) for n in n_atoms]


def _collate(cs):
    from dostransformer_amd.batch import collate
    return collate(cs)


def _module(attn_drop=0.0, seed=41):
    from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
    torch.manual_seed(seed)
    return DOSTransformer_phonon(L_, T_, 118, 4, H_, "cpu", attn_drop).double()


def _switch(module, pck=True):
    return module.set_program_dtype(torch.float64).set_per_crystal_keys(pck).to(DEV)


def _torch_loss(dg, ds, y, beta):
    return torch.sqrt(F.mse_loss(dg, y)) + beta * torch.sqrt(F.mse_loss(ds, y))


def _per_tensor(fp, got, ref, tol, tag):
    worst = 0.0
    for n, o in zip(fp.names, fp.offsets):
        k = fp.P[n].numel()
        e = _relmax(got[o:o + k], ref[o:o + k])
        worst = max(worst, e)
        assert e <= tol, (tag, n, e)
    return worst


@pytest.mark.parametrize("pck", [True, False], ids=["per_crystal", "padded_keys"])
def test_trainer64_eager_against_the_hand_written_loop(pck):
    """Two deep copies of one module, three steps each: Trainer64.step against model(batch), torch loss, backward,
    torch.optim.AdamW.  Losses within 1e-12 relative, the flat gradients of step 1 within 1e-10 relative per tensor, every
    parameter after step 3 within 1e-9."""
    from dostransformer_amd.train64 import Trainer64
    base = _module()
    hand, fused = _switch(copy.deepcopy(base), pck), _switch(copy.deepcopy(base), pck)
    lr, beta = 1e-3, 0.7
    g = _collate(_crystals(ATOMS_A, 51)).to(DEV)
    opt = torch.optim.AdamW(hand.parameters(), lr=lr, weight_decay=1e-2)
    tr = Trainer64(fused, lr=lr, beta=beta)
    for step in range(3):
        opt.zero_grad()
        dg, _, ds = hand(g)
        ref = _torch_loss(dg, ds, g.phdos, beta)
        ref.backward()
        loss = tr.step(g)
        assert loss.dtype == torch.float64 and loss.dim() == 0 and loss.is_cuda
        e = abs(float(loss) - float(ref.detach())) / abs(float(ref.detach()))
        assert e <= 1e-12, (step, e)
        if step == 0:
            worst = _per_tensor(tr._fp, tr._fp.grad, hand.flat_params().grad, 1e-10, "grad")
            print(f"pck={pck}: loss error {e:.2e}, worst per-tensor flat gradient error {worst:.2e}")
            out = tr.last_outputs
            assert torch.equal(out[0], dg) and torch.equal(out[2], ds) and out[1].shape == (sum(ATOMS_A), H_)
        opt.step()
    assert tr.step_count == 3
    a, b = fused.state_dict(), hand.state_dict()
    for k, v in b.items():
        if v.is_floating_point():
            assert float((a[k] - v).abs().max()) <= 1e-9, k
    assert float((a["embeddings.weight"] - base.state_dict()["embeddings.weight"].to(DEV)).abs().max()) > 1e-4      # it trained


def _soft64_mha(q, k, v, drop_mask=None):
    dim = q.shape[2]
    w = torch.bmm(q.transpose(0, 1), k.transpose(0, 1).transpose(1, 2)) * (dim ** -0.5)
    w = F.softmax(w, dim=-1)
    if drop_mask is not None:
        w = w * drop_mask.to(w.dtype)
    return torch.bmm(w, v.transpose(0, 1)).transpose(0, 1)


def test_trainer64_against_the_oracle_crystal_by_crystal(monkeypatch):
    """fp64 softmax on both sides, per-crystal keys: three steps against the float64 oracle run on every crystal alone, the
    batch loss over the concatenated DOS vectors and torch.optim.AdamW on the CPU.  Parameters within 1e-9."""
    from oracle import dos_oracle as O
    from dostransformer_amd import functional64 as F64
    from dostransformer_amd.train64 import Trainer64
    monkeypatch.setattr(O, "multihead_attention", _soft64_mha)
    monkeypatch.setattr(F64, "SOFTMAX64", True)
    base = _module()
    lr, beta = 1e-3, 1.0
    cs = _crystals(ATOMS_A, 51)
    singles = [_collate([c]) for c in cs]
    phdos = _collate(cs).phdos
    pr = {k: (torch.nn.Parameter(v.detach().clone()) if v.is_floating_point() else v.clone()) for k, v in base.state_dict().items()}
    opt = torch.optim.AdamW([v for v in pr.values() if isinstance(v, torch.nn.Parameter)], lr=lr, weight_decay=1e-2)
    model = _switch(copy.deepcopy(base))
    tr = Trainer64(model, lr=lr, beta=beta)
    gd = _collate(cs).to(DEV)
    for step in range(3):
        opt.zero_grad()
        outs = [O.dostransformer_phonon_forward(pr, g1, L_, T_) for g1 in singles]
        ref = O.loss_phonon(torch.cat([o[0] for o in outs]), torch.cat([o[2] for o in outs]), phdos, beta)
        ref.backward()
        opt.step()
        loss = tr.step(gd)
        ref = float(ref.detach())
        print(f"step {step}: loss {float(loss):.15g}, oracle {ref:.15g}")
        if step == 0:
            assert abs(float(loss) - ref) <= 1e-12 * abs(ref), (float(loss), ref)
    sd = model.state_dict()
    worst = 0.0
    for k, v in pr.items():
        if v.is_floating_point():
            d = float((sd[k].cpu() - v.detach()).abs().max())
            worst = max(worst, d)
            assert d <= 1e-9, (k, d)
    print(f"largest parameter difference after 3 steps: {worst:.2e}")


def _run(replay, steps, batches, seed=97, max_slots=32, attn_drop=0.1, touch=None):
    """``steps`` alternating steps of a fresh dropout-on module: -> (losses, flat clones, trainer, model).  touch: step index in
    front of which batch 0's target is written in place."""
    from dostransformer_amd.train64 import Trainer64
    model = _switch(_module(attn_drop)).train()
    torch.manual_seed(seed)                     # the dropout seed is drawn from torch's RNG at the first step
    tr = Trainer64(model, lr=1e-3, replay=replay, max_slots=max_slots)
    gs = [b.clone().to(DEV) for b in batches]
    losses, flats = [], []
    for i in range(steps):
        if touch is not None and i == touch:
            gs[0].phdos.mul_(0.5)
        losses.append(tr.step(gs[i % len(gs)]).clone())
        flats.append(tr._fp.flat.clone())
    return losses, flats, tr, model


@pytest.fixture(scope="module")
def two_batches():
    return [_collate(_crystals(ATOMS_A, 51)), _collate(_crystals(ATOMS_B, 52))]


@pytest.fixture(scope="module")
def eager_run(two_batches):
    return _run(False, 8, two_batches, touch=6)


def test_trainer64_replay_is_bitwise_eager(two_batches, eager_run):
    """Two shapes alternated, attention dropout 0.1: six steps + two more after batch 0's target was written in place; every
    loss and the flat parameters after every step torch.equal between replay = False and replay = True.  Two recordings."""
    el, ef, etr, _ = eager_run
    rl, rf, rtr, _ = _run(True, 8, two_batches, touch=6)
    for i in range(8):
        assert torch.equal(el[i], rl[i]) and torch.equal(ef[i], rf[i]), i
    assert (rtr.slot_misses, rtr.slot_hits) == (2, 6) and (etr.slot_misses, etr.slot_hits) == (0, 0)
    assert not torch.equal(el[6], el[4]) and float((el[6] - el[4]).abs()) > 1e-3       # (the written target changed the loss)
    assert all(len(s.prog) > 50 for s in rtr._slots.values())
    assert float((ef[0] - ef[5]).abs().max()) > 1e-4


def test_trainer64_replay_with_one_slot_and_refusals(two_batches, eager_run):
    """max_slots = 1: alternating shapes evict each other, every step records, the numbers are still the eager ones.  A
    ghost-padded batch is refused; a slot recorded with per-crystal keys is not replayed without them."""
    from dostransformer_amd._lib import DosxError
    from dostransformer_amd.batch import pad_batch
    el, ef, _, _ = eager_run
    rl, rf, rtr, model = _run(True, 4, two_batches, max_slots=1)
    for i in range(4):
        assert torch.equal(el[i], rl[i]) and torch.equal(ef[i], rf[i]), i
    assert (rtr.slot_misses, rtr.slot_hits, len(rtr._slots)) == (4, 0, 1)
    g = two_batches[0].clone().to(DEV)
    padded = pad_batch(g, g.x.shape[0] + 5, g.edge_index.shape[1] + 128)
    for tr in (rtr, eager_run[2]):
        before = tr.step_count
        with pytest.raises(DosxError, match="padded"):
            tr.step(padded)
        assert tr.step_count == before
    rtr.max_slots = 4
    rtr.step(g)
    rtr.step(g)
    assert (rtr.slot_misses, rtr.slot_hits) == (5, 1)
    model.set_per_crystal_keys(False)
    rtr.step(g)
    assert (rtr.slot_misses, rtr.slot_hits) == (6, 1)


@pytest.mark.parametrize("replay", [False, True], ids=["eager", "replay"])
def test_trainer64_checkpoint_resumes_bitwise(two_batches, eager_run, replay):
    """state_dict() after two steps into a fresh module + a fresh Trainer64, two more steps: bitwise the uninterrupted four
    (dropout on: the resumed run draws the masks the uninterrupted one drew)."""
    from dostransformer_amd.train64 import Trainer64
    el, ef, _, _ = eager_run
    _, _, tr, model = _run(replay, 2, two_batches)
    sd = copy.deepcopy(tr.state_dict())
    msd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    assert sd["step"] == 2 and all(v.dtype == torch.float64 for v in sd["exp_avg"].values())
    fresh = _module(0.1, seed=5)
    fresh.load_state_dict(msd)
    fresh = _switch(fresh).train()
    tr2 = Trainer64(fresh, replay=replay)
    tr2.load_state_dict(sd)
    assert tr2.step_count == 2 and tr2.lr == 1e-3
    gs = [b.clone().to(DEV) for b in two_batches]
    for i in (2, 3):
        loss = tr2.step(gs[i % 2])
        assert torch.equal(loss, el[i]) and torch.equal(tr2._fp.flat, ef[i]), i
