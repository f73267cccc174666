"""Normalised functionals in the fused trainers on a real MI355X (dosx_loss_rows_fn_norm): ``functionals=`` with
rows divided by one floored denominator functional - ``stack(centre(...), normalised_cumulative(...))``, the band centre / mean
frequency and the cumulative curve of the DOS as a shape.  Models, batches, bars and helpers are those of
tests/test_gpu_trainer_functionals.py.

The reference of the gradient tests is float64 autograd through the oracle's batch-1 forwards of the definition in
include/dosx.h, written out below (``_term_norm``): every row of this table is normalised,
``u_k = F_k(p) / max(D(p), floor) - F_k(t) / max(D(t), floor)``, ``l_b = rmse(pg_b) + beta rmse(ps_b) + lam / K sum_k e(u_k(pg_b)) +
beta lam / K sum_k e(u_k(ps_b))``, ``loss = mean_b l_b``.  The reference is unambiguous on these inputs (asserted): no oracle
prediction or target has its ``D`` within 1e-3 sum_s |den_s x_s| of the floor, and under "abs" no ``u_k`` on the kink.

What is bitwise here is bitwise by construction: a replayed or captured step issues the eager step's launches on the same
buffers; table and denominator are one trainer-owned buffer that ``set_functionals`` overwrites in place; a table without
normalised rows takes the path of DESIGN.md 9.12."""
import copy

import pytest
import torch

from tests import test_gpu_baselines64 as B64
from tests import test_gpu_train64 as T64
from tests import test_gpu_train_per_crystal as PC
from tests.gpu_util import DEV
from tests.test_gpu_trainer_functionals import CASES, LAM, _F, _S, _cdf
from tests.test_gpu_trainer_guard import _same, _state
from tests.test_gpu_trainer_loss import _fam

pytestmark = pytest.mark.gpu

# In the units of m0 = sum_s p_s / S on the unit grid.  The targets' m0 is about 0.5; an untrained model's outputs are signed, with
# m0 anywhere in -2 .. 1: about half of the predictions below lie under this floor (their denominator is the constant) and half
# above it, and a floored ratio stays of order 1.
FLOOR = 0.25
SEED = 53                              # T64.ATOMS_A crystals: the first seed from 51 on at which the reference is unambiguous


def _fn(S, floor=FLOOR):
    """centre and the normalised cumulative curve on a grid of unit length (bin width 1 / S): S rows, all over m0"""
    F = _F()
    e = (torch.arange(S, dtype=torch.float64) + 0.5) / S
    return F.stack(F.centre(e, floor, de=1.0 / S), F.normalised_cumulative(S, floor, de=1.0 / S))


def _term_norm(p, t, fn, kind):
    """(1 / K) sum_k e(u_k) of the definition, every row normalised; p, t [B,S] float64"""
    p = p.reshape(t.shape)
    assert fn.K_norm == fn.K
    u = (p @ fn.table.T) / (p @ fn.denominator).clamp(min=fn.floor)[:, None] \
        - (t @ fn.table.T) / (t @ fn.denominator).clamp(min=fn.floor)[:, None]
    return (u ** 2 if kind == "sq" else u.abs()).mean(1)


def _assert_unambiguous(p, t, fn, kind):
    p, t = p.detach().reshape(1, -1), t.detach().reshape(1, -1)
    for x in (p, t):
        assert bool(((x @ fn.denominator - fn.floor).abs() >= 1e-3 * (x.abs() @ fn.denominator.abs())).all())
    if kind == "abs":
        Dp, Dt = (p @ fn.denominator).clamp(min=fn.floor)[:, None], (t @ fn.denominator).clamp(min=fn.floor)[:, None]
        u = (p @ fn.table.T) / Dp - (t @ fn.table.T) / Dt
        U = (p.abs() @ fn.table.abs().T) / Dp + (t.abs() @ fn.table.abs().T) / Dt
        assert bool((u.abs() >= 1e-4 * U).all())


def _crystal_loss(dg, ds, y, beta, fn, kind, lam):
    """l_b of the definition for a batch of ONE crystal, float64 torch"""
    y = y.reshape(1, -1)
    rm = lambda p: torch.sqrt(((p.reshape(y.shape) - y) ** 2).mean())
    l = rm(dg) + lam * _term_norm(dg, y, fn, kind)[0]
    if ds is not None:
        l = l + beta * (rm(ds) + lam * _term_norm(ds, y, fn, kind)[0])
    return l


# =====================================================================================================================
# 1. the gradient of one step against float64 autograd through the oracle
# =====================================================================================================================
@pytest.mark.parametrize("kind", ["sq", "abs"])
def test_normalised_step_is_the_mean_of_the_batch_1_gradients_f64(monkeypatch, kind):
    """Trainer64, set_per_crystal_keys(True), fp64 softmax on both sides, loss="crystal_rmse" with centre + normalised cumulative
    on the four T64.ATOMS_A crystals: loss and crystal_losses within 1e-12 relative, every tensor of the flat gradient within
    1e-10 of its largest entry."""
    from oracle import dos_oracle as O
    from dostransformer_amd import functional64 as F64
    from dostransformer_amd.train64 import Trainer64
    monkeypatch.setattr(O, "multihead_attention", T64._soft64_mha)
    monkeypatch.setattr(F64, "SOFTMAX64", True)
    base = T64._module()
    beta = 0.7
    cs = T64._crystals(T64.ATOMS_A, SEED)
    fn = _fn(51)
    pr = {k: (v.detach().clone().requires_grad_(True) if v.is_floating_point() else v.clone()) for k, v in base.state_dict().items()}
    losses, plain = [], []
    for cr in cs:
        g1 = T64._collate([cr])
        out = O.dostransformer_phonon_forward(pr, g1, T64.L_, T64.T_)
        losses.append(_crystal_loss(out[0], out[2], g1.phdos, beta, fn, kind, LAM))
        plain.append(O.loss_phonon(out[0], out[2], g1.phdos, beta).detach())
        for p in (out[0], out[2]):
            _assert_unambiguous(p, g1.phdos, fn, kind)
    each = torch.stack(losses)
    ref = each.mean()
    ref.backward()
    assert float(ref.detach()) - float(torch.stack(plain).mean()) > 1e-6                # input condition: the term is there
    tr = Trainer64(T64._switch(copy.deepcopy(base), True), lr=1e-3, beta=beta, loss="crystal_rmse", functionals=fn,
                   functional_kind=kind, functional_weight=LAM)
    loss = tr.forward_backward(T64._collate(cs).to(DEV))
    e = abs(float(loss) - float(ref.detach())) / abs(float(ref.detach()))
    assert e <= 1e-12, e
    assert float(((tr.crystal_losses.cpu() - each.detach()).abs() / each.detach()).max()) <= 1e-12
    worst = 0.0
    for k, got in tr._fp.G.items():
        r = pr[k].grad
        d = float((got.detach().cpu() - r).abs().max() / (r.abs().max() + 1e-300))
        worst = max(worst, d)
        assert d <= 1e-10, (k, d)
    print(f"t64 crystal_rmse + normalised {kind}: loss error {e:.2e}, worst per-tensor gradient error {worst:.2e}")


def test_normalised_step_is_the_mean_of_the_batch_1_gradients_fp32():
    """Trainer(per_crystal_keys=True, loss="crystal_rmse", functionals=centre + normalised cumulative) on ph_h64, by the
    element-error rule of tests/test_gpu_train_per_crystal.py; loss and crystal_losses within (1 + beta) 1e-4."""
    from dostransformer_amd.train import Trainer
    name = "ph_h64"
    c = PC.MODELS[name]
    cs = PC._crystals(name)
    model, p = PC._model(name)
    fn = _fn(int(model._cfg.S))
    leaves = PC._leaves(p)
    names = list(leaves)
    losses, plain = [], []
    for cr in cs:
        g1 = PC._collate([cr]).to("cpu", dtype=torch.float64)
        dg, _, ds = PC._oracle_fwd("phonon", leaves, g1, c["L"], c["T"])
        losses.append(_crystal_loss(dg, ds, g1.phdos, PC.BETA, fn, "sq", LAM))
        plain.append(_crystal_loss(dg, ds, g1.phdos, PC.BETA, fn, "sq", 0.0))
        for q in (dg, ds):
            _assert_unambiguous(q, g1.phdos, fn, "sq")
    each = torch.stack(losses)
    ref = each.mean()
    grads = dict(zip(names, torch.autograd.grad(ref, [leaves[k] for k in names], allow_unused=True, retain_graph=True)))
    unw = dict(zip(names, torch.autograd.grad(torch.stack(plain).mean(), [leaves[k] for k in names], allow_unused=True)))
    diff = max(float((unw[k] - r).abs().max() / (r.abs().max() + 1e-300)) for k, r in grads.items() if r is not None)
    print(f"{name}: gradient without the term against the one with it: largest per-tensor difference {diff:.3f}")
    assert diff >= 0.05, diff                                   # input condition: far above the comparison's bar
    tr = Trainer(model, beta=PC.BETA, per_crystal_keys=True, loss="crystal_rmse", functionals=fn, functional_weight=LAM)
    loss = tr.forward_backward(PC._collate(cs).to(DEV))
    print(f"{name}: loss {float(loss):.8f}, of the batch-1 oracle losses {float(ref.detach()):.8f}")
    assert abs(float(loss) - float(ref.detach())) < (1 + PC.BETA) * 1e-4
    assert float((tr.crystal_losses.cpu().double() - each.detach()).abs().max()) < (1 + PC.BETA) * 1e-4
    PC._assert_grads(name + " crystal_rmse + normalised", model.flat_params().G, grads)


def test_normalised_step_against_the_oracle_gn64():
    """GraphnetworkTrainer64 (one output) on five synthetic crystals: loss 1e-12 relative, every gradient tensor within 1e-10 of
    its largest entry (the bars of tests/test_gpu_baselines64.py::test_trainer64_against_the_float64_oracle)."""
    from oracle import dos_oracle as O
    from dostransformer_amd import synth
    base = B64._gn(64, seed=0)
    g = synth.phonon_batch(5, seed=70, dtype=torch.float64)
    fn = _fn(51)
    pr = {k: (torch.nn.Parameter(v.detach().clone()) if v.is_floating_point() else v.clone()) for k, v in base.state_dict().items()}
    dos = O.graphnetwork_phonon_forward(pr, g, B64.L_)
    y = g.phdos.reshape(dos.shape)
    for b in range(dos.shape[0]):
        _assert_unambiguous(dos[b], y[b], fn, "sq")
    each = torch.sqrt(((dos - y) ** 2).mean(1)) + LAM * _term_norm(dos, y, fn, "sq")
    ref = each.mean()
    ref.backward()
    tr = B64._trainer(copy.deepcopy(base).to(DEV), lr=1e-3, loss="crystal_rmse", functionals=fn, functional_weight=LAM)
    loss = tr.forward_backward(g.clone().to(DEV))
    e = abs(float(loss) - float(ref.detach())) / abs(float(ref.detach()))
    assert e <= 1e-12, e
    assert float(((tr.crystal_losses.cpu() - each.detach()).abs() / each.detach()).max()) <= 1e-12
    worst, n = 0.0, 0
    for k, v in pr.items():
        if isinstance(v, torch.nn.Parameter) and v.grad is not None:
            ek = B64._relmax(tr._fp.G[k].cpu(), v.grad)
            worst, n = max(worst, ek), n + 1
            assert ek <= 1e-10, (k, ek)
    assert n > 10
    print(f"gn64 crystal_rmse + normalised: loss error {e:.2e}, worst per-tensor gradient error {worst:.2e}")


# =====================================================================================================================
# 2. mode equivalences
# =====================================================================================================================
@pytest.mark.parametrize("name,mode", CASES, ids=[f"{c}-{m}" for c, m in CASES])
def test_replay_and_graph_are_bitwise_eager(name, mode):
    from dostransformer_amd.batch import bucket_sizes, pad_batch
    c = _fam(name)
    fn = _fn(_S(c))
    for kind, loss in (("sq", "crystal_rmse"), ("abs", "mse")):
        kw = dict(loss=loss, functionals=fn, functional_kind=kind, functional_weight=LAM)
        eager, _ = c.trainer("eager", **kw)
        other, _ = c.trainer(mode, **kw)
        pad = (lambda g: g) if c.f64 else (lambda g: pad_batch(g, *bucket_sizes(g.meta.num_nodes, g.meta.num_edges, *other.bucket)))
        for step in range(3):
            assert torch.equal(eager.step(pad(c.g)), other.step(c.g)), (kind, step)
            assert torch.equal(eager.crystal_losses, other.crystal_losses), (kind, step)
        assert _same(_state(eager), _state(other)), kind
        assert (other.slot_misses, other.slot_hits) == (1, 2)
    # the term is in the objective, through the normalised entry, in the launches of the trainer without it
    plain, _ = c.trainer("eager", loss="crystal_rmse")
    with_term, _ = c.trainer("eager", loss="crystal_rmse", functionals=fn, functional_weight=LAM)
    assert float(with_term.forward_backward(pad(c.g))) > float(plain.forward_backward(pad(c.g)))
    if not c.f64:
        assert "dosx_loss_rows_fn_norm_desc" in with_term.program_stats()["entries"]
        assert with_term.program_stats()["launches"] == plain.program_stats()["launches"]


def test_a_window_of_two_and_two_is_the_step_on_the_four_f64():
    """Trainer64, window [2, 2] against ONE step on the four crystals with the normalised term: the pair's bars of
    tests/test_gpu_trainer_accumulate.py (2e-12 relative in the loss, 2e-10 of the tensor's largest entry in the gradient)."""
    from dostransformer_amd.train64 import Trainer64
    base = T64._module()
    cs = T64._crystals(T64.ATOMS_A, SEED)
    fn = _fn(51)
    mk = lambda: Trainer64(T64._switch(copy.deepcopy(base), True), lr=1e-3, beta=0.7, loss="crystal_rmse", functionals=fn,
                           functional_weight=LAM)
    tr, one = mk(), mk()
    lw = tr.step_accumulate([T64._collate(cs[:2]).to(DEV), T64._collate(cs[2:]).to(DEV)])
    l1 = one.step(T64._collate(cs).to(DEV))
    assert abs(float(lw) - float(l1)) <= 2e-12 * abs(float(l1))
    assert tr.crystal_losses.shape == (4,)
    assert float(((tr.crystal_losses - one.crystal_losses).abs() / one.crystal_losses).max()) <= 2e-12
    pair = 0.0
    for k, got in tr._fp.G.items():
        r = one._fp.G[k].detach()
        pair = max(pair, float((got.detach() - r).abs().max() / (r.abs().max() + 1e-300)))
    print(f"t64 window [2, 2] with the normalised term against one step: worst per-tensor gradient difference {pair:.2e}")
    assert pair <= 2e-10


@pytest.mark.parametrize("name", ["phonon", "t64", "gn64"])
def test_set_functionals_is_read_by_the_next_replayed_step(name):
    """lr = 0 and no weight decay: the parameters stand still, a step's loss and flat gradient are functions of the table alone.
    Two replayed steps with table A, set_functionals(B) - other rows AND another denominator, the same K, K_norm and floor -, a
    third: no new recording (slot counts), the buffer's address is the same, and loss, crystal_losses and gradient are bitwise
    those of a trainer CONSTRUCTED with B.  Another K_norm or floor is refused."""
    F = _F()
    c = _fam(name)
    S = _S(c)
    fa = _fn(S)
    e = (torch.arange(S, dtype=torch.float64) + 0.5) / S
    # B: the second moment and the cumulative rows over a denominator that weighs the upper half of the grid double
    den = torch.where(e > 0.5, 2.0, 1.0) / S
    fb = F.normalised(F.stack(F.moments(e, orders=(2,), de=1.0 / S), F.Functionals(_cdf(S).table[:S - 1])), den, FLOOR)
    assert (fb.K, fb.K_norm, fb.floor) == (fa.K, fa.K_norm, fa.floor) and not torch.equal(fa.table, fb.table)
    assert not torch.equal(fa.denominator, fb.denominator)
    kw = dict(loss="crystal_rmse", functional_kind="sq", functional_weight=LAM)

    def still(tr):
        tr.lr = tr.wd = 0.0
        return tr

    a = still(c.trainer("replay", functionals=fa, **kw)[0])
    b = still(c.trainer("replay", functionals=fb, **kw)[0])
    l0 = a.step(c.g).clone()
    ptr = a._fn_dev.data_ptr()
    assert torch.equal(a.step(c.g), l0)
    assert (a.slot_misses, a.slot_hits, len(a._slots)) == (1, 1, 1)
    a.set_functionals(fb)
    la, lb = a.step(c.g), b.step(c.g)
    assert (a.slot_misses, a.slot_hits, len(a._slots)) == (1, 2, 1) and a._fn_dev.data_ptr() == ptr
    assert torch.equal(la, lb) and not torch.equal(la, l0)
    assert torch.equal(a.crystal_losses, b.crystal_losses)
    torch.cuda.synchronize()
    assert torch.equal(a._fp.grad, b._fp.grad) and torch.equal(a._fp.flat, b._fp.flat)
    with pytest.raises(ValueError, match="normalised rows"):
        a.set_functionals(F.Functionals(fb.table, fb.names, denominator=den, norm_rows=range(fa.K - 1), floor=FLOOR))
    with pytest.raises(ValueError, match="floor"):
        a.set_functionals(F.Functionals(fb.table, fb.names, denominator=den, norm_rows=range(fa.K), floor=2 * FLOOR))
    assert (a.slot_misses, a.slot_hits) == (1, 2)


@pytest.mark.parametrize("name,mode", [(c, m) for c in ("phonon", "t64", "gn64") for m in ("eager", "replay")])
def test_a_table_without_normalised_rows_trains_the_bits_of_the_linear_trainer(name, mode):
    """A Functionals that went through the new builders' machinery but has no normalised row - stack() of plain parts - issues
    dosx_loss_rows_fn and trains the bits of the trainer given the bare table."""
    F = _F()
    c = _fam(name)
    S = _S(c)
    fn = F.stack(F.Functionals(_cdf(S).table[:S - 1]), F.moments(torch.linspace(0.0, 1.0, S), orders=(0,), de=1.0 / S))
    assert fn.K_norm == 0 and fn.denominator is None
    kw = dict(loss="crystal_rmse", functional_kind="abs", functional_weight=LAM)
    bare, _ = c.trainer(mode, functionals=fn.table.clone(), **kw)
    new, _ = c.trainer(mode, functionals=fn, **kw)
    for step in range(3):
        assert torch.equal(bare.step(c.g), new.step(c.g)), step
        assert torch.equal(bare.crystal_losses, new.crystal_losses), step
    assert _same(_state(bare), _state(new))
    if not c.f64:
        entries = new.program_stats()["entries"]
        assert "dosx_loss_rows_fn" in entries and not any("fn_norm" in n for n in entries)
