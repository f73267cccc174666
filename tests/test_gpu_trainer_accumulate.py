"""``step_accumulate`` / ``step_dataset_accumulate`` of the fused trainers on a real MI355X: several micro-batches, ONE optimizer
step on the objective of the concatenated batch (csrc/grad_accumulate.hip).  The models, batches and bars are those
of tests/test_gpu_trainer_loss.py (L2 T2 H32, 4 - 5 synthetic crystals), ``ph_h64`` of tests/test_gpu_train_per_crystal.py and
``T64.ATOMS_A``; the windows are ragged - 2 + 1 + 1 or 2 + 1 + 2 crystals - so that the mean of the per-batch means is not the
mean over crystals.

What is bitwise here is bitwise by construction: the window's gradient is ``((G1 + G2) + G3)`` of the gradients a twin trainer's
public ``forward_backward(g_k, n_global=T)`` leaves (eDOS default loss: the one objective whose public route takes a foreign
count), summed with torch on the device; parameters and moments are ``ops.adamw`` - or the twin's own ``optimizer_step()`` under the
same options - applied to that sum.  What is compared with the float64 oracle keeps the bars of the tests it shares the
reference with."""
import copy

import numpy as np
import pytest
import torch

from tests import test_gpu_train64 as T64
from tests import test_gpu_train_per_crystal as PC
from tests.gpu_util import DEV
from tests.test_gpu_trainer_guard import _same, _state
from tests.test_gpu_trainer_loss import CASES, FAMILIES, _fam

pytestmark = pytest.mark.gpu

SIZES = {"phonon": (2, 1, 1), "edos": (2, 1, 1), "t64": (2, 1, 1), "gn64": (2, 1, 2), "gnp": (2, 1, 2)}
_CUTS = {}


def _cut(name):
    """the family's batch cut into its ragged micro-batches (made once, shared, never written to)"""
    if name not in _CUTS:
        from dostransformer_amd.batch import collate, split_crystals
        cs = split_crystals(_fam(name).g)
        assert sum(SIZES[name]) == len(cs)
        out, o = [], 0
        for s in SIZES[name]:
            out.append(collate(cs[o:o + s]).to(DEV))
            o += s
        _CUTS[name] = out
    return _CUTS[name]


def _padded(g, bucket=(8, 128)):
    """the batch as the fp32 trainer's replay sees it: the eager twin runs on it (ghost rows are exact, but they change shapes)"""
    from dostransformer_amd.batch import bucket_sizes, pad_batch
    return pad_batch(g, *bucket_sizes(g.meta.num_nodes, g.meta.num_edges, *bucket))


def _seed(tr):
    s = getattr(tr.model, "_drop_seed", None)
    return None if s is None else int(s.item())


def _sum_in_order(ts):
    out = ts[0]
    for t in ts[1:]:
        out = torch.add(out, t)
    return out


def _compose(twin, gs, T):
    """What a window is made of, by the twin's PUBLIC entries: forward_backward(g_k, n_global=T) for every micro-batch, the flat
    gradients and the losses summed with torch in the window's order, the sum written into the twin's gradient buffer -
    ``twin.optimizer_step()`` (or ops.adamw) then steps on it.  -> (the summed gradient, the summed loss, n_train)"""
    Gs, Ls = [], []
    for g in gs:
        loss = twin.forward_backward(g, n_global=T)
        Gs.append(twin._fp.grad.clone())
        Ls.append(loss.clone())
    G, L, n = _sum_in_order(Gs), _sum_in_order(Ls), twin._fp.n_train
    twin._fp.grad[:n].copy_(G[:n])
    return G, L, n


def _twin_batches(mode, gs):
    return [_padded(g) for g in gs] if mode == "replay" else gs


# =====================================================================================================================
# 1. exactness
# =====================================================================================================================
@pytest.mark.parametrize("mode", ["eager", "replay"])
def test_window_is_the_sum_of_the_twins_gradients_and_adamw_on_it(mode):
    from dostransformer_amd import ops
    c, gs = _fam("edos"), _cut("edos")
    T = sum(SIZES["edos"])
    tr, _ = c.trainer(mode)
    twin, _ = c.trainer("eager")
    loss = tr.step_accumulate(gs)
    G, L, n = _compose(twin, _twin_batches(mode, gs), T)
    assert n == tr._fp.n_train and n > 0
    assert torch.equal(tr._fp.grad[:n], G[:n])
    assert loss.dim() == 0 and loss.is_cuda and torch.equal(loss, L)
    fp = twin._fp
    ops.adamw(fp.flat, G, twin._m, twin._v, n, 1e-4, 0.9, 0.999, 1e-8, 1e-2, 1)
    assert _same(_state(tr), _state(twin))
    assert (tr.step_count, twin.step_count) == (1, 0) and tr.crystal_losses is None
    # not the sum of three own-count steps' gradients: every micro-batch was normalised by T, not by its own count
    own = twin.forward_backward(_twin_batches(mode, gs)[1])
    assert float(own) > 2.0 * float(twin.forward_backward(_twin_batches(mode, gs)[1], n_global=T))
    if mode == "replay":
        assert tr.slot_misses + tr.slot_hits == 3 and tr.slot_misses >= 2      # counted per micro-batch
        assert all(key[4] == T for key in tr._slots)                           # ... and keyed with the window's total


# =====================================================================================================================
# 2. it is the big batch's objective
# =====================================================================================================================
def test_fp32_window_follows_the_mean_of_the_batch_1_gradients_over_all_crystals():
    """Trainer(per_crystal_keys=True, loss="crystal_rmse") on ph_h64, window 2 + 1 + 1: the flat gradient against the mean over all
    T crystals of the float64 oracle's batch-1 gradients, by PC._assert_grads; the loss and crystal_losses within (1 + beta) 1e-4
    (test_crystal_rmse_with_per_crystal_keys_is_the_mean_of_the_batch_1_gradients_fp32's reference and bars)."""
    from oracle import dos_oracle as O
    from dostransformer_amd.train import Trainer
    name = "ph_h64"
    c = PC.MODELS[name]
    cs = PC._crystals(name)
    sizes = (2, 1, 1)
    model, p = PC._model(name)
    leaves = PC._leaves(p)
    names = list(leaves)
    losses = []
    for cr in cs:
        g1 = PC._collate([cr]).to("cpu", dtype=torch.float64)
        dg, _, ds = PC._oracle_fwd("phonon", leaves, g1, c["L"], c["T"])
        losses.append(O.loss_phonon(dg, ds, g1.phdos, PC.BETA))
    each = torch.stack(losses)
    ref = each.mean()
    params = [leaves[k] for k in names]
    grads = dict(zip(names, torch.autograd.grad(ref, params, allow_unused=True, retain_graph=True)))
    # input condition: the mean of the per-batch means is another objective, by more than the comparison's bar
    naive = torch.stack([each[0:2].mean(), each[2:3].mean(), each[3:4].mean()]).mean()
    ngr = dict(zip(names, torch.autograd.grad(naive, params, allow_unused=True)))
    diff = max(float((ngr[k] - r).abs().max() / (r.abs().max() + 1e-6)) for k, r in grads.items() if r is not None)
    print(f"{name}: mean of the per-batch means against the mean over crystals: largest per-tensor gradient difference {diff:.3g} "
          f"(bar of the comparison {PC.F64_MAX:g})")
    assert diff > PC.F64_MAX, diff
    gs, o = [], 0
    for s in sizes:
        gs.append(PC._collate(cs[o:o + s]).to(DEV))
        o += s
    tr = Trainer(model, beta=PC.BETA, per_crystal_keys=True, loss="crystal_rmse")
    loss = tr.step_accumulate(gs)
    print(f"{name}: window loss {float(loss):.8f}, mean of the batch-1 oracle losses {float(ref.detach()):.8f}")
    assert abs(float(loss) - float(ref.detach())) < (1 + PC.BETA) * 1e-4
    assert tr.crystal_losses.shape == (len(cs),)
    assert float((tr.crystal_losses.cpu().double() - each.detach()).abs().max()) < (1 + PC.BETA) * 1e-4
    G = model.flat_params().G
    PC._assert_grads(name + " window", G, grads)
    # ONE step on the concatenated batch: within the bar of the same reference, so the pair agrees within twice the bar
    model1, _ = PC._model(name)
    one = Trainer(model1, beta=PC.BETA, per_crystal_keys=True, loss="crystal_rmse")
    loss1 = one.step(PC._collate(cs).to(DEV))
    G1 = model1.flat_params().G
    PC._assert_grads(name + " one step", G1, grads)
    worst = max(float((G[k].detach().cpu().double() - G1[k].detach().cpu().double()).abs().max() / (r.abs().max() + 1e-6))
                for k, r in grads.items() if r is not None)
    print(f"{name}: window against one step on the concatenated batch: worst per-tensor gradient difference {worst:.3g}")
    assert worst < 2 * PC.F64_MAX and abs(float(loss) - float(loss1)) < 2 * (1 + PC.BETA) * 1e-4


def test_float64_window_follows_the_mean_of_the_batch_1_gradients_over_all_crystals(monkeypatch):
    """Trainer64, set_per_crystal_keys(True), fp64 softmax on both sides: loss 1e-12 relative, every tensor of the flat gradient
    within 1e-10 of its largest entry (test_crystal_rmse_..._f64's reference and bars)."""
    from oracle import dos_oracle as O
    from dostransformer_amd import functional64 as F64
    from dostransformer_amd.train64 import Trainer64
    monkeypatch.setattr(O, "multihead_attention", T64._soft64_mha)
    monkeypatch.setattr(F64, "SOFTMAX64", True)
    base = T64._module()
    beta = 0.7
    cs = T64._crystals(T64.ATOMS_A, 51)
    sizes = (2, 1, 1)
    pr = {k: (v.detach().clone().requires_grad_(True) if v.is_floating_point() else v.clone()) for k, v in base.state_dict().items()}
    leaves = [v for v in pr.values() if v.is_floating_point() and v.requires_grad]
    losses = []
    for cr in cs:
        g1 = T64._collate([cr])
        out = O.dostransformer_phonon_forward(pr, g1, T64.L_, T64.T_)
        losses.append(O.loss_phonon(out[0], out[2], g1.phdos, beta))
    each = torch.stack(losses)
    ref = each.mean()
    naive = torch.stack([each[0:2].mean(), each[2:3].mean(), each[3:4].mean()]).mean()
    ngr = torch.autograd.grad(naive, leaves, allow_unused=True, retain_graph=True)
    ref.backward()
    diff = max(float((a - v.grad).abs().max() / (v.grad.abs().max() + 1e-300)) for a, v in zip(ngr, leaves)
               if a is not None and v.grad is not None)
    print(f"t64: mean of the per-batch means against the mean over crystals: largest per-tensor gradient difference {diff:.3g}")
    assert diff > 1e-10, diff
    gs, o = [], 0
    for s in sizes:
        gs.append(T64._collate(cs[o:o + s]).to(DEV))
        o += s
    tr = Trainer64(T64._switch(copy.deepcopy(base), True), lr=1e-3, beta=beta, loss="crystal_rmse")
    loss = tr.step_accumulate(gs)
    e = abs(float(loss) - float(ref.detach())) / abs(float(ref.detach()))
    assert e <= 1e-12, e
    assert tr.crystal_losses.shape == (len(cs),)
    assert float(((tr.crystal_losses.cpu() - each.detach()).abs() / each.detach()).max()) <= 1e-12
    one = Trainer64(T64._switch(copy.deepcopy(base), True), lr=1e-3, beta=beta, loss="crystal_rmse")
    one.step(T64._collate(cs).to(DEV))
    worst = pair = 0.0
    for k, got in tr._fp.G.items():
        r = pr[k].grad
        w = float((got.detach().cpu() - r).abs().max() / (r.abs().max() + 1e-300))
        w1 = float((one._fp.G[k].detach().cpu() - r).abs().max() / (r.abs().max() + 1e-300))
        pair = max(pair, float((got.detach() - one._fp.G[k].detach()).abs().max().cpu() / (r.abs().max() + 1e-300)))
        worst = max(worst, w)
        assert w <= 1e-10 and w1 <= 1e-10, (k, w, w1)
    print(f"t64 window: loss error {e:.2e}, worst per-tensor gradient error {worst:.2e}, against one step {pair:.2e}")
    assert pair <= 2e-10


# =====================================================================================================================
# 3. K = 1 is step
# =====================================================================================================================
@pytest.mark.parametrize("name,mode", CASES, ids=[f"{c}-{m}" for c, m in CASES])
def test_a_window_of_one_is_step_bit_for_bit(name, mode):
    c = _fam(name)
    for kw in ({}, {"loss": "mse"}):
        a, _ = c.trainer(mode, **kw)
        b, _ = c.trainer(mode, **kw)
        for step in range(3):
            assert torch.equal(a.step(c.g), b.step_accumulate([c.g])), (kw, step)
            assert _seed(a) == _seed(b)
        assert _same(_state(a), _state(b)) and a.step_count == b.step_count == 3
        assert b._acc is None                                            # no accumulate launch, no accumulator
        assert (a.slot_misses, a.slot_hits) == (b.slot_misses, b.slot_hits)
        if kw:
            assert torch.equal(a.crystal_losses, b.crystal_losses)


def test_a_dataset_window_of_one_is_step_dataset_bit_for_bit():
    from tests.test_gpu_weight_ema import _dataset
    c, ds = _fam("phonon"), _dataset()
    a, _ = c.trainer("replay")
    b, _ = c.trainer("replay")
    for sel in ([0, 1, 2, 3], [4, 5, 6, 7], [0, 1, 2, 3]):
        assert torch.equal(a.step_dataset(ds, np.array(sel)), b.step_dataset_accumulate(ds, [np.array(sel)]))
    assert _same(_state(a), _state(b)) and b._acc is None


# =====================================================================================================================
# 4. replay is eager, bitwise
# =====================================================================================================================
@pytest.mark.parametrize("name,kw,mode", [(f, {"loss": "mse"}, "replay") for f in FAMILIES] + [("edos", {}, "replay"),
                                                                                             ("phonon", {"loss": "mse"}, "graph")],
                         ids=[f + "-mse-replay" for f in FAMILIES] + ["edos-default-replay", "phonon-mse-graph"])
def test_replayed_windows_are_bitwise_the_eager_ones(name, kw, mode):
    """Three windows [ga, gb, ga]: the first and the last micro-batch share a slot, which is replayed twice inside a window
    (``graph``: the slot's captured HIP graphs)."""
    c = _fam(name)
    ga, gb = _cut(name)[0], _cut(name)[1]
    T = 2 * SIZES[name][0] + SIZES[name][1]
    eager, _ = c.trainer("eager", **kw)
    replay, _ = c.trainer(mode, **kw)
    pad = (lambda g: g) if c.f64 else _padded
    for w in range(3):
        le = eager.step_accumulate([pad(ga), pad(gb), pad(ga)])
        lr = replay.step_accumulate([ga, gb, ga])
        assert torch.equal(le, lr), w
        if kw:
            assert eager.crystal_losses.shape == (T,) and torch.equal(eager.crystal_losses, replay.crystal_losses), w
            k = SIZES[name][0]                                           # the same crystals first and last: the same losses
            assert torch.equal(replay.crystal_losses[:k], replay.crystal_losses[T - k:])
    assert _same(_state(eager), _state(replay))
    assert eager.step_count == replay.step_count == 3
    assert (replay.slot_misses, replay.slot_hits) == (2, 7) and (eager.slot_misses, eager.slot_hits) == (0, 0)
    for key in replay._slots:
        assert key[4 if not c.f64 else -1] == T, key                     # the window's total is part of the slot key


def test_fp32_dataset_windows_are_bitwise_the_batch_object_ones():
    from dostransformer_amd import synth
    from dostransformer_amd.batch import collate
    from dostransformer_amd.loader import DeviceDataset
    c = _fam("phonon")
    cs = synth.phonon_crystals(8, seed=91, dtype=torch.float32)
    ds = DeviceDataset(cs, DEV)
    nmax = max(int(cr["x"].shape[0]) for cr in cs)
    a, _ = c.trainer("replay", loss="crystal_rmse")
    b, _ = c.trainer("replay", loss="crystal_rmse")
    sels = [[0, 1, 2], [3, 4], [5, 6, 7]]
    for w in range(3):
        la = a.step_dataset_accumulate(ds, [np.array(s) for s in sels], n_max=nmax)
        lb = b.step_accumulate([collate([cs[j] for j in s], n_max=nmax).to(DEV) for s in sels])
        assert torch.equal(la, lb), w
        assert a.crystal_losses.shape == (8,) and torch.equal(a.crystal_losses, b.crystal_losses)
    assert _same(_state(a), _state(b)) and a.step_count == 3
    assert (a.slot_misses + a.slot_hits, b.slot_misses + b.slot_hits) == (9, 9) and a.slot_hits >= 6
    # the eager trainer's dataset form is the batch-object form on ds.collate
    e1, _ = c.trainer("eager", loss="crystal_rmse")
    e2, _ = c.trainer("eager", loss="crystal_rmse")
    assert torch.equal(e1.step_dataset_accumulate(ds, sels), e2.step_accumulate([ds.collate(s) for s in sels]))
    assert _same(_state(e1), _state(e2))


def test_float64_dataset_windows_are_bitwise_the_batch_object_ones():
    from dostransformer_amd.loader import DeviceDataset
    from dostransformer_amd.train64 import Trainer64
    cs = T64._crystals(T64.ATOMS_A + T64.ATOMS_B, 77)
    ds = DeviceDataset(cs, DEV, dtype=torch.float64)
    base = T64._module()
    mk = lambda: Trainer64(T64._switch(copy.deepcopy(base), True), lr=1e-3, replay=True, bucket=(16, 128), loss="mae")
    a, b = mk(), mk()
    sels = [[0, 1, 2], [3, 4], [5, 6]]
    for w in range(2):
        la = a.step_dataset_accumulate(ds, sels, n_max=19)
        lb = b.step_accumulate([ds.collate(s, n_max=19) for s in sels])
        assert torch.equal(la, lb), w
        assert a.crystal_losses.shape == (7,) and torch.equal(a.crystal_losses, b.crystal_losses)
    assert _same(_state(a), _state(b)) and a.step_count == 2
    assert all(key[-1] == 7 for key in a._slots)


# =====================================================================================================================
# 5. the guard judges the window
# =====================================================================================================================
@pytest.mark.parametrize("mode", ["eager", "replay"])
def test_clipped_window_is_the_composition_with_the_coefficient_applied(mode):
    c, gs = _fam("edos"), _cut("edos")
    T = sum(SIZES["edos"])
    probe, _ = c.trainer(mode, skip_nonfinite=True)
    probe.step_accumulate(gs)
    mx = 0.05 * probe.guard_report().norm
    assert mx > 0
    tr, _ = c.trainer(mode, max_grad_norm=mx)
    twin, _ = c.trainer("eager", max_grad_norm=mx)
    for w in range(2):
        loss = tr.step_accumulate(gs)
        G, L, n = _compose(twin, _twin_batches(mode, gs), T)
        twin.optimizer_step()
        assert torch.equal(loss, L) and torch.equal(tr._fp.grad[:n], G[:n]), w
        total = float(G[:n].double().pow(2).sum().sqrt())
        r = tr.guard_report()
        print(f"edos-{mode} window {w + 1}: norm {r.norm:.8g} against the float64 norm of the summed gradient {total:.8g}, "
              f"coefficient {r.clip:.4f}")
        assert abs(float(tr.grad_norm) - total) <= 1e-6 * total and float(tr.grad_norm) == r.norm
        assert r.clip < 1.0 and not r.skipped_last and r.applied == w + 1
        assert _same(_state(tr), _state(twin)), w
    assert tr.step_count == 2


@pytest.mark.parametrize("name,mode", [(f, m) for f in ("phonon", "t64", "gn64") for m in ("eager", "replay")])
def test_nan_in_the_second_micro_batch_skips_the_whole_window(name, mode):
    from dostransformer_amd._lib import DosxError
    c, gs = _fam(name), _cut(name)
    kw = dict(skip_nonfinite=True, loss="mse", ema_decay=0.9)
    tr, _ = c.trainer(mode, **kw)
    clean, _ = c.trainer(mode, **kw)
    bad = gs[1].clone()
    t = gs[1].phdos.clone()
    t.view(-1)[7] = float("nan")
    bad.phdos = t
    assert torch.equal(tr.step_accumulate(gs), clean.step_accumulate(gs))
    before = _state(tr) + (tr._ema.clone(),)
    loss = tr.step_accumulate([gs[0], bad, gs[2]])
    assert not bool(torch.isfinite(loss))
    assert _same(before, _state(tr) + (tr._ema.clone(),))
    r = tr.guard_report()
    assert r.skipped_last and "non-finite gradient" in r.reasons and (r.applied, r.skipped, r.first_skip_step) == (1, 1, 2)
    assert r.first_bad[0] in tr._fp.names and r.n_bad > 0
    k = SIZES[name][0]
    assert (~torch.isfinite(tr.crystal_losses)).tolist() == [False] * k + [True] + [False] * (sum(SIZES[name]) - k - 1)
    assert tr.step_count == 2 and tr.state_dict()["step"] == 1
    with pytest.raises(DosxError, match=r"step 2: gradient of .*\[\d+\] is not finite; 1 step skipped"):
        tr.check()
    assert tr.step_count == 1
    # neither AdamW's time nor the average's warm-up advanced: the next clean window is the window of a trainer that never saw it
    assert torch.equal(tr.step_accumulate(gs), clean.step_accumulate(gs))
    assert _same(_state(tr) + (tr._ema,), _state(clean) + (clean._ema,))
    assert tr.step_count == clean.step_count == 2 and tr.guard_report().applied == 1          # (counted since the check)


# =====================================================================================================================
# 6. composition
# =====================================================================================================================
@pytest.mark.parametrize("mode", ["eager", "replay"])
def test_frozen_trunk_no_decay_group_average_and_clipping_in_one_window(mode):
    from dostransformer_amd import param_groups as pg
    from tests.test_gpu_finetune import TRUNK
    c, gs = _fam("edos"), _cut("edos")
    T = sum(SIZES["edos"])

    def mk(md, **more):
        m = c.model().freeze(*TRUNK)
        return c._tr(m, **({"replay": True} if md == "replay" else {}), ema_decay=0.9,
                     param_groups=[{"params": pg.no_decay(m), "weight_decay": 0.0}], **more)

    probe = mk(mode, skip_nonfinite=True)
    probe.step_accumulate(gs)
    mx = 0.05 * probe.guard_report().norm
    tr, twin = mk(mode, max_grad_norm=mx), mk("eager", max_grad_norm=mx)
    for w in range(2):
        ema_before = None if tr._ema is None else tr._ema.clone()
        loss = tr.step_accumulate(gs)
        G, L, n = _compose(twin, _twin_batches(mode, gs), T)
        twin.optimizer_step()
        assert 0 < n < tr._fp.total and n == tr._fp.n_train
        assert torch.equal(loss, L) and torch.equal(tr._fp.grad[:n], G[:n]), w
        assert _same(_state(tr) + (tr._ema,), _state(twin) + (twin._ema,)), w
        assert tr.guard_report().clip < 1.0
        if ema_before is not None:
            assert not torch.equal(ema_before[:n], tr._ema[:n]) and torch.equal(ema_before[n:], tr._ema[n:])
    assert tr.step_count == 2 and tr.guard_report().applied == 2          # the average moved once per window: the twin's two launches
    assert "window" not in "".join(tr.state_dict()) and set(tr.state_dict()) == set(twin.state_dict())


def test_dropout_draws_a_fresh_mask_for_every_micro_batch():
    from dostransformer_amd.embedder_eDOS.DOSTransformer import DOSTransformer
    from dostransformer_amd.train import Trainer
    gs = _cut("edos")
    torch.manual_seed(3)
    model = DOSTransformer(2, 2, 200, 41, 2, 32, DEV, 0.3).to(DEV).train()
    tr = Trainer(model, lr=1e-4)
    tr.step_accumulate(gs)
    s1 = _seed(tr)
    tr.step_accumulate(gs[:2])
    s2 = _seed(tr)
    tr.step_accumulate(gs)
    assert s1 is not None and (s2 - s1, _seed(tr) - s2) == (2, 3)
    # two micro-batches of the SAME crystals: the accumulator holds G1, the gradient G1 + G2 - with one mask for both that
    # would be 2 G1 exactly
    tr.step_accumulate([gs[0], gs[0]])
    n = tr._fp.n_train
    assert not torch.equal(tr._fp.grad[:n], 2.0 * tr._acc[:n])
    model.eval()                                                         # no dropout: the same window IS 2 G1, and the seed stands
    s3 = _seed(tr)
    tr.step_accumulate([gs[0], gs[0]])
    assert torch.equal(tr._fp.grad[:n], 2.0 * tr._acc[:n]) and _seed(tr) == s3


# =====================================================================================================================
# 7. refusals on the device
# =====================================================================================================================
def test_refusals_leave_everything_where_it_was():
    from dostransformer_amd._lib import DosxError
    from tests.test_gpu_weight_ema import _dataset
    c, gs = _fam("phonon"), _cut("phonon")
    for mode in ("eager", "replay"):
        tr, _ = c.trainer(mode)                                          # the reference's pooled RMSE
        tr.step(c.g)
        before, seed = _state(tr), _seed(tr)
        with pytest.raises(DosxError, match='loss="crystal_rmse"'):
            tr.step_accumulate(gs)
        with pytest.raises(DosxError, match='loss="crystal_rmse"'):
            tr.step_dataset_accumulate(_dataset(), [[0, 1], [2]])
        assert _same(before, _state(tr)) and tr.step_count == 1 and _seed(tr) == seed and tr._acc is None
    t64, g64 = _fam("t64"), _cut("t64")
    tr, _ = t64.trainer("eager")
    with pytest.raises(DosxError, match='loss="crystal_rmse"'):
        tr.step_accumulate(g64)
    from dostransformer_amd.batch import bucket_sizes, pad_batch
    tr, _ = t64.trainer("eager", loss="mse")
    ghost = pad_batch(g64[1], *bucket_sizes(g64[1].meta.num_nodes, g64[1].meta.num_edges, 16, 128))
    with pytest.raises(DosxError, match="ghost-padded"):
        tr.step_accumulate([g64[0], ghost])
    assert tr.step_count == 0 and tr._fp is None and tr._acc is None
    # inside ema_weights()
    tr, _ = c.trainer("eager", loss="mse", ema_decay=0.9)
    tr.step_accumulate(gs)
    before = _state(tr)
    with tr.ema_weights():
        with pytest.raises(DosxError, match="ema_weights"):
            tr.step_accumulate(gs)
        with pytest.raises(DosxError, match="ema_weights"):
            tr.step_dataset_accumulate(_dataset(), [[0, 1], [2]])
    assert _same(before, _state(tr)) and tr.step_count == 1
    # the public refusal of a foreign count stands
    with pytest.raises(ValueError, match="n_global"):
        tr.step(gs[0], n_global=4)
    with pytest.raises(ValueError, match="n_global"):
        tr.forward_backward(gs[0], n_global=4)
    with pytest.raises(ValueError, match="empty window"):
        tr.step_accumulate([])


@pytest.mark.parametrize("mode", ["eager", "replay"])
def test_an_exception_in_the_second_micro_batch_moves_nothing(mode):
    """A batch of the other node width on a baseline: refused by the trainer in front of that micro-batch's program, after the
    first one has run and its gradient has been copied into the accumulator."""
    from dostransformer_amd._lib import DosxError
    c, gs = _fam("gnp"), _cut("gnp")
    kw = dict(loss="mse", ema_decay=0.9)
    tr, _ = c.trainer(mode, **kw)
    clean, _ = c.trainer(mode, **kw)
    assert torch.equal(tr.step_accumulate(gs), clean.step_accumulate(gs))
    wide = gs[1].clone()
    wide.x = torch.zeros(gs[1].x.shape[0], gs[1].x.shape[1] + 1, dtype=gs[1].x.dtype, device=DEV)
    before = _state(tr) + (tr._ema.clone(),)
    with pytest.raises(DosxError, match="node encoder"):
        tr.step_accumulate([gs[0], wide, gs[2]])
    assert _same(before, _state(tr) + (tr._ema,)) and tr.step_count == 1 and tr._window_total is None
    with pytest.raises(ValueError, match="n_global"):                    # ... and the internal route is closed again
        tr.step(gs[0], n_global=5)
    for w in range(2):
        assert torch.equal(tr.step_accumulate(gs), clean.step_accumulate(gs)), w
    assert _same(_state(tr) + (tr._ema,), _state(clean) + (clean._ema,)) and tr.step_count == 3
