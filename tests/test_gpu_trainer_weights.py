"""``sample_weights=True`` / ``bin_weights=...`` of the fused trainers on a real MI355X (dosx_loss_rows_w): the
models, batches and bars are those of tests/test_gpu_trainer_loss.py and tests/test_gpu_trainer_accumulate.py (L2 T2 H32, 4 - 5
synthetic crystals; ``ph_h64`` of tests/test_gpu_train_per_crystal.py and ``T64.ATOMS_A`` against the float64 oracle).

What is bitwise here is bitwise by construction: all-ones weights multiply by 1.0, a replayed step issues the eager step's
launches on the same buffers, ``step_dataset`` gathers out of the dataset's table what ``ds.collate`` puts on the batch, and a
crystal of weight 0 contributes exact zeros whatever its target holds."""
import copy

import numpy as np
import pytest
import torch

from tests import test_gpu_train64 as T64
from tests import test_gpu_train_per_crystal as PC
from tests.gpu_util import DEV
from tests.test_gpu_trainer_accumulate import _padded
from tests.test_gpu_trainer_guard import _same, _state
from tests.test_gpu_trainer_loss import CASES, FAMILIES, _fam

pytestmark = pytest.mark.gpu

WEIGHTS = [2.0, 0.5, 0.0, 1.0]                     # a doubled, a halved, a dropped and a plain crystal


def _weighted(g, w):
    """a copy of batch g that carries the [B] field `weight` (in the batch's own floating-point dtype)"""
    out = g.clone()
    out.weight = torch.as_tensor(w, dtype=torch.float64).to(g.x.dtype).to(g.x.device)
    assert out.weight.shape == (g.num_graphs,)
    return out


def _random_weights(B, S, seed):
    gen = torch.Generator().manual_seed(seed)
    w = 0.25 * 16.0 ** torch.rand(B, generator=gen, dtype=torch.float64)
    v = 2.0 * torch.rand(S, generator=gen, dtype=torch.float64)
    v[[0, S // 3]] = 0.0
    return w, v


def _S(c):
    return int(c.model()._cfg.S)


# =====================================================================================================================
# 1. the weighted objective: (1 / B) sum_b w_b g_b of the oracle's batch-1 gradients
# =====================================================================================================================
def test_weighted_step_is_the_weighted_mean_of_the_batch_1_gradients_f64(monkeypatch):
    """Trainer64, set_per_crystal_keys(True), fp64 softmax on both sides, loss="crystal_rmse", the four T64.ATOMS_A crystals with
    weights [2, 0.5, 0, 1]: loss within 1e-12 relative, every tensor of the flat gradient within 1e-10 of its largest entry."""
    from oracle import dos_oracle as O
    from dostransformer_amd import functional64 as F64
    from dostransformer_amd.train64 import Trainer64
    monkeypatch.setattr(O, "multihead_attention", T64._soft64_mha)
    monkeypatch.setattr(F64, "SOFTMAX64", True)
    base = T64._module()
    beta = 0.7
    cs = T64._crystals(T64.ATOMS_A, 51)
    w = torch.tensor(WEIGHTS, dtype=torch.float64)
    pr = {k: (v.detach().clone().requires_grad_(True) if v.is_floating_point() else v.clone()) for k, v in base.state_dict().items()}
    losses = []
    for cr in cs:
        g1 = T64._collate([cr])
        out = O.dostransformer_phonon_forward(pr, g1, T64.L_, T64.T_)
        losses.append(O.loss_phonon(out[0], out[2], g1.phdos, beta))
    each = torch.stack(losses)
    ref = (w * each).sum() / len(cs)
    plain = each.mean().detach()
    ref.backward()
    assert abs(float(ref.detach()) - float(plain)) > 1e-3 * float(plain)             # input condition: the weights matter
    tr = Trainer64(T64._switch(copy.deepcopy(base), True), lr=1e-3, beta=beta, loss="crystal_rmse", sample_weights=True)
    loss = tr.forward_backward(_weighted(T64._collate(cs).to(DEV), WEIGHTS))
    e = abs(float(loss) - float(ref.detach())) / abs(float(ref.detach()))
    assert e <= 1e-12, e
    assert float(((tr.crystal_losses.cpu() - each.detach()).abs() / each.detach()).max()) <= 1e-12      # unweighted, all four
    worst = 0.0
    for k, got in tr._fp.G.items():
        r = pr[k].grad
        d = float((got.detach().cpu() - r).abs().max() / (r.abs().max() + 1e-300))
        worst = max(worst, d)
        assert d <= 1e-10, (k, d)
    print(f"t64 weighted crystal_rmse: loss error {e:.2e}, worst per-tensor gradient error {worst:.2e}")


def test_weighted_step_is_the_weighted_mean_of_the_batch_1_gradients_fp32():
    """Trainer(per_crystal_keys=True, loss="crystal_rmse", sample_weights=True) on ph_h64 with weights [2, 0.5, 0, 1], by the
    element-error rule of tests/test_gpu_train_per_crystal.py; loss and crystal_losses within (1 + beta) 1e-4 (the bars of
    test_crystal_rmse_with_per_crystal_keys_is_the_mean_of_the_batch_1_gradients_fp32)."""
    from oracle import dos_oracle as O
    from dostransformer_amd.train import Trainer
    name = "ph_h64"
    c = PC.MODELS[name]
    cs = PC._crystals(name)
    w = torch.tensor(WEIGHTS, dtype=torch.float64)
    model, p = PC._model(name)
    leaves = PC._leaves(p)
    names = list(leaves)
    losses = []
    for cr in cs:
        g1 = PC._collate([cr]).to("cpu", dtype=torch.float64)
        dg, _, ds = PC._oracle_fwd("phonon", leaves, g1, c["L"], c["T"])
        losses.append(O.loss_phonon(dg, ds, g1.phdos, PC.BETA))
    each = torch.stack(losses)
    ref = (w * each).sum() / len(cs)
    grads = dict(zip(names, torch.autograd.grad(ref, [leaves[k] for k in names], allow_unused=True, retain_graph=True)))
    unw = dict(zip(names, torch.autograd.grad(each.mean(), [leaves[k] for k in names], allow_unused=True)))
    diff = max(float((unw[k] - r).abs().max() / (r.abs().max() + 1e-300)) for k, r in grads.items() if r is not None)
    print(f"{name}: unweighted against weighted mean of the batch-1 gradients: largest per-tensor difference {diff:.3f}")
    assert diff >= 0.05, diff                                   # input condition: far above the comparison's bar
    tr = Trainer(model, beta=PC.BETA, per_crystal_keys=True, loss="crystal_rmse", sample_weights=True)
    loss = tr.forward_backward(_weighted(PC._collate(cs).to(DEV), WEIGHTS))
    print(f"{name}: weighted loss {float(loss):.8f}, of the batch-1 oracle losses {float(ref.detach()):.8f}")
    assert abs(float(loss) - float(ref.detach())) < (1 + PC.BETA) * 1e-4
    assert float((tr.crystal_losses.cpu().double() - each.detach()).abs().max()) < (1 + PC.BETA) * 1e-4
    PC._assert_grads(name + " weighted crystal_rmse", model.flat_params().G, grads)


# =====================================================================================================================
# 2. bitwise
# =====================================================================================================================
@pytest.mark.parametrize("name,mode", CASES, ids=[f"{c}-{m}" for c, m in CASES])
def test_all_ones_trains_the_bits_of_the_trainer_without_the_flag(name, mode):
    c = _fam(name)
    g1 = _weighted(c.g, [1.0] * c.B)
    for kind in ("crystal_rmse", "mae"):
        plain, _ = c.trainer(mode, loss=kind)
        tr, _ = c.trainer(mode, loss=kind, sample_weights=True)
        for step in range(3):
            assert torch.equal(plain.step(c.g), tr.step(g1)), (kind, step)
            assert torch.equal(plain.crystal_losses, tr.crystal_losses), (kind, step)
        assert _same(_state(plain), _state(tr)), kind
        wname = "dosx_loss_rows_w_f64" if c.f64 else "dosx_loss_rows_w"
        pname = "dosx_loss_rows_f64" if c.f64 else "dosx_loss_rows"
        if not c.f64:                                           # (train.Trainer keeps program_stats)
            assert wname in tr.program_stats()["entries"] and pname not in tr.program_stats()["entries"]
            assert pname in plain.program_stats()["entries"] and wname not in plain.program_stats()["entries"]
            assert tr.program_stats()["launches"] == plain.program_stats()["launches"]
        if mode != "eager":
            assert (tr.slot_misses, tr.slot_hits) == (1, 2)


@pytest.mark.parametrize("name", FAMILIES)
def test_replay_is_bitwise_eager_with_weights_and_bin_weights(name):
    from dostransformer_amd.batch import bucket_sizes, pad_batch
    c = _fam(name)
    w, v = _random_weights(c.B, _S(c), 11)
    kinds = ("crystal_rmse", "huber")
    for kind in kinds:
        kw = {"loss": kind, "sample_weights": True, "bin_weights": v, **({"huber_delta": c.first_delta()} if kind == "huber" else {})}
        eager, _ = c.trainer("eager", **kw)
        replay, _ = c.trainer("replay", **kw)
        ga, gb = _weighted(c.g, w), _weighted(c.g, w.flip(0))
        pad = (lambda g: g) if c.f64 else (lambda g: pad_batch(g, *bucket_sizes(g.meta.num_nodes, g.meta.num_edges, *replay.bucket)))
        for step, g in enumerate((ga, gb, ga)):                 # the second batch's weights reach the slot's static buffer
            assert torch.equal(eager.step(pad(g)), replay.step(g)), (kind, step)
            assert torch.equal(eager.crystal_losses, replay.crystal_losses), (kind, step)
        assert _same(_state(eager), _state(replay)), kind
        assert (replay.slot_misses, replay.slot_hits) == (1, 2)
    # the weights are read: other weights, another loss
    a, _ = c.trainer("eager", loss="mse", sample_weights=True)
    assert not torch.equal(a.forward_backward(_weighted(c.g, w)), a.forward_backward(_weighted(c.g, w.flip(0))))


def _dataset32(weights=None):
    from dostransformer_amd import synth
    from dostransformer_amd.loader import DeviceDataset
    cs = synth.phonon_crystals(8, 91, torch.float32)
    if weights is not None:
        for cr, x in zip(cs, weights):
            cr["weight"] = float(x)
    return DeviceDataset(cs, DEV)


def test_step_dataset_gathers_out_of_the_table_fp32():
    """step_dataset with the dataset's table is bitwise step(ds.collate(idx)); a second set_weights is read by the next REPLAYED
    step (no new recording) and is bitwise the eager step with the new values; a second dataset records slots of its own."""
    c = _fam("phonon")
    w0, _ = _random_weights(8, 51, 21)
    w1, _ = _random_weights(8, 51, 22)
    w0[5], w1[1] = 0.0, 0.0
    ds = _dataset32(w0)
    assert torch.equal(ds.weights.cpu().double(), w0.float().double())
    kw = dict(loss="crystal_rmse", sample_weights=True)
    a, _ = c.trainer("replay", **kw)
    b, _ = c.trainer("replay", **kw)
    e, _ = c.trainer("eager", **kw)
    sels = [np.array([0, 1, 2, 3]), np.array([4, 5, 6, 7]), np.array([0, 1, 2, 3])]
    for k, sel in enumerate(sels):
        g = ds.collate(sel)
        assert torch.equal(g.weight, ds.weights[torch.from_numpy(sel).to(DEV)]) and g.weight.dtype == torch.float32
        la = a.step_dataset(ds, sel)
        assert torch.equal(la, b.step(g)) and torch.equal(la, e.step(_padded(g))), k
        assert torch.equal(a.crystal_losses, e.crystal_losses), k
    assert _same(_state(a), _state(b)) and _same(_state(a), _state(e))
    misses = a.slot_misses
    assert (misses, a.slot_hits) == (2, 1)
    assert all(key[-1] == ds._f32_tables()["weight"].data_ptr() for key in a._slots)          # the table is the key's last field
    ptr = ds.weights.data_ptr()
    ds.set_weights(w1)                                           # in place: the recorded launches read the new values
    assert ds.weights.data_ptr() == ptr
    for k, sel in enumerate(sels[:2]):
        la = a.step_dataset(ds, sel)
        assert torch.equal(la, e.step(_padded(ds.collate(sel)))), k
    assert _same(_state(a), _state(e)) and a.slot_misses == misses and a.slot_hits == 3
    # the old values would have given another step
    probe, _ = c.trainer("eager", **kw)
    old, new = _weighted(ds.collate(sels[0]), w0[:4]), ds.collate(sels[0])
    assert not torch.equal(probe.forward_backward(_padded(old)), probe.forward_backward(_padded(new)))
    # a second dataset: its own table, its own slots - never a replay on the first one's pointer
    ds2 = _dataset32(w0)
    la = a.step_dataset(ds2, sels[0])
    assert torch.equal(la, e.step(_padded(ds2.collate(sels[0]))))
    assert a.slot_misses == misses + 1 and _same(_state(a), _state(e))
    # a dataset without weights is refused before anything moves
    before = _state(a)
    with pytest.raises(ValueError, match="set_weights"):
        a.step_dataset(_dataset32(), sels[0])
    with pytest.raises(ValueError, match="weight"):
        a.step(c.g)
    with pytest.raises(ValueError, match="weight"):
        e.step(c.g)
    assert _same(before, _state(a))


def test_step_dataset_gathers_out_of_the_table_f64():
    from dostransformer_amd.loader import DeviceDataset
    from dostransformer_amd.train64 import Trainer64
    cs = T64._crystals(T64.ATOMS_A + T64.ATOMS_B, 77)
    w0, _ = _random_weights(7, 51, 23)
    w1, _ = _random_weights(7, 51, 24)
    w0[2] = 0.0
    for cr, x in zip(cs, w0):
        cr["weight"] = x
    ds = DeviceDataset(cs, DEV, dtype=torch.float64)
    assert torch.equal(ds.weights.cpu(), w0) and ds._f64_tables()["weight"] is ds.weights
    base = T64._module()
    mk = lambda: Trainer64(T64._switch(copy.deepcopy(base), True), lr=1e-3, replay=True, bucket=(16, 128), loss="mae",
                           sample_weights=True)
    a, b = mk(), mk()
    sels = [[0, 1, 2], [3, 4, 5, 6], [0, 1, 2]]
    for sel in sels:
        assert torch.equal(a.step_dataset(ds, sel, n_max=19), b.step(ds.collate(sel, n_max=19))), sel
    misses = a.slot_misses
    ds.set_weights(w1)
    for sel in sels[:2]:
        assert torch.equal(a.step_dataset(ds, sel, n_max=19), b.step(ds.collate(sel, n_max=19))), sel
        assert torch.equal(a.crystal_losses, b.crystal_losses)
    assert _same(_state(a), _state(b)) and a.slot_misses == misses == 2 and a.step_count == 5
    assert all(key[-1] == ds.weights.data_ptr() for key in a._slots)


# =====================================================================================================================
# 3. weight 0 through the guard
# =====================================================================================================================
@pytest.mark.parametrize("name,mode", [(f, m) for f in ("phonon", "t64", "gn64") for m in ("eager", "replay")])
def test_a_poisoned_target_under_weight_zero_is_a_step_like_any_other(name, mode):
    """Cfg.poisoned() plants a NaN in crystal 0's target.  skip_nonfinite=True with w_0 = 0: the step is taken, the report is
    clean, parameters and moments are bitwise those of the same step on the clean target at w_0 = 0; with w_0 = 1 it is skipped."""
    c = _fam(name)
    w = [0.0] + [1.5, 0.75, 1.0, 2.0][:c.B - 1]
    kw = dict(skip_nonfinite=True, loss="mse", sample_weights=True)
    tr, _ = c.trainer(mode, **kw)
    clean, _ = c.trainer(mode, **kw)
    bad = c.poisoned()
    for step in range(2):                                        # (replay: recorded on the poisoned batch, then replayed)
        la, lb = tr.step(_weighted(bad, w)), clean.step(_weighted(c.g, w))
        assert bool(torch.isfinite(la)) and torch.equal(la, lb), step
        r = tr.guard_report()
        assert not r.skipped_last and (r.applied, r.skipped) == (step + 1, 0) and r.n_bad == 0, r
        assert (~torch.isfinite(tr.crystal_losses)).tolist() == [True] + [False] * (c.B - 1)      # the crystal's own loss says so
        assert bool(torch.isfinite(clean.crystal_losses).all())
    assert _same(_state(tr), _state(clean))
    before = _state(tr)
    loss = tr.step(_weighted(bad, [1.0] + w[1:]))
    assert not bool(torch.isfinite(loss)) and _same(before, _state(tr))
    r = tr.guard_report()
    assert r.skipped_last and (r.applied, r.skipped) == (2, 1)


# =====================================================================================================================
# 4. windows
# =====================================================================================================================
def _cut_weighted(collate, cs, sizes, w):
    gs, o = [], 0
    for s in sizes:
        gs.append(_weighted(collate(cs[o:o + s]).to(DEV), w[o:o + s]))
        o += s
    return gs


def test_ragged_weighted_window_is_the_weighted_step_f64():
    """Trainer64, window 2 + 1 + 1 with weights [2, 0.5, 0, 1] against ONE weighted step on the four crystals: the pair's bars of
    test_float64_window_follows_the_mean_of_the_batch_1_gradients_over_all_crystals (each side within 1e-12 / 1e-10 of the same
    reference: 2e-12 relative in the loss, 2e-10 of the tensor's largest entry in the gradient)."""
    from dostransformer_amd.train64 import Trainer64
    base = T64._module()
    cs = T64._crystals(T64.ATOMS_A, 51)
    mk = lambda: Trainer64(T64._switch(copy.deepcopy(base), True), lr=1e-3, beta=0.7, loss="crystal_rmse", sample_weights=True)
    tr, one, naive = mk(), mk(), mk()
    loss = tr.step_accumulate(_cut_weighted(T64._collate, cs, (2, 1, 1), WEIGHTS))
    loss1 = one.step(_weighted(T64._collate(cs).to(DEV), WEIGHTS))
    assert abs(float(loss) - float(loss1)) <= 2e-12 * abs(float(loss1))
    assert tr.crystal_losses.shape == (4,)
    assert float(((tr.crystal_losses - one.crystal_losses).abs() / one.crystal_losses).max()) <= 2e-12
    pair = 0.0
    for k, got in tr._fp.G.items():
        r = one._fp.G[k].detach()
        pair = max(pair, float((got.detach() - r).abs().max() / (r.abs().max() + 1e-300)))
    print(f"t64 weighted window against one weighted step: worst per-tensor gradient difference {pair:.2e}")
    assert pair <= 2e-10
    # input condition: the unweighted window is another step, far above the bar
    naive.step_accumulate(_cut_weighted(T64._collate, cs, (2, 1, 1), [1.0] * 4))
    far = max(float((naive._fp.G[k].detach() - one._fp.G[k].detach()).abs().max() / (one._fp.G[k].detach().abs().max() + 1e-300))
              for k in tr._fp.G)
    assert far > 1e-3, far


def test_ragged_weighted_window_is_the_weighted_step_fp32():
    """Trainer on ph_h64, the pair's bars of test_fp32_window_follows_the_mean_of_the_batch_1_gradients_over_all_crystals:
    twice PC.F64_MAX per tensor, twice (1 + beta) 1e-4 in the loss."""
    from dostransformer_amd.train import Trainer
    name = "ph_h64"
    cs = PC._crystals(name)
    model, _ = PC._model(name)
    model1, _ = PC._model(name)
    kw = dict(beta=PC.BETA, per_crystal_keys=True, loss="crystal_rmse", sample_weights=True)
    tr, one = Trainer(model, **kw), Trainer(model1, **kw)
    loss = tr.step_accumulate(_cut_weighted(PC._collate, cs, (2, 1, 1), WEIGHTS))
    loss1 = one.step(_weighted(PC._collate(cs).to(DEV), WEIGHTS))
    G, G1 = model.flat_params().G, model1.flat_params().G
    worst = max(float((G[k].detach().double() - G1[k].detach().double()).abs().max() / (G1[k].detach().double().abs().max() + 1e-6))
                for k in G1)
    print(f"{name}: weighted window against one weighted step: worst per-tensor gradient difference {worst:.3g}, losses "
          f"{float(loss):.8f} / {float(loss1):.8f}")
    assert worst < 2 * PC.F64_MAX and abs(float(loss) - float(loss1)) < 2 * (1 + PC.BETA) * 1e-4
    assert tr.crystal_losses.shape == (4,)


def test_dataset_windows_gather_too():
    c = _fam("phonon")
    w0, v = _random_weights(8, 51, 31)
    ds = _dataset32(w0)
    kw = dict(loss="mse", sample_weights=True, bin_weights=v)
    a, _ = c.trainer("replay", **kw)
    b, _ = c.trainer("replay", **kw)
    sels = [[0, 1, 2], [3, 4], [5, 6, 7]]
    nmax = int(ds.n_nodes.max())
    for w in range(2):
        la = a.step_dataset_accumulate(ds, [np.array(s) for s in sels], n_max=nmax)
        lb = b.step_accumulate([ds.collate(s, n_max=nmax) for s in sels])
        assert torch.equal(la, lb), w
        assert a.crystal_losses.shape == (8,) and torch.equal(a.crystal_losses, b.crystal_losses)
    assert _same(_state(a), _state(b)) and a.step_count == 2


# =====================================================================================================================
# 5. composition, evaluation
# =====================================================================================================================
def test_composes_with_the_average_and_a_no_decay_group():
    from dostransformer_amd import param_groups as pg
    c = _fam("phonon")
    m = c.model()
    w, v = _random_weights(c.B, 51, 41)
    tr = c._tr(m, replay=True, loss="huber", huber_delta=c.first_delta(), ema_decay=0.99, max_grad_norm=1e30, sample_weights=True,
               bin_weights=v, param_groups=[{"params": pg.no_decay(m), "weight_decay": 0.0}])
    g = _weighted(c.g, w)
    for _ in range(3):
        assert bool(torch.isfinite(tr.step(g)))
    tr.check()
    assert (tr.slot_misses, tr.slot_hits, tr.step_count) == (1, 2, 3)
    assert tr.guard_report().applied == 3 and tr.crystal_losses.shape == (c.B,)
    assert set(tr.state_dict()["hyper"]) == {"lr", "betas", "eps", "weight_decay", "beta"}          # the checkpoint it always was
    entries = tr.program_stats()["entries"]
    assert "dosx_loss_rows_w" in entries and "dosx_loss_rows" not in entries
    with tr.ema_weights():
        pass


def test_weighted_evaluation():
    """test_per_crystal(weights=...): the four figures are sum_c w_c m_c / sum_c w_c of the per-crystal table - float64 numpy on
    the table read back, 1e-12 relative; weights=None is the plain mean, bit for bit; per_crystal does not change."""
    from dostransformer_amd import evaluate
    from dostransformer_amd.predict import Predictor
    w0, _ = _random_weights(8, 51, 51)
    w0[3] = 0.0
    ds = _dataset32(w0)
    model = _fam("phonon").model().eval()
    pred = Predictor(model, per_crystal_keys=True)
    plain = evaluate.test_per_crystal(pred, ds, batch_size=3)
    again = evaluate.test_per_crystal(pred, ds, batch_size=3, weights=None)
    table = plain.per_crystal.cpu().numpy().astype(np.float64)
    assert plain[:4] == again[:4] == tuple(plain.per_crystal.mean(0).tolist()) and torch.equal(plain.per_crystal, again.per_crystal)
    w1, _ = _random_weights(8, 51, 52)
    idx = [6, 1, 3, 4, 0]
    for weights, want_w, kw in ((True, ds.weights.cpu().numpy().astype(np.float64), {}), (w1, w1.numpy(), {}),
                                (w1.tolist(), w1.numpy(), {}), (w1[:5], w1[:5].numpy(), dict(indices=idx)),
                                (True, ds.weights.cpu().numpy().astype(np.float64)[idx], dict(indices=idx))):
        res = evaluate.test_per_crystal(pred, ds, batch_size=3, weights=weights, **kw)
        tab = res.per_crystal.cpu().numpy().astype(np.float64)
        if not kw:
            assert torch.equal(res.per_crystal, plain.per_crystal)
        want = (tab * want_w[:, None]).sum(0) / want_w.sum()
        for got, ref in zip(res[:4], want):
            assert abs(got - ref) <= 1e-12 * abs(ref), (got, ref)
    assert abs(res.rmse - float(table[idx, 0].mean())) > 1e-6 * res.rmse                    # (the weights matter)
    with pytest.raises(ValueError, match="weights for 8 crystals"):
        evaluate.test_per_crystal(pred, ds, batch_size=3, weights=w1[:5])
    with pytest.raises(ValueError, match="set_weights"):
        evaluate.test_per_crystal(pred, _dataset32(), batch_size=3, weights=True)
