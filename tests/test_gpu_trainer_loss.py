"""``loss=`` / ``huber_delta=`` of the fused trainers on a real MI355X: ``Trainer`` (phonon, eDOS and the fp32 baseline
``Graphnetwork_phonon``), ``Trainer64`` and ``GraphnetworkTrainer64`` with the per-crystal RMSE, MSE, MAE and Huber losses of
csrc/loss_rows.hip; the models, batches and bars are tests/test_gpu_trainer_guard.py's (L2 T2 H32, 4 - 5 synthetic crystals).

Bars, as test_gpu_trainer_guard.test_small_max_grad_norm_against_the_hand_written_loop: against ``model(batch)`` -> the loss in
torch ops -> ``backward()`` -> ``torch.optim.AdamW`` the loss of each of three steps, every parameter after the third and the first
moment after the first (fp32 5e-5 / 3.1e-4 / 1e-3, float64 1e-12 relative / 1e-9 / 1e-9).  The batch-1 objective: the rules of
tests/test_gpu_train_per_crystal.py (fp32) and the 1e-12 / 1e-10 bars of tests/test_gpu_train64.py (float64).

MAE and Huber have kinks; the hand-written loop and the fused step run different forward kernels, so an output within rounding of
a kink could legitimately take either branch.  The tests assert on the hand loop's own outputs, at every step, that no residual
lies within 1e-4 of 0 (MAE) or of +-delta (Huber); the batches' synthetic seeds (SEEDS) were picked so that this holds."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import test_gpu_train64 as T64
from tests import test_gpu_train_per_crystal as PC
from tests.gpu_util import DEV, _FakeDist
from tests.test_gpu_trainer_guard import MODES, Cfg, _max_diff, _per_tensor, _same, _state

pytestmark = pytest.mark.gpu

KINDS = ["crystal_rmse", "mse", "mae", "huber"]
FAMILIES = ["phonon", "edos", "t64", "gn64", "gnp"]
CASES = [(c, m) for c in FAMILIES for m in ("eager", "replay")] + [("phonon", "graph")]
KINK_MARGIN = 1e-4
# synthetic seed of each family's batch: the first one at which no residual of the hand-written loop comes within KINK_MARGIN of
# 0 or of +-delta on any of the three steps (delta = the median |residual| of the first step)
SEEDS = {"phonon": 71, "edos": 155, "t64": 100, "gn64": 73, "gnp": 74}


class Fam(Cfg):
    """Cfg with the batch made from SEEDS and one more family: "gnp", the fp32 baseline Graphnetwork_phonon under train.Trainer."""

    def __init__(self, name, seed=None):
        from dostransformer_amd import synth
        seed = SEEDS[name] if seed is None else seed
        if name == "gnp":
            from dostransformer_amd.embedder_phDOS.graphnetwork_phonon import Graphnetwork_phonon
            from dostransformer_amd.train import Trainer
            self.name, self.f64, self.beta, self.poison = name, False, 1.0, float("nan")
            self._mk = lambda: Graphnetwork_phonon(2, 118, 4, 32, 51, DEV).to(DEV)
            self.target = "phdos"
            self._tr = lambda m, **kw: Trainer(m, lr=1e-4, **kw)
            self.lr, self.loss_bar = 1e-4, (lambda ref: 5e-5)
            self.param_bar, self.moment_bar, self.norm_bar = 3.1e-4, 1e-3, 1e-4
        else:
            super().__init__(name)
        if name == "phonon":
            self.g = synth.phonon_batch(4, seed=seed, dtype=torch.float32).to(DEV)
        elif name == "edos":
            self.g = synth.edos_batch(4, seed=seed, dtype=torch.float32).to(DEV)
        elif name == "t64":
            self.g = T64._collate(T64._crystals(T64.ATOMS_A, seed)).to(DEV)
        else:
            self.g = synth.phonon_batch(5, seed=seed, dtype=torch.float64 if name == "gn64" else torch.float32).to(DEV)
        self.one = name in ("gn64", "gnp")
        self.B = int(self.g.num_graphs)

    def outputs(self, model, g):
        out = model(g)
        return [out] if self.one else [out[0], out[2]]

    def target_of(self, g, B):
        if self.name == "edos":
            return torch.where(g.y_ft < 0, torch.zeros_like(g.y_ft), g.y_ft).reshape(B, -1)
        return g.phdos.reshape(B, -1)

    def hand(self, model, g, kind, delta=None):
        """the loss written in torch ops -> (loss, |residuals| of every output)"""
        outs = self.outputs(model, g)
        y = self.target_of(g, outs[0].shape[0]).to(outs[0].dtype)

        def f(p):
            p = p.reshape(y.shape)
            if kind == "crystal_rmse":
                return torch.sqrt(((p - y) ** 2).mean(1)).mean()
            if kind == "mse":
                return F.mse_loss(p, y)
            if kind == "mae":
                return F.l1_loss(p, y)
            return F.huber_loss(p, y, delta=delta)

        loss = f(outs[0]) + (self.beta * f(outs[1]) if not self.one else 0.0)
        return loss, torch.cat([(p.reshape(y.shape) - y).detach().abs().reshape(-1) for p in outs])

    def first_delta(self, g=None):
        """The median |residual| of the first step, so that both Huber branches are populated - taken BETWEEN the two middle
        residuals (an odd count: between the middle one and the one below it): delta itself must not be a residual."""
        with torch.no_grad():
            _, r = self.hand(self.model(), self.g if g is None else g, "mse")
        s = r.sort().values
        return float(0.5 * (s[s.numel() // 2 - 1] + s[s.numel() // 2]))


_FAMS = {}


def _fam(name):
    if name not in _FAMS:
        _FAMS[name] = Fam(name)
    return _FAMS[name]


def _kw(c, kind):
    return {"loss": kind, **({"huber_delta": c.first_delta()} if kind == "huber" else {})}


def kink_margin(kind, r, delta):
    """distance of the closest residual to a kink of the loss (inf: the loss has none)"""
    if kind == "mae":
        return float(r.min())
    if kind == "huber":
        return float((r - delta).abs().min())
    return float("inf")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,mode", CASES, ids=[f"{c}-{m}" for c, m in CASES])
def test_loss_kinds_against_the_hand_written_loop(name, mode, kind):
    c = _fam(name)
    kw = _kw(c, kind)
    delta = kw.get("huber_delta")
    tr, _ = c.trainer(mode, **kw)
    hand = c.model()
    opt = torch.optim.AdamW(hand.parameters(), lr=c.lr, weight_decay=1e-2)
    for step in range(3):
        opt.zero_grad()
        ref, r = c.hand(hand, c.g, kind, delta)
        margin = kink_margin(kind, r, delta)
        assert margin > KINK_MARGIN, (step, margin)
        if kind == "huber":
            below = int((r < delta).sum())
            assert 0 < below < r.numel()                                  # both branches are populated ...
            if step == 0:
                assert below == r.numel() // 2                            # ... on the first step by halves: delta is the median
        ref.backward()
        opt.step()
        loss = tr.step(c.g)
        e = abs(float(loss) - float(ref.detach()))
        print(f"{name}-{mode}-{kind} step {step + 1}: loss {float(loss):.8g}, error {e:.3g}, closest residual to a kink {margin:.3g}")
        assert e <= c.loss_bar(float(ref.detach())), (step, e)
        assert tr.crystal_losses.shape == (c.B,) and tr.crystal_losses.is_cuda and tr.crystal_losses.dtype == loss.dtype
        assert abs(float(tr.crystal_losses.mean()) - float(loss)) <= c.loss_bar(float(loss))
        if step == 0:
            worst_m = _per_tensor(tr, hand, lambda n, p: opt.state[p]["exp_avg"], tr._m, True)
    worst_p = _per_tensor(tr, hand, lambda n, p: p.detach(), tr._fp.flat, False)
    print(f"{name}-{mode}-{kind}: worst parameter error {worst_p:.3g} ({c.param_bar:g}), worst relative first-moment error after "
          f"step 1 {worst_m:.3g} ({c.moment_bar:g})")
    assert worst_p <= c.param_bar and worst_m <= c.moment_bar
    if mode != "eager":
        assert (tr.slot_misses, tr.slot_hits) == (1, 2)


# ---- what the feature is for ------------------------------------------------------------------------------------------------
def test_crystal_rmse_with_per_crystal_keys_is_the_mean_of_the_batch_1_gradients_fp32():
    """Trainer(per_crystal_keys=True, loss="crystal_rmse"), one eager step on B crystals: the flat gradient is the mean over the
    crystals of the gradients of the float64 oracle run crystal by crystal with the reference's own loss (O.loss_phonon on a batch
    of one, `main_phDOS.py:52-55,109-114`), by the element-error rule of tests/test_gpu_train_per_crystal.py - and the pooled RMSE
    of the default loss is NOT that (input condition)."""
    from oracle import dos_oracle as O
    from dostransformer_amd.train import Trainer
    name = "ph_h64"
    c = PC.MODELS[name]
    cs = PC._crystals(name)
    B = len(cs)
    model, p = PC._model(name)
    leaves = PC._leaves(p)
    names = list(leaves)
    losses = []
    for cr in cs:
        g1 = PC._collate([cr]).to("cpu", dtype=torch.float64)
        dg, _, ds = PC._oracle_fwd("phonon", leaves, g1, c["L"], c["T"])
        losses.append(O.loss_phonon(dg, ds, g1.phdos, PC.BETA))
    ref = torch.stack(losses).mean()
    grads = dict(zip(names, torch.autograd.grad(ref, [leaves[k] for k in names], allow_unused=True)))
    pooled = PC._oracle_batch1(name, p)[3]                      # the default objective through the same batch-1 forwards
    diff = max(float((pooled[k] - r).abs().max() / (r.abs().max() + 1e-300)) for k, r in grads.items() if r is not None)
    print(f"{name}: pooled-RMSE gradient against the mean of the batch-1 gradients: largest per-tensor difference {diff:.3f}")
    assert diff >= 0.05, diff
    tr = Trainer(model, beta=PC.BETA, per_crystal_keys=True, loss="crystal_rmse")
    loss = tr.forward_backward(PC._collate(cs).to(DEV))
    print(f"{name}: loss {float(loss):.8f}, mean of the batch-1 oracle losses {float(ref):.8f}")
    assert abs(float(loss) - float(ref.detach())) < (1 + PC.BETA) * 1e-4
    ref_each = torch.stack(losses).detach()
    assert float((tr.crystal_losses.cpu().double() - ref_each).abs().max()) < (1 + PC.BETA) * 1e-4
    PC._assert_grads(name + " crystal_rmse", model.flat_params().G, grads)


def test_crystal_rmse_with_per_crystal_keys_is_the_mean_of_the_batch_1_gradients_f64(monkeypatch):
    """Trainer64 on a module with set_per_crystal_keys(True), fp64 softmax on both sides (as tests/test_gpu_train64.py::
    test_trainer64_against_the_oracle_crystal_by_crystal): loss within 1e-12 relative, every tensor of the flat gradient within
    1e-10 of its largest entry."""
    from oracle import dos_oracle as O
    from dostransformer_amd import functional64 as F64
    from dostransformer_amd.train64 import Trainer64
    monkeypatch.setattr(O, "multihead_attention", T64._soft64_mha)
    monkeypatch.setattr(F64, "SOFTMAX64", True)
    base = T64._module()
    beta = 0.7
    cs = T64._crystals(T64.ATOMS_A, 51)
    pr = {k: (v.detach().clone().requires_grad_(True) if v.is_floating_point() else v.clone()) for k, v in base.state_dict().items()}
    losses = []
    for cr in cs:
        g1 = T64._collate([cr])
        out = O.dostransformer_phonon_forward(pr, g1, T64.L_, T64.T_)
        losses.append(O.loss_phonon(out[0], out[2], g1.phdos, beta))
    ref = torch.stack(losses).mean()
    ref.backward()
    model = T64._switch(copy.deepcopy(base), True)
    tr = Trainer64(model, lr=1e-3, beta=beta, loss="crystal_rmse")
    loss = tr.forward_backward(T64._collate(cs).to(DEV))
    e = abs(float(loss) - float(ref.detach())) / abs(float(ref.detach()))
    assert e <= 1e-12, e
    each = torch.stack(losses).detach()
    assert float(((tr.crystal_losses.cpu() - each).abs() / each).max()) <= 1e-12
    worst = 0.0
    for k, got in tr._fp.G.items():
        r = pr[k].grad
        w = float((got.detach().cpu() - r).abs().max() / (r.abs().max() + 1e-300))
        worst = max(worst, w)
        assert w <= 1e-10, (k, w)
    print(f"t64 crystal_rmse: loss error {e:.2e}, worst per-tensor gradient error {worst:.2e}")


# ---- bitwise ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["eager", "replay"])
def test_crystal_rmse_on_edos_trains_the_bits_of_the_default(mode):
    """On an eDOS model the default loss IS the mean of the per-crystal RMSEs: through the new entry, bit for bit the same run."""
    c = _fam("edos")
    plain, _ = c.trainer(mode)
    tr, _ = c.trainer(mode, loss="crystal_rmse")
    for step in range(3):
        assert torch.equal(plain.step(c.g), tr.step(c.g)), step
    assert _same(_state(plain), _state(tr))
    assert plain.crystal_losses is None and tr.crystal_losses.shape == (c.B,)
    assert "dosx_loss_rows" in tr.program_stats()["entries"] and "dosx_loss_edos" not in tr.program_stats()["entries"]
    assert "dosx_loss_rows" not in plain.program_stats()["entries"]


@pytest.mark.parametrize("name", FAMILIES)
def test_replay_is_bitwise_eager_for_every_kind(name):
    """The fp32 trainer replays on the batch ghost-padded to its bucket; the eager step runs on that padded batch (the ghost rows
    are exact, tests/test_gpu_train_per_crystal.py::test_flagged_replay_and_graph_steps_equal_the_eager_step).  The float64
    trainers key their slots by the exact shape."""
    from dostransformer_amd.batch import bucket_sizes, pad_batch
    c = _fam(name)
    for kind in KINDS:
        kw = _kw(c, kind)
        eager, _ = c.trainer("eager", **kw)
        replay, _ = c.trainer("replay", **kw)
        ge = c.g if c.f64 else pad_batch(c.g, *bucket_sizes(c.g.meta.num_nodes, c.g.meta.num_edges, *replay.bucket))
        for step in range(3):
            assert torch.equal(eager.step(ge), replay.step(c.g)), (kind, step)
            assert torch.equal(eager.crystal_losses, replay.crystal_losses), (kind, step)
        assert _same(_state(eager), _state(replay)), kind
        assert replay.slot_hits == 2


def test_step_dataset_records_two_slots_and_replays():
    from tests.test_gpu_weight_ema import _dataset
    c = _fam("phonon")
    ds = _dataset()
    tr, _ = c.trainer("replay", loss="mae")
    twin, _ = c.trainer("eager", loss="mae")
    sels = [np.array([0, 1, 2, 3]), np.array([4, 5, 6, 7])]
    ptrs = []
    for rnd in range(2):
        for sel in sels:
            la, lb = tr.step_dataset(ds, sel), twin.step(ds.collate(sel))
            assert abs(float(la) - float(lb)) <= c.loss_bar(float(lb)), (rnd, sel)
            assert tr.crystal_losses.shape == (4,) and abs(float(tr.crystal_losses.mean()) - float(la)) <= 1e-6
            ptrs.append(tr.crystal_losses.data_ptr())
    assert (tr.slot_misses, tr.slot_hits, len(tr._slots)) == (2, 2, 2)
    assert ptrs[0] == ptrs[2] and ptrs[1] == ptrs[3] and ptrs[0] != ptrs[1]      # views of the two slots' static buffers


# ---- combinations -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", [("phonon", "eager"), ("phonon", "replay"), ("t64", "replay"), ("gnp", "eager")])
def test_crystal_losses_rank_the_doctored_crystal(name, mode):
    """crystal_losses: [B] on the device, its mean the returned loss, its argmax the crystal whose target was scaled by 3; None
    under the default loss."""
    c = _fam(name)
    g = c.g.clone()
    y = c.g.phdos.clone().reshape(c.B, -1)
    y[2] *= 3.0
    g.phdos = y.reshape(c.g.phdos.shape)
    tr, _ = c.trainer(mode, loss="mse")
    for _ in range(2):
        loss = tr.step(g)
        cl = tr.crystal_losses
        assert cl.shape == (c.B,) and cl.is_cuda and cl.dtype == loss.dtype
        assert abs(float(cl.mean()) - float(loss)) <= c.loss_bar(float(loss))
        assert int(cl.argmax()) == 2, cl
    plain, _ = c.trainer(mode)
    plain.step(g)
    assert plain.crystal_losses is None


@pytest.mark.parametrize("name,mode", [(c, m) for c in ("phonon", "edos", "t64", "gn64") for m in ("eager", "replay")])
def test_poisoned_target_under_mse_is_skipped(name, mode):
    """skip_nonfinite=True does not look at the loss: one good step, then Cfg.poisoned() - the step is skipped, parameters and
    moments are bitwise untouched, and crystal_losses names the crystal."""
    c = _fam(name)
    tr, _ = c.trainer(mode, skip_nonfinite=True, loss="mse")
    assert bool(torch.isfinite(tr.step(c.g)))
    before = _state(tr)
    loss = tr.step(c.poisoned())
    assert not bool(torch.isfinite(loss))
    assert _same(before, _state(tr))
    r = tr.guard_report()
    assert r.skipped_last and (r.applied, r.skipped) == (1, 1)
    bad = ~torch.isfinite(tr.crystal_losses)
    assert bad.tolist() == [True] + [False] * (c.B - 1)          # element 7 of the flat target lies in crystal 0


def test_composes_with_the_average_and_a_no_decay_group():
    from dostransformer_amd import param_groups as pg
    c = _fam("phonon")
    m = c.model()
    tr = c._tr(m, replay=True, loss="huber", huber_delta=c.first_delta(), ema_decay=0.99, max_grad_norm=1e30,
               param_groups=[{"params": pg.no_decay(m), "weight_decay": 0.0}])
    for _ in range(3):
        assert bool(torch.isfinite(tr.step(c.g)))
    tr.check()
    assert (tr.slot_misses, tr.slot_hits, tr.step_count) == (1, 2, 3)
    assert tr.guard_report().applied == 3 and tr.crystal_losses.shape == (c.B,)
    assert set(tr.state_dict()["hyper"]) == {"lr", "betas", "eps", "weight_decay", "beta"}          # the checkpoint it always was
    with tr.ema_weights():
        pass


def test_refusals():
    from dostransformer_amd._lib import DosxError
    from dostransformer_amd.train import Trainer
    c, b = _fam("phonon"), _fam("gnp")
    with pytest.raises(DosxError, match="single-GPU mode: not with dist"):
        Trainer(c.model(), dist=_FakeDist(None), loss="mae")
    for fam, mode in ((c, "eager"), (c, "replay"), (b, "eager")):
        tr, _ = fam.trainer(mode, loss="mse")
        with pytest.raises(ValueError, match="n_global"):
            tr.step(fam.g, n_global=fam.B + 1)
    for fam in (c, _fam("t64"), _fam("gn64")):
        with pytest.raises(ValueError, match="crystal_rmse"):
            fam.trainer("eager", loss="rmse")
        with pytest.raises(ValueError, match="huber_delta"):
            fam.trainer("eager", loss="mae", huber_delta=1.0)
        with pytest.raises(ValueError, match="huber_delta"):
            fam.trainer("eager", loss="huber")
