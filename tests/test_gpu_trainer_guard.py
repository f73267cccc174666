"""The guarded optimizer step through the trainers on a real MI355X: ``Trainer`` (phonon and eDOS), ``Trainer64`` and
``GraphnetworkTrainer64`` with ``max_grad_norm`` / ``skip_nonfinite``, each in eager and ``replay=True`` mode, ``Trainer`` also
with ``graph=True``; the smallest models of the suite (L2 T2 H32, 4 - 5 synthetic crystals, as tests/test_gpu_train64.py).

Bars.  Against the hand-written loop (``model(batch)`` -> loss -> ``backward()`` -> ``clip_grad_norm_`` -> ``torch.optim.AdamW``):
fp32 the loss within 5e-5 and every parameter within 3.1e-4 after three steps at lr = 1e-4
(tests/test_gpu_step.py::test_reference_style_loop_with_fp64_batches_and_torch_adamw), float64 the loss within 1e-12 relative and
every parameter within 1e-9 (tests/test_gpu_train64.py::test_trainer64_eager_against_the_hand_written_loop).  AdamW's update
m / sqrt(v) hardly depends on the gradient's scale, so the parameters alone would not notice a coefficient that was never
applied; the first moment does, linearly.  It is therefore compared too, after the FIRST step - both sides then started from the
same parameters, so their gradients come from the same kernels on the same inputs and differ by summation order alone (1e-5 /
1e-10 per tensor in the tests named above; later steps add the fp32 trajectories' own drift, which these small eDOS models
amplify) - per tensor relative to the tensor's largest entry: within 1e-3 (fp32) / 1e-9 (float64); a dropped coefficient of 0.05
shows as a factor 20."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import test_gpu_train64 as T64
from tests.gpu_util import DEV, _FakeDist
from tests.test_gpu_baselines64 import _gn

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
MODES = {"eager": {}, "replay": {"replay": True}, "graph": {"graph": True}}
CASES = [(c, m) for c in ("phonon", "edos", "t64", "gn64") for m in ("eager", "replay")] + [("phonon", "graph")]
IDS = [f"{c}-{m}" for c, m in CASES]


class Cfg:
    """One trainer family: model factory (same bits every call), trainer factory, one batch, the target's field, the
    hand-written loss, the bars."""

    def __init__(self, name):
        from dostransformer_amd import synth
        from dostransformer_amd.train import Trainer
        from dostransformer_amd.train64 import GraphnetworkTrainer64, Trainer64
        self.name, self.f64 = name, name in ("t64", "gn64")
        self.beta = 0.7
        # a NaN in an eDOS target never reaches the loss: dosx_loss_edos clamps the target with fmaxf(y, 0), which returns 0 for a
        # NaN - the poison of that case is +inf, which the clamp keeps
        self.poison = INF if name == "edos" else NAN
        if name == "phonon":
            from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
            self._mk = lambda: DOSTransformer_phonon(2, 2, 118, 4, 32, DEV, 0.0).to(DEV)
            self.g, self.target = synth.phonon_batch(4, seed=71, dtype=torch.float32).to(DEV), "phdos"
            self._tr = lambda m, **kw: Trainer(m, lr=1e-4, beta=self.beta, **kw)
        elif name == "edos":
            from dostransformer_amd.embedder_eDOS.DOSTransformer import DOSTransformer
            self._mk = lambda: DOSTransformer(2, 2, 200, 41, 2, 32, DEV, 0.0).to(DEV)
            self.g, self.target = synth.edos_batch(4, seed=72, dtype=torch.float32).to(DEV), "y_ft"
            self._tr = lambda m, **kw: Trainer(m, lr=1e-4, beta=self.beta, **kw)
        elif name == "t64":
            base = T64._module()
            self._mk = lambda: T64._switch(copy.deepcopy(base), True)
            self.g, self.target = T64._collate(T64._crystals(T64.ATOMS_A, 51)).to(DEV), "phdos"
            self._tr = lambda m, **kw: Trainer64(m, lr=1e-3, beta=self.beta, **kw)
        else:
            base = _gn(32, seed=5)
            self._mk = lambda: copy.deepcopy(base).to(DEV)
            self.g, self.target = synth.phonon_batch(5, seed=73, dtype=torch.float64).to(DEV), "phdos"
            self._tr = lambda m, **kw: GraphnetworkTrainer64(m, lr=1e-3, **kw)
        self.lr = 1e-3 if self.f64 else 1e-4
        self.loss_bar = (lambda ref: 1e-12 * abs(ref)) if self.f64 else (lambda ref: 5e-5)
        self.param_bar, self.moment_bar, self.norm_bar = (1e-9, 1e-9, 1e-10) if self.f64 else (3.1e-4, 1e-3, 1e-4)

    def model(self):
        torch.manual_seed(3)
        return self._mk()

    def trainer(self, mode, **kw):
        m = self.model()
        return self._tr(m, **MODES[mode], **kw), m

    def hand_loss(self, model, g):
        out = model(g)
        if self.name == "gn64":
            return torch.sqrt(F.mse_loss(out, g.phdos.reshape(out.shape)))
        dg, _, ds = out
        if self.name == "edos":
            y = torch.where(g.y_ft < 0, torch.zeros_like(g.y_ft), g.y_ft).reshape(dg.shape[0], -1)
            return torch.sqrt(((y - dg) ** 2).mean(1)).mean() + self.beta * torch.sqrt(((y - ds) ** 2).mean(1)).mean()
        return torch.sqrt(F.mse_loss(dg, g.phdos)) + self.beta * torch.sqrt(F.mse_loss(ds, g.phdos))

    def poisoned(self):
        """the batch with ONE target element replaced: only the loss and the gradients see it, no index does"""
        bad = self.g.clone()
        t = getattr(self.g, self.target).clone()
        t.view(-1)[7] = self.poison
        setattr(bad, self.target, t)
        return bad


_CFGS = {}


def _cfg(name):
    if name not in _CFGS:
        _CFGS[name] = Cfg(name)
    return _CFGS[name]


def _state(tr):
    torch.cuda.synchronize()
    return tr._fp.flat.clone(), tr._m.clone(), tr._v.clone()


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _max_diff(a, b):
    return float((a - b).abs().max())


def _per_tensor(tr, hand, ref_of, flat, relative):
    """worst difference, over the live parameters, between the trainer's flat buffer and the hand-written loop's tensor ref_of(name,
    parameter); relative: to the reference tensor's largest entry"""
    fp, params, worst = tr._fp, dict(hand.named_parameters()), 0.0
    for n, o in zip(fp.names, fp.offsets):
        ref = ref_of(n, params[n]).reshape(-1)
        e = _max_diff(flat[o:o + ref.numel()], ref)
        worst = max(worst, e / (float(ref.abs().max()) + 1e-300) if relative else e)
    return worst


@pytest.mark.parametrize("name,mode", CASES, ids=IDS)
def test_guard_on_and_nothing_trips_is_bitwise_the_unguarded_trainer(name, mode):
    """skip_nonfinite=True, max_grad_norm=1e30, three steps: losses, parameters and moments are bit for bit those of the same
    trainer without the arguments - and the record counted three applied steps with a coefficient of exactly 1."""
    c = _cfg(name)
    plain, _ = c.trainer(mode)
    guarded, _ = c.trainer(mode, skip_nonfinite=True, max_grad_norm=1e30)
    assert guarded.guarded and not plain.guarded
    for step in range(3):
        la, lb = plain.step(c.g), guarded.step(c.g)
        assert torch.equal(la, lb), step
    assert _same(_state(plain), _state(guarded))
    r = guarded.guard_report()
    assert (r.applied, r.skipped, r.skipped_last, r.clip, r.n_bad, r.first_bad, r.reasons) == (3, 0, False, 1.0, 0, None, ())
    assert r.norm > 0 and float(guarded.grad_norm) == r.norm and guarded.grad_norm.is_cuda and guarded.grad_norm.dim() == 0
    assert guarded.step_count == plain.step_count == 3 and guarded.state_dict()["step"] == 3
    guarded.check()                                                     # nothing skipped: nothing raised


@pytest.mark.parametrize("name,mode", CASES, ids=IDS)
def test_small_max_grad_norm_against_the_hand_written_loop(name, mode):
    """max_grad_norm = a twentieth of the first step's norm (read from guard_report(); the norm of these small models falls by up
    to 7x within three steps), three steps: the coefficient is < 1 on every one of them and the trainer follows model(batch) ->
    loss -> backward() -> clip_grad_norm_ -> torch.optim.AdamW at the bars of the module docstring; the gradient buffer keeps the
    UNCLIPPED gradient."""
    c = _cfg(name)
    probe, _ = c.trainer(mode, skip_nonfinite=True)
    probe.step(c.g)
    mx = 0.05 * probe.guard_report().norm
    assert mx > 0
    tr, fused = c.trainer(mode, max_grad_norm=mx)
    hand = c.model()
    opt = torch.optim.AdamW(hand.parameters(), lr=c.lr, weight_decay=1e-2)
    for step in range(3):
        opt.zero_grad()
        ref = c.hand_loss(hand, c.g)
        ref.backward()
        total = float(torch.nn.utils.clip_grad_norm_(hand.parameters(), mx))
        opt.step()
        loss = tr.step(c.g)
        r = tr.guard_report()
        e = abs(float(loss) - float(ref.detach()))
        print(f"{name}-{mode} step {step + 1}: loss error {e:.3g}, norm {r.norm:.6g} against {total:.6g}, coefficient {r.clip:.4f}")
        assert e <= c.loss_bar(float(ref.detach())), (step, e)
        assert r.clip < 1.0 and not r.skipped_last and r.applied == step + 1
        assert abs(r.norm - total) <= c.norm_bar * total and abs(r.clip - mx / (total + 1e-6)) <= 2 * c.norm_bar
        g2 = float(tr._fp.grad.double().pow(2).sum().sqrt())
        assert abs(g2 - r.norm) <= 1e-6 * r.norm                        # the flat gradient is the unclipped one
        if step == 0:
            worst_m = _per_tensor(tr, hand, lambda n, p: opt.state[p]["exp_avg"], tr._m, True)
    worst_p = _per_tensor(tr, hand, lambda n, p: p.detach(), tr._fp.flat, False)
    print(f"{name}-{mode}: worst parameter error {worst_p:.3g} ({c.param_bar:g}), worst relative first-moment error after step 1 "
          f"{worst_m:.3g} ({c.moment_bar:g})")
    assert worst_p <= c.param_bar and worst_m <= c.moment_bar


@pytest.mark.parametrize("name,mode", CASES, ids=IDS)
def test_poisoned_target_is_skipped_reported_and_recovered_from(name, mode):
    """One good step, then a batch whose target holds one NaN (+inf for eDOS, see Cfg): the step is skipped, parameters and
    moments stay bitwise, guard_report() names a live parameter.  A further good step before check() either applies or - a
    stale non-finite value in a replayed slot - is skipped too with the state intact.  check() raises DosxError with the step
    number, after which step_count is the applied count; two further good batches then give the parameters of a trainer that
    never saw the bad batch, at the bars of the module docstring."""
    from dostransformer_amd._lib import DosxError
    c = _cfg(name)
    tr, _ = c.trainer(mode, skip_nonfinite=True)
    twin, _ = c.trainer(mode)
    bad = c.poisoned()
    assert torch.equal(tr.step(c.g), twin.step(c.g))
    before = _state(tr)
    loss = tr.step(bad)
    assert not bool(torch.isfinite(loss))
    assert _same(before, _state(tr))
    r = tr.guard_report()
    assert r.skipped_last and "non-finite gradient" in r.reasons and (r.applied, r.skipped, r.first_skip_step) == (1, 1, 2) and r.n_bad > 0
    pname, pidx = r.first_bad
    assert pname in tr._fp.names and 0 <= pidx < tr._fp.P[pname].numel() and r.first_skip_bad == r.first_bad
    assert tr.state_dict()["step"] == 1 and tr.step_count == 2
    tr.step(c.g)
    r = tr.guard_report()
    applied = 1
    if r.skipped_last:                                                  # a stale non-finite value survived in the slot
        assert _same(before, _state(tr)) and (r.applied, r.skipped) == (1, 2)
    else:
        twin.step(c.g)
        applied = 2
        assert (r.applied, r.skipped) == (2, 1)
    print(f"{name}-{mode}: the good step behind the poisoned one was {'skipped too' if r.skipped_last else 'applied'}")
    with pytest.raises(DosxError, match=r"step 2: gradient of .*\[\d+\] is not finite"):
        tr.check()
    assert tr.step_count == applied and tr.guard_report().skipped == 0 and len(tr._slots) == 0
    tr.check()                                                          # settled: does not raise again
    for _ in range(2):
        la, lb = tr.step(c.g), twin.step(c.g)
        assert abs(float(la) - float(lb)) <= c.loss_bar(float(lb))
    r = tr.guard_report()
    assert (r.applied, r.skipped) == (2, 0) and tr.step_count == twin.step_count == applied + 2
    a, b = _state(tr), _state(twin)
    e = _max_diff(a[0], b[0])
    print(f"{name}-{mode}: parameters against the trainer that never saw the bad batch: {e:.3g} ({c.param_bar:g})")
    assert e <= c.param_bar
    for x, y in zip(a[1:], b[1:]):
        assert _max_diff(x, y) <= c.moment_bar * float(y.abs().max())


@pytest.mark.parametrize("name", ["phonon", "t64"])
def test_checkpoint_round_trip_after_a_skip(name):
    """good, poisoned (skipped), good: state_dict()["step"] is the applied count 2, before and after check(); a fresh trainer
    that loads the checkpoint has step_count 2 and a zeroed record, and continues bit for bit with the settled original."""
    from dostransformer_amd._lib import DosxError
    c = _cfg(name)
    tr, model = c.trainer("eager", skip_nonfinite=True, max_grad_norm=1e30)
    for g in (c.g, c.poisoned(), c.g):
        tr.step(g)
    assert tr.step_count == 3 and tr.state_dict()["step"] == 2
    with pytest.raises(DosxError, match="step 2"):
        tr.check()
    sd, msd = tr.state_dict(), copy.deepcopy(model.state_dict())
    assert sd["step"] == 2 and tr.step_count == 2
    tr2, model2 = c.trainer("eager", skip_nonfinite=True, max_grad_norm=1e30)
    tr2.step(c.poisoned())                                              # something in the record for load_state_dict to zero
    model2.load_state_dict(msd)
    tr2.load_state_dict(sd)
    assert tr2.step_count == 2 and tr2.guard_report().skipped == 0 and tr2.guard_report().applied == 0
    for _ in range(2):
        assert torch.equal(tr.step(c.g), tr2.step(c.g))
    assert _same(_state(tr), _state(tr2)) and tr.state_dict()["step"] == tr2.state_dict()["step"] == 4


def test_step_dataset_runs_behind_the_guard():
    """Trainer.step_dataset (collate into the bucket + replay) with the guard on and nothing tripping: bitwise the unguarded one."""
    from dostransformer_amd import synth
    from dostransformer_amd.loader import DeviceDataset
    c = _cfg("phonon")
    cs = synth.phonon_crystals(8, seed=43, dtype=torch.float32)
    ds = DeviceDataset(cs, DEV)
    nmax = max(int(x["x"].shape[0]) for x in cs)
    plain, _ = c.trainer("replay")
    guarded, _ = c.trainer("replay", max_grad_norm=1e30)
    for sel in ([0, 1, 2, 3], [4, 5, 6, 7], [3, 2, 1, 0]):
        assert torch.equal(plain.step_dataset(ds, np.array(sel), n_max=nmax), guarded.step_dataset(ds, np.array(sel), n_max=nmax))
    assert _same(_state(plain), _state(guarded)) and guarded.guard_report().applied == 3


def test_refusals():
    """dist= together with the guard raises DosxError (as per_crystal_keys does), a negative max_grad_norm ValueError, and a
    trainer without the guard has no record to report."""
    from dostransformer_amd._lib import DosxError
    from dostransformer_amd.train import Trainer
    from dostransformer_amd.train64 import GraphnetworkTrainer64, Trainer64
    c = _cfg("phonon")
    for kw in ({"max_grad_norm": 1.0}, {"skip_nonfinite": True}):
        with pytest.raises(DosxError, match="not with dist"):
            Trainer(c.model(), dist=_FakeDist(None), **kw)
    Trainer(c.model(), dist=_FakeDist(None))                            # without the guard: accepted as before
    with pytest.raises(ValueError, match="max_grad_norm"):
        Trainer(c.model(), max_grad_norm=-1.0)
    with pytest.raises(ValueError, match="max_grad_norm"):
        Trainer64(_cfg("t64").model(), max_grad_norm=-0.5)
    with pytest.raises(ValueError, match="max_grad_norm"):
        GraphnetworkTrainer64(_cfg("gn64").model(), max_grad_norm=float("nan"))
    plain = Trainer(c.model())
    with pytest.raises(DosxError, match="no gradient guard"):
        plain.guard_report()
    with pytest.raises(DosxError, match="no gradient guard"):
        plain.grad_norm
