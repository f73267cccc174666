"""CPU-only checks of the host side of the weight average (dostransformer_amd/ema.py and the ``ema_decay=`` / ``ema_warmup=``
arguments of the trainers): validation, the refusal under data parallelism, the checkpoint keys and the three load
combinations, re-homing by name, and ``ema_weights()`` on a module that is not on the GPU - REFUSED (the swap is a device launch),
not a silent no-op.  Modules on the CPU; nothing is launched."""
import io

import pytest
import torch

LR, WD = 1e-3, 1e-2
PLAIN_KEYS = ["drop_seed_base", "exp_avg", "exp_avg_sq", "hyper", "step"]


def _phonon(L=2, T=1, H=16, seed=0):
    from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
    torch.manual_seed(seed)
    return DOSTransformer_phonon(L, T, 118, 4, H, "cpu", 0.0)


def _save_load(obj):
    buf = io.BytesIO()
    torch.save(obj, buf)
    buf.seek(0)
    return torch.load(buf, weights_only=True)


def test_constructors_validate_the_decay():
    from dostransformer_amd._lib import DosxError
    from dostransformer_amd.train import Trainer
    from dostransformer_amd.train64 import GraphnetworkTrainer64, Trainer64
    import inspect
    for cls in (Trainer, Trainer64, GraphnetworkTrainer64):
        sig = inspect.signature(cls.__init__).parameters
        assert sig["ema_decay"].default is None and sig["ema_warmup"].default is True, cls
    for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"Trainer: ema_decay must be in \[0, 1\) or None"):
            Trainer(_phonon(), ema_decay=bad)
    for ok in (0.0, 0.5, 0.9999):
        tr = Trainer(_phonon(), ema_decay=ok)
        assert tr.ema_decay == ok and tr.ema_warmup is True
    tr = Trainer(_phonon(), ema_decay=0.9, ema_warmup=False)
    assert tr.ema_warmup is False
    tr.ema_decay = 0.99                                         # read at every step: assignable between steps
    assert tr.ema_decay == 0.99
    with pytest.raises(ValueError, match="ema_decay must be in"):
        tr.ema_decay = 1.0
    with pytest.raises(ValueError, match="cannot be switched off"):
        tr.ema_decay = None
    assert tr.ema_decay == 0.99
    plain = Trainer(_phonon())
    assert plain.ema_decay is None
    with pytest.raises(DosxError, match="built without ema_decay"):
        plain.ema_decay = 0.9
    for what in (plain.ema_state_dict, lambda: plain.ema_weights().__enter__()):
        with pytest.raises(DosxError, match="keeps no weight average"):
            what()
    # the float64 drivers validate the same way, in front of their model check's successor
    m64 = _phonon().double().set_program_dtype(torch.float64)
    with pytest.raises(ValueError, match=r"Trainer64: ema_decay must be in \[0, 1\)"):
        Trainer64(m64, ema_decay=2.0)
    assert Trainer64(m64, ema_decay=0.5, ema_warmup=False).ema_decay == 0.5


def test_refused_under_data_parallelism():
    from dostransformer_amd._lib import DosxError
    from dostransformer_amd.train import Trainer
    from tests.gpu_util import _FakeDist
    with pytest.raises(DosxError, match=r"Trainer\(ema_decay=\.\.\.\) is a single-GPU mode: not with dist"):
        Trainer(_phonon(), dist=_FakeDist(None), ema_decay=0.9)
    assert Trainer(_phonon(), dist=_FakeDist(None)).ema_decay is None          # (without: as before)


def test_state_dict_keys_appear_only_with_an_average():
    from dostransformer_amd.train import Trainer
    plain = Trainer(_phonon(), lr=LR, weight_decay=WD)
    assert sorted(plain.state_dict()) == PLAIN_KEYS                                                  # the file it always wrote
    tr = Trainer(_phonon(), lr=LR, weight_decay=WD, ema_decay=0.9, ema_warmup=False)
    sd = _save_load(tr.state_dict())
    assert sorted(set(sd) - set(PLAIN_KEYS)) == ["ema", "ema_hyper"]
    assert sd["ema_hyper"] == {"decay": 0.9, "warmup": False, "t0": 0}
    fp = tr._fp
    assert sorted(sd["ema"]) == sorted(fp.names) == sorted(sd["exp_avg"])
    for n in fp.names:                                           # the average starts at the parameters, in the flat dtype
        assert sd["ema"][n].dtype == torch.float32 and torch.equal(sd["ema"][n], fp.P[n].detach())
    assert tr._ema.shape == fp.flat.shape and tr._ema.dtype == fp.flat.dtype and tr._ema.data_ptr() != fp.flat.data_ptr()


def test_the_three_load_combinations():
    from dostransformer_amd.train import Trainer
    src = Trainer(_phonon(seed=1), lr=LR, weight_decay=WD, ema_decay=0.95, ema_warmup=True)
    src._state(src.model.flat_params())
    with torch.no_grad():
        src._ema.mul_(0.5)
        src._m.fill_(0.25)
    src.step_count, src._ema_t0 = 7, 3
    sd = _save_load(src.state_dict())
    assert sd["ema_hyper"] == {"decay": 0.95, "warmup": True, "t0": 3} and sd["step"] == 7
    # 1. a file with an average into a trainer with one: restored by name, hyper-parameters included
    a = Trainer(_phonon(seed=2), lr=LR, weight_decay=WD, ema_decay=0.5, ema_warmup=False)
    a.load_state_dict(sd)
    assert (a.ema_decay, a.ema_warmup, a._ema_t0, a.step_count) == (0.95, True, 3, 7)
    assert a._fp.names == src._fp.names and torch.equal(a._ema, src._ema) and bool((a._m[:8] == 0.25).all())
    assert not torch.equal(a._ema, a._fp.flat)
    # 2. a file without into a trainer with: the average starts at the loaded parameters, t0 = the file's step
    plain_sd = dict(sd)
    del plain_sd["ema"], plain_sd["ema_hyper"]
    b = Trainer(_phonon(seed=2), lr=LR, weight_decay=WD, ema_decay=0.5, ema_warmup=False)
    b.load_state_dict(plain_sd)
    assert (b.ema_decay, b.ema_warmup, b._ema_t0, b.step_count) == (0.5, False, 7, 7)
    assert torch.equal(b._ema, b._fp.flat) and b._ema.data_ptr() != b._fp.flat.data_ptr()
    # 3. a file with into a trainer without: ignored, and the file it writes is the plain one
    c = Trainer(_phonon(seed=2), lr=LR, weight_decay=WD)
    c.load_state_dict(sd)
    assert c.ema_decay is None and c._ema is None and c.step_count == 7 and bool((c._m[:8] == 0.25).all())
    assert sorted(c.state_dict()) == PLAIN_KEYS
    # a file whose average lacks a parameter is refused by name
    broken = dict(sd)
    broken["ema"] = {k: v for k, v in sd["ema"].items() if k != "fc.weight"}
    with pytest.raises(KeyError, match="weight average lacks"):
        Trainer(_phonon(seed=2), ema_decay=0.5).load_state_dict(broken)


def test_the_average_follows_a_new_layout_by_name():
    from dostransformer_amd.train import Trainer
    model = _phonon()
    tr = Trainer(model, ema_decay=0.9)
    tr._state(model.flat_params())
    fp0 = tr._fp
    with torch.no_grad():
        tr._ema.copy_(torch.arange(fp0.total, dtype=torch.float32))
    before = {n: tr._ema[o:o + fp0.P[n].numel()].clone() for n, o in zip(fp0.names, fp0.offsets)}
    tr.step_count = 4
    model.freeze("GN_encoder.")
    fp1 = model.flat_params()
    assert fp1 is not fp0 and fp1.names != fp0.names
    tr._state(fp1)
    assert tr._fp is fp1 and tr._ema_t0 == 0                     # (averaging began at step 0: re-homing does not restart it)
    for n, o in zip(fp1.names, fp1.offsets):
        assert torch.equal(tr._ema[o:o + fp1.P[n].numel()], before[n]), n


def test_ema_state_dict_has_the_models_keys():
    from dostransformer_amd.train import Trainer
    model = _phonon()
    tr = Trainer(model, ema_decay=0.9)
    tr._state(model.flat_params())
    with torch.no_grad():
        tr._ema.add_(1.0)
    sd = tr.ema_state_dict()
    ref = model.state_dict()
    assert list(sd) == list(ref)
    live = set(tr._fp.names)
    assert live and any(k not in live for k in ref)              # (dead parameters: the model's own values)
    for k, v in ref.items():
        assert sd[k].device.type == "cpu" and sd[k].shape == v.shape and sd[k].dtype == v.dtype
        assert torch.equal(sd[k], v.detach() + 1.0 if k in live else v.detach()), k
    fresh = _phonon(seed=5)
    fresh.load_state_dict(sd)                                    # serves plain_model.load_state_dict(...)


def test_ema_weights_on_a_cpu_module_is_refused():
    from dostransformer_amd._lib import DosxError
    from dostransformer_amd.train import Trainer
    model = _phonon()
    tr = Trainer(model, ema_decay=0.9)
    flat = model.flat_params().flat.clone()
    with pytest.raises(DosxError, match=r"ema_weights: the module is on cpu"):
        with tr.ema_weights():
            raise AssertionError("the body must not run")
    assert tr._ema_block is False and torch.equal(model.flat_params().flat, flat)
    assert sorted(set(tr.state_dict()) - set(PLAIN_KEYS)) == ["ema", "ema_hyper"]       # nothing is left in the refusing state


def test_inside_the_block_the_trainer_refuses():
    """The block's flag alone (set by hand: no launch on the CPU) makes every entry that trains, freezes or checkpoints raise,
    naming the block; ``_state`` is what a freeze() inside runs into at the next step."""
    from dostransformer_amd._lib import DosxError
    from dostransformer_amd.train import Trainer
    model = _phonon()
    tr = Trainer(model, ema_decay=0.9)
    tr._state(model.flat_params())
    tr._ema_block = True
    calls = {"step": lambda: tr.step(None), "step_dataset": lambda: tr.step_dataset(None, [0]),
             "forward_backward": lambda: tr.forward_backward(None), "optimizer_step": tr.optimizer_step,
             "state_dict": tr.state_dict, "load_state_dict": lambda: tr.load_state_dict({}),
             "_state": lambda: tr._state(model.flat_params())}
    for name, fn in calls.items():
        with pytest.raises(DosxError, match=r"inside `with trainer\.ema_weights\(\):`") as e:
            fn()
        assert f"Trainer.{name}" in str(e.value), (name, str(e.value))
    with pytest.raises(DosxError, match="does not nest"):
        tr.ema_weights().__enter__()
    tr._ema_block = False
    assert sorted(set(tr.state_dict()) - set(PLAIN_KEYS)) == ["ema", "ema_hyper"]
