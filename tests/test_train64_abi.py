"""CPU-only checks of the float64 training step's entry points (csrc/f64_train.hip, csrc/adamw.hip) and of train64.Trainer64's refusals:
declared, replayable, prototyped with double hyper-parameters; arguments are refused before any launch; which modules
Trainer64 takes.  (Exports, thunks and argument types against the header: tests/test_lib_abi.py, for the whole header.)"""
import os

import pytest
import torch

from tests.util import dosx_lib as _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["dosx_loss_phonon_f64", "dosx_adamw_f64"]


def test_train64_symbols_declared_exported_replayable_and_prototyped():
    import ctypes as C
    _l = _lib()
    lib = _l.load()
    header = open(os.path.join(ROOT, "include", "dosx.h")).read()
    for n in SYMBOLS:
        assert f"int {n}(" in header, n
        ni, nf = C.c_int(0), C.c_int(0)
        assert lib.dosx_replay_op(n.encode(), C.byref(ni), C.byref(nf)) >= 0, n
        args = getattr(lib, n).argtypes
        assert len(args) == ni.value + nf.value, n
        assert sum(1 for t in args if t is C.c_double) == nf.value, n          # every hyper-parameter replays as a double
    assert _l._SIGS["dosx_loss_phonon_f64"].count(C.c_double) == 1 and _l._SIGS["dosx_adamw_f64"].count(C.c_double) == 5


def test_train64_argument_validation_needs_no_gpu():
    lib = _lib().load()
    err = lambda: lib.dosx_last_error().decode()
    fake = 4096                                   # never dereferenced: every call below is refused before any launch
    loss = lambda *a: lib.dosx_loss_phonon_f64(*a, None)
    ok = [fake, fake, fake, 1.0, fake, fake, fake, None, 51]
    for i in (0, 1, 2, 4, 5, 6):                  # every pointer but sse
        a = list(ok)
        a[i] = None
        assert loss(*a) == -22 and "dosx_loss_phonon_f64" in err() and "NULL" in err(), i
    for count in (0, -3):
        assert loss(*ok[:8], count) == -22 and "count" in err() and str(count) in err()
    adam = lambda p, g, m, v, n, step: lib.dosx_adamw_f64(p, g, m, v, n, 1e-4, 0.9, 0.999, 1e-8, 1e-2, step, None)
    for i in range(4):
        a = [fake] * 4
        a[i] = None
        assert adam(*a, 8, 1) == -22 and "dosx_adamw_f64" in err() and "NULL" in err(), i
    for step in (0, -1):
        assert adam(fake, fake, fake, fake, 8, step) == -22 and "step" in err() and str(step) in err()
    assert adam(fake, fake, fake, fake, -1, 1) == -22 and "n must not be negative" in err()
    for i in range(4):
        a = [fake] * 4
        a[i] = fake + 8                           # a double-aligned pointer that is not 16-byte aligned
        assert adam(*a, 8, 1) == -22 and "16-byte aligned" in err(), i
    assert adam(fake, fake, fake, fake, 0, 1) == 0                                # nothing to do, nothing launched


def _phonon(dtype=torch.float64):
    from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
    torch.manual_seed(0)
    return DOSTransformer_phonon(2, 1, 118, 4, 16, "cpu", 0.0).to(dtype)


def test_trainer64_takes_only_a_float64_switched_phonon_module():
    from dostransformer_amd._lib import DosxError
    from dostransformer_amd.embedder_eDOS.DOSTransformer import DOSTransformer
    from dostransformer_amd.embedder_phDOS.graphnetwork_phonon import Graphnetwork_phonon
    from dostransformer_amd.train import Trainer
    from dostransformer_amd.train64 import Trainer64
    for bad in (_phonon(torch.float32),                                  # the fp32 program
                _phonon(),                                               # float64 parameters, not switched: still the fp32 program
                DOSTransformer(2, 1, 200, 41, 2, 16, "cpu", 0.0),        # eDOS
                DOSTransformer(2, 1, 200, 41, 2, 16, "cpu", 0.0).double(),
                Graphnetwork_phonon(2, 118, 4, 16, 16, "cpu").double(),
                torch.nn.Linear(2, 2)):
        with pytest.raises(DosxError, match="Trainer"):
            Trainer64(bad)
    m64 = _phonon().set_program_dtype(torch.float64)
    tr = Trainer64(m64, lr=1e-3, beta=0.5, replay=True, max_slots=3)
    assert (tr.lr, tr.beta, tr.replay, tr.max_slots, tr.step_count, tr.slot_hits, tr.slot_misses) == (1e-3, 0.5, True, 3, 0, 0, 0)
    with pytest.raises(TypeError):
        Trainer64(m64, dist=None)                  # no parameters that only raise
    with pytest.raises(TypeError):
        Trainer64(m64, graph=True)
    # switched back to fp32 under a live driver: refused at the step, before anything runs
    m64.set_program_dtype(torch.float32)
    with pytest.raises(DosxError, match="Trainer"):
        tr.forward_backward(object())
    m64.set_program_dtype(torch.float64)
    with pytest.raises(DosxError, match="loss.backward") as e:
        Trainer(m64)
    assert "Trainer64" in str(e.value)


def test_trainer64_state_dict_is_float64_in_adamw_vocabulary():
    from dostransformer_amd.train64 import Trainer64
    m64 = _phonon().set_program_dtype(torch.float64)
    tr = Trainer64(m64, lr=3e-4)
    sd = tr.state_dict()
    assert set(sd) == {"step", "exp_avg", "exp_avg_sq", "drop_seed_base", "hyper"} and sd["step"] == 0
    fp = m64.flat_params()
    assert set(sd["exp_avg"]) == set(fp.names) == set(sd["exp_avg_sq"])
    assert all(v.dtype == torch.float64 and v.shape == fp.P[k].shape for k, v in sd["exp_avg"].items())
    sd["step"] = 7
    sd["exp_avg"] = {k: torch.full_like(v, 0.25) for k, v in sd["exp_avg"].items()}
    sd["hyper"]["lr"] = 5e-4
    tr2 = Trainer64(_phonon().set_program_dtype(torch.float64))
    tr2.load_state_dict(sd)
    assert tr2.step_count == 7 and tr2.lr == 5e-4 and tr2._m.dtype == torch.float64
    assert all(bool((v == 0.25).all()) for v in tr2.state_dict()["exp_avg"].values())
