"""CPU-only checks of the per-crystal loss entries (csrc/loss_rows.hip: dosx_loss_rows / dosx_loss_rows_f64) and of the trainers'
``loss=`` / ``huber_delta=`` arguments: declared, exported, replayable, prototyped with their scalars in the operands' type;
every refusal of include/dosx.h comes back as -22 with a message that names the entry, before any launch; the argument errors
of the three trainers.  (Exports, thunks and argument types against the header: tests/test_lib_abi.py, for the whole header.)"""
import ctypes as C
import math
import os

import pytest
import torch

from tests.util import dosx_lib as _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"dosx_loss_rows": C.c_float, "dosx_loss_rows_f64": C.c_double}
FAKE = 4096                                       # never dereferenced: every call below is refused before any launch


def test_loss_rows_symbols_declared_exported_replayable_and_prototyped():
    _l = _lib()
    lib = _l.load()
    header = open(os.path.join(ROOT, "include", "dosx.h")).read()
    for n, scalar in SYMBOLS.items():
        assert f"int {n}(" in header, n
        assert hasattr(lib, n), n
        ni, nf = C.c_int(0), C.c_int(0)
        assert lib.dosx_replay_op(n.encode(), C.byref(ni), C.byref(nf)) >= 0, n
        args = getattr(lib, n).argtypes
        assert len(args) == 15 and len(args) == ni.value + nf.value, n
        other = C.c_double if scalar is C.c_float else C.c_float
        assert _l._SIGS[n].count(scalar) == 2 == nf.value and _l._SIGS[n].count(other) == 0, n       # beta, delta
        assert _l._SIGS[n].count(C.c_int) == 5, n                                                     # B, S, B_global, kind, clamp_target
    from dostransformer_amd import _abi, ops
    assert (_abi.DOSX_LOSS_RMSE, _abi.DOSX_LOSS_MSE, _abi.DOSX_LOSS_MAE, _abi.DOSX_LOSS_HUBER) == (0, 1, 2, 3)
    assert ops.LOSS_KINDS == {"crystal_rmse": _abi.DOSX_LOSS_RMSE, "mse": _abi.DOSX_LOSS_MSE, "mae": _abi.DOSX_LOSS_MAE,
                              "huber": _abi.DOSX_LOSS_HUBER}


@pytest.mark.parametrize("name", list(SYMBOLS))
def test_loss_rows_argument_validation_needs_no_gpu(name):
    lib = _lib().load()
    err = lambda: lib.dosx_last_error().decode()
    fn = getattr(lib, name)
    # pg, ps, y, B, S, B_global, kind, clamp_target, beta, delta, dpg, dps, per_crystal, loss
    ok = [FAKE, FAKE, FAKE, 5, 51, 5, 0, 0, 1.0, 0.0, FAKE, FAKE, FAKE, FAKE]
    call = lambda a: fn(*a, None)

    def refused(a, *words):
        assert call(a) == -22, a
        e = err()
        assert e.startswith(name + ":") and all(w in e for w in words), e

    for i in (0, 2, 10, 13):                      # pg, y, dpg, loss
        a = list(ok)
        a[i] = None
        refused(a, "NULL")
    for i in (1, 11):                             # ps without dps, dps without ps
        a = list(ok)
        a[i] = None
        refused(a, "ps", "dps")
    for i, word in ((3, "B="), (4, "S="), (5, "B_global=")):
        for v in (0, -3):
            a = list(ok)
            a[i] = v
            refused(a, word + str(v))
    for kind in (-1, 4, 17):
        a = list(ok)
        a[6] = kind
        refused(a, "kind=" + str(kind))
    for delta in (0.0, -0.25, math.inf, math.nan):
        a = list(ok)
        a[6], a[9] = 3, delta
        refused(a, "HUBER", "delta")
    a = list(ok)
    a[3], a[4], a[5] = 1 << 16, 1 << 15, 1 << 16  # B * S = 2^31
    refused(a, "2^31", str(1 << 31))
    a[3] = (1 << 16) + 1
    refused(a, "2^31")


def _phonon(dtype=torch.float32):
    from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
    torch.manual_seed(0)
    return DOSTransformer_phonon(2, 1, 118, 4, 16, "cpu", 0.0).to(dtype)


def _trainers():
    from dostransformer_amd.embedder_phDOS.graphnetwork_phonon import Graphnetwork_phonon
    from dostransformer_amd.train import Trainer
    from dostransformer_amd.train64 import GraphnetworkTrainer64, Trainer64
    return [(Trainer, lambda: _phonon()), (Trainer, lambda: Graphnetwork_phonon(2, 118, 4, 16, 16, "cpu")),
            (Trainer64, lambda: _phonon(torch.float64).set_program_dtype(torch.float64)),
            (GraphnetworkTrainer64, lambda: Graphnetwork_phonon(2, 118, 4, 16, 16, "cpu").double())]


def test_trainers_refuse_unknown_losses_and_misplaced_deltas():
    from dostransformer_amd import ops
    for cls, model in _trainers():
        m = model()
        with pytest.raises(ValueError) as e:
            cls(m, loss="nope")
        assert all(k in str(e.value) for k in ops.LOSS_KINDS), e.value           # the message lists the accepted names
        with pytest.raises(ValueError, match="huber_delta"):
            cls(m, loss="mae", huber_delta=1.0)
        with pytest.raises(ValueError, match="huber_delta"):
            cls(m, huber_delta=1.0)                                              # the default loss takes none either
        with pytest.raises(ValueError, match="huber_delta"):
            cls(m, loss="huber")
        for bad in (0.0, -1.0, math.inf, math.nan):
            with pytest.raises(ValueError, match="huber_delta"):
                cls(m, loss="huber", huber_delta=bad)
        tr = cls(m, loss="huber", huber_delta=0.25)
        assert (tr.loss, tr.huber_delta, tr.crystal_losses) == ("huber", 0.25, None)
        tr = cls(m)
        assert (tr.loss, tr.huber_delta, tr.crystal_losses) == (None, None, None)
        assert "loss" not in tr.state_dict()["hyper"] and "huber_delta" not in tr.state_dict()["hyper"]


def test_trainer_refuses_loss_under_data_parallelism():
    from dostransformer_amd._lib import DosxError
    from dostransformer_amd.train import Trainer
    from tests.gpu_util import _FakeDist
    with pytest.raises(DosxError, match="single-GPU mode: not with dist"):
        Trainer(_phonon(), dist=_FakeDist(None), loss="mse")
