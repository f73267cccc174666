"""CPU-only checks of the gradient-accumulation entries (csrc/grad_accumulate.hip: dosx_grad_accumulate / _f64) and of what the
trainers' ``step_accumulate`` / ``step_dataset_accumulate`` refuse without running a program: declared, exported, replayable,
prototyped with operands of their own type; every refusal of include/dosx.h comes back as -22 with a message that starts with
the entry's name, before any launch (fake pointers, never dereferenced); n == 0 is a no-op; an empty window, ``dist`` and more
than one batch on the reference's pooled phonon loss raise on a CPU model, which launches nothing."""
import ctypes as C
import os
import re

import pytest
import torch

from tests.util import dosx_lib as _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"dosx_grad_accumulate": "float", "dosx_grad_accumulate_f64": "double"}
FAKE = 1 << 20                                    # 16-byte aligned, never dereferenced: every call below is refused or a no-op
N = 1000                                          # elements: the vectors [FAKE + k * STEP, + N * 8) do not touch
STEP = 1 << 16


def test_symbols_declared_exported_replayable_and_prototyped():
    _l = _lib()
    lib = _l.load()
    header = open(os.path.join(ROOT, "include", "dosx.h")).read()
    for n, t in SYMBOLS.items():
        assert f"int {n}(" in header, n
        proto = re.search(r"int " + n + r"\(([^;]*)\);", header).group(1)
        assert proto.count(t + "*") == 6 and proto.count(("double" if t == "float" else "float") + "*") == 0, proto
        assert hasattr(lib, n), n
        ni, nf = C.c_int(0), C.c_int(0)
        assert lib.dosx_replay_op(n.encode(), C.byref(ni), C.byref(nf)) >= 0, n
        args = getattr(lib, n).argtypes
        assert len(args) == 8 and (ni.value, nf.value) == (8, 0), n
        assert _l._SIGS[n].count(C.c_int64) == 1 and _l._SIGS[n].count(C.c_void_p) == 7, n      # n; six operands and the stream
    from dostransformer_amd import _abi, ops
    assert (_abi.DOSX_ACCUM_THREADS, _abi.DOSX_ACCUM_MAX_BLOCKS) == (256, 2048)
    assert callable(ops.grad_accumulate) and callable(ops.grad_accumulate64)


@pytest.mark.parametrize("name", list(SYMBOLS))
def test_argument_validation_needs_no_gpu(name):
    lib = _lib().load()
    fn = getattr(lib, name)
    size = 4 if name == "dosx_grad_accumulate" else 8
    D, A, B, SD, SA, SB = (FAKE + k * STEP for k in range(6))
    # dst, a, b, n, sdst, sa, sb
    ok = [D, A, B, N, SD, SA, SB]

    def refused(a, *words):
        assert fn(*a, None) == -22, a
        e = lib.dosx_last_error().decode()
        assert e.startswith(name + ":") and all(w in e for w in words), e

    def with_(**kw):
        a = list(ok)
        for k, v in kw.items():
            a["dst a b n sdst sa sb".split().index(k)] = v
        return a

    refused(with_(dst=None), "NULL")
    refused(with_(a=None), "NULL")
    refused(with_(dst=None, a=None, b=None, sdst=None, sa=None, sb=None), "NULL")
    for n in (-1, -(1 << 40)):
        refused(with_(n=n), "negative", str(n))
    for k in ("dst", "a", "b"):
        for off in (4, 8):
            refused(with_(**{k: ok["dst a b".split().index(k)] + off}), "16-byte")
    # partial overlaps of dst with a and with b, from either side; the same with b == NULL for a
    for shift in (16, -16, (N - 1) * size // 16 * 16):
        refused(with_(a=D + shift), "overlaps a")
        refused(with_(a=D + shift, b=None), "overlaps a")
        refused(with_(b=D + shift), "overlaps b")
    refused(with_(sa=None), "sdst", "sa")
    refused(with_(sdst=None), "sdst", "sa")
    refused(with_(sdst=None, sa=None), "sb")
    refused(with_(sdst=D + 16 * 3), "inside dst")
    refused(with_(sb=D), "inside dst")
    refused(with_(sdst=A + 32), "inside a")
    refused(with_(sdst=SD + size // 2), "aligned")
    # a refusal comes before the n == 0 return
    refused(with_(n=0, dst=None), "NULL")
    # n == 0: a no-op without a launch, in every form - dst apart, dst == a, dst == b, copy, with and without the scalars
    for a in (with_(n=0), with_(n=0, a=D), with_(n=0, b=D), with_(n=0, b=None), with_(n=0, sdst=None, sa=None, sb=None),
              with_(n=0, b=None, sb=None)):
        assert fn(*a, None) == 0, a


# ---- the trainers: what a window refuses before any program runs -----------------------------------------------------------------
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


def _batches(k, dtype=torch.float32):
    from dostransformer_amd import synth
    return [synth.phonon_batch(2, seed=5 + i, dtype=dtype) for i in range(k)]


def _untouched(tr):
    return tr.step_count == 0 and tr._fp is None and tr._acc is None and tr._window_total is None and len(tr._slots) == 0 \
        and getattr(tr.model, "_drop_seed", None) is None


def test_every_trainer_has_both_window_entries_and_refuses_an_empty_window():
    for cls, model in _trainers():
        tr = cls(model(), loss="mse")
        for call in (lambda: tr.step_accumulate([]), lambda: tr.step_accumulate(iter(())),
                     lambda: tr.step_dataset_accumulate(None, [])):
            with pytest.raises(ValueError, match="empty window"):
                call()
        with pytest.raises(ValueError, match="batch 1 of the window is empty"):
            tr.step_dataset_accumulate(None, [[0, 1], []])
        assert _untouched(tr)


def test_more_than_one_batch_on_the_pooled_phonon_loss_is_refused_by_name():
    from dostransformer_amd._lib import DosxError
    for cls, model in _trainers():
        tr = cls(model())
        with pytest.raises(DosxError, match='loss="crystal_rmse"'):
            tr.step_accumulate(_batches(2))
        with pytest.raises(DosxError, match='loss="crystal_rmse"'):
            tr.step_dataset_accumulate(None, [[0, 1], [2]])
        assert _untouched(tr)


def test_window_under_data_parallelism_is_refused():
    from dostransformer_amd._lib import DosxError
    from dostransformer_amd.embedder_eDOS.DOSTransformer import DOSTransformer
    from dostransformer_amd.train import Trainer
    from tests.gpu_util import _FakeDist
    torch.manual_seed(0)
    for model in (_phonon(), DOSTransformer(2, 1, 200, 41, 2, 16, "cpu", 0.0)):
        tr = Trainer(model, dist=_FakeDist(None))
        for k in (1, 2):
            with pytest.raises(DosxError, match="single-GPU mode: not with dist"):
                tr.step_accumulate(_batches(k))
            with pytest.raises(DosxError, match="single-GPU mode: not with dist"):
                tr.step_dataset_accumulate(None, [[0]] * k)
        assert _untouched(tr)


def test_the_public_refusals_of_a_foreign_count_stand():
    """The window's total travels on an internal route: outside a window n_global must still be the batch's own count."""
    from dostransformer_amd.train import Trainer
    tr = Trainer(_phonon(), loss="mse")
    assert tr._window_total is None
    assert tr._whole_or_window(4, 4) and not tr._whole_or_window(4, 5)
    with pytest.raises(ValueError, match="n_global"):
        tr._require_whole_batch(4, 5)
    tr._window_total = 9
    try:
        assert tr._whole_or_window(4, 9) and not tr._whole_or_window(4, 5)
    finally:
        tr._window_total = None
