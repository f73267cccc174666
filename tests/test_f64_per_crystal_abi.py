"""CPU-only checks of the per-crystal key counts of the float64 attention (DosxAttn64.key_ptr) and of the module switch that
uses them (DOSTransformerBase.set_per_crystal_keys): DosxAttn64 has key_ptr behind accumulate (its C layout is checked field by
field in tests/test_lib_abi.py), and the switch belongs to the float64 program of DOSTransformer_phonon alone."""
import pytest
import torch

from tests.util import dosx_lib as _lib


def test_attn64_key_ptr_matches_c_layout():
    _l = _lib()
    fields = [f for f, _ in _l.Attn64._fields_]
    assert "key_ptr" in fields
    assert fields[-2:] == ["accumulate", "key_ptr"]                 # appended: every earlier offset stays
    assert max(getattr(_l.Attn64, f).offset for f in fields) == _l.Attn64.key_ptr.offset > _l.Attn64.accumulate.offset
    assert _l.Attn64().key_ptr is None                              # default: today's behaviour


def test_attention64_signatures_take_key_ptr_last():
    import inspect
    from dostransformer_amd import ops
    fwd = list(inspect.signature(ops.attention64).parameters)
    bwd = list(inspect.signature(ops.attention_bwd64).parameters)
    assert fwd[-3:] == ["mask", "softmax64", "key_ptr"]
    assert bwd[-4:] == ["mask", "softmax64", "accumulate", "key_ptr"]
    assert inspect.signature(ops.attention64).parameters["key_ptr"].default is None
    assert inspect.signature(ops.attention_bwd64).parameters["key_ptr"].default is None


def _phonon(dtype=torch.float64):
    from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
    torch.manual_seed(0)
    return DOSTransformer_phonon(2, 1, 118, 4, 16, "cpu", 0.0).to(dtype)


def test_set_per_crystal_keys_belongs_to_the_float64_program():
    from dostransformer_amd._lib import DosxError
    from dostransformer_amd.embedder_eDOS.DOSTransformer import DOSTransformer
    from dostransformer_amd.predict import Predictor
    from dostransformer_amd.train import Trainer
    m = _phonon().set_program_dtype(torch.float64)
    assert m.per_crystal_keys is False
    assert m.set_per_crystal_keys(True) is m
    assert m.per_crystal_keys is True
    with pytest.raises(AttributeError):
        m.per_crystal_keys = False                                   # read-only
    for drv in (Trainer, Predictor):                                 # the fp32 drivers still refuse a float64 module
        with pytest.raises(DosxError, match="loss.backward"):
            drv(m)
    assert m.set_per_crystal_keys(False) is m and m.per_crystal_keys is False
    m.set_per_crystal_keys(True)
    m.set_program_dtype(torch.float64)                               # staying float64 keeps it
    assert m.per_crystal_keys is True
    m.set_program_dtype(torch.float32)                               # the fp32 program has no such switch: cleared
    assert m.per_crystal_keys is False and m.program_dtype == torch.float32
    with pytest.raises(DosxError, match="Predictor"):
        m.set_per_crystal_keys(True)
    assert m.set_per_crystal_keys(False) is m                        # clearing is always allowed
    with pytest.raises(DosxError, match="Predictor"):
        _phonon(dtype=torch.float32).set_per_crystal_keys(True)
    with pytest.raises(DosxError, match="Predictor"):
        _phonon().set_per_crystal_keys(True)                         # float64 parameters, fp32 program
    edos = DOSTransformer(2, 1, 200, 41, 2, 16, "cpu", 0.0).double()
    with pytest.raises(DosxError):
        edos.set_per_crystal_keys(True)
    assert edos.per_crystal_keys is False
