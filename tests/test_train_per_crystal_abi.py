"""Per-crystal keys of the fp32 trainer, the parts a machine without a GPU can check: DosxFfnBwd ends in att_key_ptr (its C
layout and field order are checked against the header in tests/test_lib_abi.py), Trainer(per_crystal_keys=...) as an interface,
and that model.set_per_crystal_keys stays the float64 program's switch."""
import pytest
import torch


def test_ffn_bwd_mirror_has_the_c_layout_with_att_key_ptr_last():
    from dostransformer_amd import _lib
    names = [n for n, _ in _lib.FfnBwd._fields_]
    assert names[-1] == "att_key_ptr"
    assert max(getattr(_lib.FfnBwd, n).offset for n in names) == _lib.FfnBwd.att_key_ptr.offset


def _cpu_model():
    from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
    return DOSTransformer_phonon(2, 1, 118, 4, 16, "cpu", 0.0)


def test_trainer_flag_is_a_read_only_attribute():
    from dostransformer_amd.train import Trainer
    model = _cpu_model()
    assert Trainer(model).per_crystal_keys is False
    tr = Trainer(model, per_crystal_keys=True)
    assert tr.per_crystal_keys is True
    with pytest.raises(AttributeError):
        tr.per_crystal_keys = False
    assert tr.per_crystal_keys is True


def test_trainer_refuses_the_flag_under_data_parallelism():
    from dostransformer_amd._lib import DosxError
    from dostransformer_amd.train import Trainer

    class _Dist:
        world, rank = 2, 0

    with pytest.raises(DosxError, match="per_crystal_keys"):
        Trainer(_cpu_model(), dist=_Dist(), per_crystal_keys=True)
    assert Trainer(_cpu_model(), dist=_Dist()).per_crystal_keys is False       # (the flag off: as before)


def test_set_per_crystal_keys_still_belongs_to_the_float64_program():
    from dostransformer_amd._lib import DosxError
    model = _cpu_model()
    with pytest.raises(DosxError):
        model.set_per_crystal_keys(True)
    assert model.per_crystal_keys is False
