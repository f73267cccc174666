"""CPU-only checks of the float64 attention entry points (csrc/f64_attention.hip) and of the program switch of
DOSTransformer_phonon (set_program_dtype): declared by the header, arguments are refused before any launch, and which modules
run which program.  (Exports, thunks, the DosxAttn64 layout and its constants: tests/test_lib_abi.py, for the whole header.)"""
import ctypes as C
import os

import pytest
import torch

from tests.util import dosx_lib as _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["dosx_attention_f64", "dosx_attention_bwd_f64", "dosx_dense_rows_f64", "dosx_dense_rows_bwd_f64",
           "dosx_index_sum_f64"]


def test_attention_f64_symbols_declared_exported_and_replayable():
    header = open(os.path.join(ROOT, "include", "dosx.h")).read()
    for n in SYMBOLS:
        assert f"int {n}(" in header, n                  # `int`: replayable (every such entry has a thunk, test_lib_abi.py)


def test_attention_f64_argument_validation_needs_no_gpu():
    _l = _lib()
    lib = _l.load()
    err = lambda: lib.dosx_last_error().decode()
    fake = 4096                                   # never dereferenced: every call below is refused before any launch

    def desc(**kw):
        d = _l.Attn64()
        d.Sq, d.Bq, d.Nk, d.Bk, d.H = 51, 4, 9, 2, 64
        for f in ("q", "x", "kvhat", "gamma0", "beta0", "out", "probs", "dout", "dq", "ds", "dkvhat", "part"):
            setattr(d, f, fake)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    for fn in (lib.dosx_attention_f64, lib.dosx_attention_bwd_f64):
        for kw, msg in [(dict(H=0), "H=0"), (dict(H=513), "H=513"), (dict(Nk=0), "Nk=0"), (dict(Bq=5), "multiple"),
                        (dict(q=None), "NULL"), (dict(kvhat=None), "NULL"), (dict(probs=None), "NULL"), (dict(flags=4), "flags")]:
            assert fn(C.byref(desc(**kw)), None) != 0, kw
            assert msg in err(), (kw, err())
        assert fn(None, None) != 0 and "NULL" in err()
    assert lib.dosx_attention_f64(C.byref(desc(out=None)), None) != 0 and "NULL" in err()
    assert lib.dosx_attention_bwd_f64(C.byref(desc(ds=None)), None) != 0 and "NULL" in err()
    assert lib.dosx_attention_bwd_f64(C.byref(desc(part=None)), None) != 0 and "NULL" in err()
    assert lib.dosx_dense_rows_f64(fake, None, fake, fake, 2, 4, 16, None) != 0 and "NULL" in err()
    assert lib.dosx_dense_rows_f64(fake, fake, fake, fake, 2, 4, 2048, None) != 0 and "H=2048" in err()
    assert lib.dosx_dense_rows_bwd_f64(fake, fake, fake, fake, fake, 2, 0, 16, 1, None) != 0 and "nmax=0" in err()
    assert lib.dosx_index_sum_f64(fake, 8, None, 3, fake, 8, 7, 8, 0, None) != 0 and "NULL" in err()
    assert lib.dosx_index_sum_f64(fake, 4, fake, 3, fake, 8, 7, 8, 0, None) != 0 and "ld_src=4" in err()


def _phonon(H=16, dtype=torch.float64):
    from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
    torch.manual_seed(0)
    return DOSTransformer_phonon(2, 1, 118, 4, H, "cpu", 0.0).to(dtype)


def test_dostransformer_phonon_program_switch():
    """Opt-in float64 program: an un-switched float64 module still runs fp32; a switched one runs (and re-homes its flat
    parameters in) float64; fp32, mixed, eDOS and hidden-520 modules and other dtypes are refused at the call; the fp32
    drivers refuse a switched module; switching back restores the fp32 program."""
    from dostransformer_amd._lib import DosxError
    from dostransformer_amd.embedder_eDOS.DOSTransformer import DOSTransformer
    from dostransformer_amd.predict import Predictor
    from dostransformer_amd.train import Trainer
    m = _phonon()
    assert m.program_dtype == torch.float32 and m._flat_dtype() == torch.float32
    assert m.set_program_dtype(torch.float64) is m
    assert m.program_dtype == torch.float64 and m._flat_dtype() == torch.float64
    fp = m.flat_params()
    assert fp.dtype == torch.float64 and m.embeddings.weight.dtype == torch.float64
    assert all(p.dtype == torch.float64 for p in m.state_dict().values() if p.is_floating_point())
    for drv in (Trainer, Predictor):
        with pytest.raises(DosxError, match="loss.backward"):
            drv(m)
    with pytest.raises(DosxError):
        m.set_program_dtype(torch.float16)
    assert m.program_dtype == torch.float64
    m.set_program_dtype(torch.float32)
    assert m.program_dtype == torch.float32 and m.flat_params().dtype == torch.float32
    Trainer(m)
    Predictor(m)
    with pytest.raises(DosxError, match="float64"):
        _phonon(dtype=torch.float32).set_program_dtype(torch.float64)
    mixed = _phonon()
    mixed.out_layer.float()
    with pytest.raises(DosxError, match="float64"):
        mixed.set_program_dtype(torch.float64)
    ok = _phonon().set_program_dtype(torch.float64)
    ok.fc.float()                                  # the re-homing call checks again
    with pytest.raises(DosxError):
        ok.flat_params()
    with pytest.raises(DosxError, match="hidden"):
        _phonon(H=520).set_program_dtype(torch.float64)
    with pytest.raises(DosxError, match="DOSTransformer_phonon"):
        DOSTransformer(2, 1, 200, 41, 2, 16, "cpu", 0.0).double().set_program_dtype(torch.float64)
