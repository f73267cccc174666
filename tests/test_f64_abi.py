"""CPU-only checks of the float64 entry points (csrc/f64.hip): declared by the header, argument validation before any device
work; and the float64 dispatch decisions that need no GPU.  (That the binding matches the header - exports, struct layouts,
argument types - is tests/test_lib_abi.py's, for the whole header at once.)"""
import ctypes as C
import os

import pytest
import torch

from tests.util import dosx_lib as _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64_SYMBOLS = ["dosx_gemm_f64", "dosx_wgrad_f64", "dosx_colsum_f64", "dosx_layernorm_f64", "dosx_layernorm_bwd_f64",
               "dosx_act_bwd_f64", "dosx_edge_feat_sh1_f64", "dosx_segment_mean_f64", "dosx_segment_mean_bwd_f64",
               "dosx_gather_bwd_f64", "dosx_graph_pool_f64", "dosx_rows_add_f64", "dosx_reduce_rows_f64"]


def test_f64_symbols_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "dosx.h")).read()
    for n in F64_SYMBOLS:
        assert f"int {n}(" in header, n


def test_f64_argument_validation_needs_no_gpu():
    _l = _lib()
    lib = _l.load()
    err = lambda: lib.dosx_last_error().decode()
    fake = 4096                                   # never dereferenced: every call below is refused before any launch
    g = _l.Gemm64()
    g.M, g.N, g.K, g.nseg = 8, 16, 4, 1
    g.a[0] = _l.Seg64(fake, 4, 3, _l.RowMap(_l.BIG, 0, 1, 0, None))
    g.w, g.ldw, g.out, g.ldo = fake, 4, fake, 16
    assert lib.dosx_gemm_f64(C.byref(g), None) != 0 and "K=4" in err()
    g.a[0].width = 4
    g.act = 3
    assert lib.dosx_gemm_f64(C.byref(g), None) != 0 and "alpha" in err()
    g.act, g.w_layout = 0, 2
    assert lib.dosx_gemm_f64(C.byref(g), None) != 0 and "w_layout" in err()
    assert lib.dosx_gemm_f64(None, None) != 0 and "NULL" in err()
    w = _l.Wgrad64()
    w.M, w.N, w.K, w.nseg, w.nsplit = 600, 16, 4, 1, 3
    w.x[0] = _l.Seg64(fake, 4, 4, _l.RowMap(_l.BIG, 0, 1, 0, None))
    w.dy, w.lddy, w.dw, w.ldd = fake, 16, fake, 4
    assert lib.dosx_wgrad_f64(C.byref(w), None) != 0 and "partials" in err()
    assert lib.dosx_colsum_f64(fake, 1000, 8, 8, None, fake, 0, None) != 0 and "partials" in err()
    assert lib.dosx_layernorm_f64(fake, fake, fake, None, fake, fake, fake, 4, 2048, None) != 0 and "W=2048" in err()
    assert lib.dosx_act_bwd_f64(fake, fake, 8, 3, None, fake, None, 4, 8, None) != 0 and "PReLU" in err()
    assert lib.dosx_gather_bwd_f64(fake, 8, fake, fake, fake, None, 0, None, 0, fake, 4, 8, None) != 0 and "ldc" in err()
    assert lib.dosx_edge_feat_sh1_f64(fake, fake, 4, 0.0, None) != 0 and "r_max" in err()


def _phonon_models(dtype):
    from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
    from dostransformer_amd.embedder_phDOS.graphnetwork_phonon import Graphnetwork_phonon
    torch.manual_seed(0)
    return (DOSTransformer_phonon(2, 1, 118, 4, 16, "cpu", 0.0).to(dtype), Graphnetwork_phonon(2, 118, 4, 16, 51, "cpu").to(dtype))


def test_f64_dispatch_decisions():
    """Which modules run the float64 program, and which float64 modules are refused (DosxError, never a silent fp32 run).
    Modules without a float64 program keep their fp32 computation, as before."""
    from dostransformer_amd._lib import DosxError
    from dostransformer_amd.embedder_eDOS.DOSTransformer import DOSTransformer
    from dostransformer_amd.embedder_eDOS.graphnetwork import Graphnetwork
    from dostransformer_amd.predict import Predictor
    from dostransformer_amd.train import Trainer
    dt, gn = _phonon_models(torch.float64)
    assert gn._flat_dtype() == torch.float64
    dt32, gn32 = _phonon_models(torch.float32)
    assert gn32._flat_dtype() == torch.float32 and dt32._flat_dtype() == torch.float32
    # DOSTransformer_phonon has no float64 program: a float64 one stays on the fp32 path, and its drivers accept it
    assert dt._flat_dtype() == torch.float32
    Trainer(dt)
    Predictor(dt)
    gn.out_layer[2].float()                       # mixed live dtypes
    with pytest.raises(DosxError, match="mix"):
        gn._flat_dtype()
    ed = DOSTransformer(2, 1, 200, 41, 2, 16, "cpu", 0.0).double()
    assert ed._flat_dtype() == torch.float32      # eDOS: fp32 computation whatever the module dtype, as before
    assert Graphnetwork(2, 200, 41, 2, 16, 201, "cpu").double()._flat_dtype() == torch.float32
    from dostransformer_amd.embedder_phDOS.graphnetwork_phonon import Graphnetwork_phonon
    with pytest.raises(DosxError, match="hidden"):
        Graphnetwork_phonon(1, 118, 4, 520, 51, "cpu").double()._flat_dtype()
