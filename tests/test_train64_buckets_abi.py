"""CPU-only checks of the float64 trainer's shape buckets: the padded float64 collate entry (csrc/csr.hip) is declared,
replayable and prototyped like its fp32 twin (exports, thunks, argument types: tests/test_lib_abi.py) and refuses bad descriptors
before any launch; train64.Trainer64 takes ``bucket`` /
``promote``; predict.Predictor64 takes only a float64-switched phonon module."""
import ctypes as C
import os

import pytest
import torch

from tests.util import dosx_lib as _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dosx_collate_padded_f64"


def test_collate_padded_f64_declared_exported_replayable_and_prototyped():
    _l = _lib()
    lib = _l.load()
    header = open(os.path.join(ROOT, "include", "dosx.h")).read()
    assert f"int {NAME}(const DosxCollate* d, dosx_stream_t stream);" in header
    ni, nf = C.c_int(0), C.c_int(0)
    assert lib.dosx_replay_op(NAME.encode(), C.byref(ni), C.byref(nf)) >= 0 and (ni.value, nf.value) == (2, 0)
    assert getattr(lib, NAME).argtypes == lib.dosx_collate_padded.argtypes == [C.POINTER(_l.Collate), C.c_void_p]
    # the descriptor is the fp32 entry's: its layout has not moved
    assert C.sizeof(_l.Collate) == 10 * 4 + 32 * 8 + 2 * 4 + 6 * 8 and _l.Collate.x_all.offset == 40 + 11 * 8


def _descriptor(_l):
    """A descriptor every check accepts; the addresses are never dereferenced (each call below is refused before a launch)."""
    d = _l.Collate()
    d.B, d.N, d.E, d.N_pad, d.E_pad, d.n_max, d.Fa, d.Fe, d.S, d.n_glob = 2, 5, 100, 8, 128, 3, 118, 3, 51, 0
    for k, _ in _l.Collate._fields_[10:42]:
        setattr(d, k, 4096)
    d.glob_all = d.glob = None
    return d


def test_collate_padded_f64_argument_validation_needs_no_gpu():
    _l = _lib()
    lib = _l.load()
    err = lambda: lib.dosx_last_error().decode()
    call = lambda d: lib.dosx_collate_padded_f64(C.byref(d), None)
    assert lib.dosx_collate_padded_f64(None, None) == -22 and NAME in err() and "null descriptor" in err()
    for n_pad in (5, 4):                          # N_pad < N + 1: no room for a ghost node
        d = _descriptor(_l)
        d.N_pad = n_pad
        assert call(d) == -22 and NAME in err() and "ghost" in err() and f"N_pad={n_pad}" in err()
    for k in ("x_all", "edge_feat_all", "target_all", "system_all", "sel", "node_ptr_all", "rowptr_dst_all"):
        d = _descriptor(_l)
        setattr(d, k, None)
        assert call(d) == -22 and NAME in err() and "null input" in err(), k
    for k in ("x", "edge_feat", "target", "system", "graph_ptr", "node_row", "edge_row"):
        d = _descriptor(_l)
        setattr(d, k, None)
        assert call(d) == -22 and NAME in err() and "null output" in err(), k
    d = _descriptor(_l)
    d.n_glob, d.glob_all, d.glob = 2, 4096, 4096
    assert call(d) == -22 and "n_glob" in err()
    d = _descriptor(_l)
    d.seg_tile = 4096
    assert call(d) == -22 and "seg_tile" in err()
    d = _descriptor(_l)
    d.x = 4096 + 4                                # a float-aligned address that cannot hold doubles
    assert call(d) == -22 and "8-byte aligned" in err()
    # the fp32 twin still names itself in its own refusals
    d = _descriptor(_l)
    d.N_pad = 5
    assert lib.dosx_collate_padded(C.byref(d), None) == -22 and err().startswith("dosx_collate_padded:")


def _phonon(dtype=torch.float64, attn_drop=0.0):
    from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
    torch.manual_seed(0)
    return DOSTransformer_phonon(2, 1, 118, 4, 16, "cpu", attn_drop).to(dtype)


def test_trainer64_takes_bucket_and_promote():
    from dostransformer_amd.slots import Slot
    from dostransformer_amd.train64 import Trainer64
    m64 = _phonon().set_program_dtype(torch.float64)
    tr = Trainer64(m64)
    assert tr.bucket is None and tr.promote == 0.0 and tr.slot_promoted == 0
    tr = Trainer64(m64, bucket=(8, 128), promote=0.1)
    assert tr.bucket == (8, 128) and tr.promote == 0.1 and not tr.replay
    for bad in ((8,), (0, 128), (8, 128, 1)):
        with pytest.raises(ValueError, match="bucket"):
            Trainer64(m64, bucket=bad)
    with pytest.raises(ValueError, match="promote"):
        Trainer64(m64, bucket=(8, 128), promote=-0.1)
    with pytest.raises(TypeError):
        Trainer64(m64, bucket=(8, 128), dist=None)
    with pytest.raises(TypeError):
        Trainer64(m64, bucket=(8, 128), graph=True)
    assert callable(tr.step_dataset)
    slot = Slot.empty("phonon", "cpu", torch.float64, 4, 48, 896, 19, 118, 3, 51)
    g, m = slot.g, slot.g.meta
    assert g.x.shape == (48, 118) and g.edge_vec.shape == (896, 3) and g.phdos.shape == (4, 51)
    assert all(g[k].dtype == torch.float64 for k in ("x", "edge_vec", "phdos")) and g.system.dtype == torch.int32
    assert (m.num_nodes, m.num_edges, m.num_graphs, m.n_max, m.seg_tile) == (48, 896, 4, 19, None)
    assert m.rowptr_dst.shape == (49,) and m.graph_ptr.shape == (5,) and m.inv_deg.dtype == torch.float32
    assert slot.real_nodes == 48
    slot.set_real_nodes(41)
    assert slot.real_nodes == 41 and g.real_nodes == 41


def test_predictor64_takes_only_a_float64_switched_phonon_module():
    from dostransformer_amd._lib import DosxError
    from dostransformer_amd.embedder_eDOS.DOSTransformer import DOSTransformer
    from dostransformer_amd.predict import Predictor, Predictor64
    for bad in (_phonon(torch.float32), _phonon(), DOSTransformer(2, 1, 200, 41, 2, 16, "cpu", 0.0),
                DOSTransformer(2, 1, 200, 41, 2, 16, "cpu", 0.0).double(), torch.nn.Linear(2, 2)):
        with pytest.raises(DosxError, match="Predictor64"):
            Predictor64(bad)
    m64 = _phonon().set_program_dtype(torch.float64)
    p = Predictor64(m64)
    assert p.bucket == (8, 128) and (p.slot_hits, p.slot_misses) == (0, 0) and p.eval() is p and not m64.training
    with pytest.raises(DosxError, match="float64"):
        Predictor(m64)                             # the fp32 Predictor keeps refusing a float64 module
    m64.set_program_dtype(torch.float32)           # switched back under a live Predictor64: refused at the call
    with pytest.raises(DosxError, match="Predictor64"):
        p(object())
    drop = _phonon(attn_drop=0.1).set_program_dtype(torch.float64).train()
    with pytest.raises(RuntimeError, match="eval"):
        Predictor64(drop)(object())
