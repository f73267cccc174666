"""CPU-only checks of the Electron-DOS graph builder's boundary: dosx_knn_graph (csrc/knn.hip) is declared, replayable and
prototyped; DosxKnn has the size and field order its contract states (exports, thunks, argument types and the C layout field by
field: tests/test_lib_abi.py, for the whole header); every bad descriptor is refused before any launch; and the
host side of featurize.build_edos_all (element table, device check, synthetic structures) behaves."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests.util import dosx_lib as _lib, in_all_three_builds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "dosx_knn_graph"
POINTERS = ("pos", "cell", "atom_ptr", "centers", "nbr_idx", "nbr_shift", "nbr_dist", "nbr_count", "edge_attr")


def test_knn_graph_declared_exported_replayable_and_prototyped():
    _l = _lib()
    lib = _l.load()
    header = open(os.path.join(ROOT, "include", "dosx.h")).read()
    thunks = open(os.path.join(ROOT, "dostransformer_amd", "csrc", "replay_thunks.inc")).read()
    assert f"int {NAME}(const DosxKnn* d, dosx_stream_t stream);" in header
    assert f'{{"{NAME}", thunk_{NAME}, 2, 0}}' in thunks
    ni, nf = C.c_int(0), C.c_int(0)
    assert lib.dosx_replay_op(NAME.encode(), C.byref(ni), C.byref(nf)) >= 0 and (ni.value, nf.value) == (2, 0)
    assert getattr(lib, NAME).argtypes == [C.POINTER(_l.Knn), C.c_void_p]
    assert in_all_three_builds("knn.hip")                 # libdosx.so and the two diagnostic builds


def test_knn_descriptor_matches_c_layout():
    _l = _lib()
    fields = [k for k, _ in _l.Knn._fields_]
    assert C.sizeof(_l.Knn) == 6 * 4 + 4 * 8 + 9 * 8
    assert fields == ["C", "N", "K", "G", "pbc_mask", "reserved", "radius", "tol", "pad_dist", "var"] + list(POINTERS)


def _descriptor(_l):
    """A descriptor every check accepts; the addresses are never dereferenced (each call below is refused before a launch)."""
    d = _l.Knn()
    d.C, d.N, d.K, d.G, d.pbc_mask = 3, 40, 12, 41, 7
    d.radius, d.tol, d.pad_dist, d.var = 8.0, 1e-8, 9.0, 0.2
    for i, k in enumerate(POINTERS):
        setattr(d, k, 0x10000 * (i + 1))
    return d


def test_knn_graph_argument_validation_needs_no_gpu():
    _l = _lib()
    lib = _l.load()
    err = lambda: lib.dosx_last_error().decode()

    def refused(d, word=""):
        assert lib.dosx_knn_graph(C.byref(d), None) == -22
        assert NAME in err() and word in err(), err()

    assert lib.dosx_knn_graph(None, None) == -22 and NAME in err() and "null descriptor" in err()
    for field, bad, word in (("C", 0, "C=0"), ("C", -2, "C=-2"), ("N", -1, "N=-1"), ("K", 0, "K=0"), ("K", 17, "K=17"),
                             ("K", -3, "K=-3"), ("radius", 0.0, "radius"), ("radius", -8.0, "radius"), ("tol", -1e-8, "tol"),
                             ("G", 0, "G=0"), ("G", -41, "G=-41"), ("var", 0.0, "var"), ("var", -0.2, "var")):
        d = _descriptor(_l)
        setattr(d, field, bad)
        refused(d, word)
    for k in ("pos", "cell", "atom_ptr"):
        d = _descriptor(_l)
        setattr(d, k, None)
        refused(d, "null input")
    for k in ("nbr_idx", "nbr_shift", "nbr_dist", "nbr_count"):
        d = _descriptor(_l)
        setattr(d, k, None)
        refused(d, "null output")
    d = _descriptor(_l)
    d.centers = None
    refused(d, "null centers")
    d = _descriptor(_l)
    d.N, d.K = 1 << 27, 16                                     # N*K = 2^31: past the 32-bit edge index
    refused(d, "N*K")
    # without edge_attr the feature fields are ignored, and N == 0 returns before any launch
    d = _descriptor(_l)
    d.N, d.edge_attr, d.centers, d.G, d.var = 0, None, None, 0, 0.0
    assert lib.dosx_knn_graph(C.byref(d), None) == 0
    d = _descriptor(_l)
    d.N = 0
    assert lib.dosx_knn_graph(C.byref(d), None) == 0


def test_load_elem_feats_standardises_like_sklearn_scale(tmp_path):
    from dostransformer_amd import featurize
    rng = np.random.default_rng(0)
    raw = rng.normal(size=(100, 7)) * rng.uniform(0.1, 30.0, 7) + rng.uniform(-5, 5, 7)
    raw[:, 3] = 2.5                                            # a zero-variance column: divided by 1, so it becomes 0
    table = {s: raw[i].tolist() for i, s in enumerate(featurize.SYMBOLS[:100])}
    table["Og"] = [0.0] * 7                                    # elements past the first hundred are not read
    path = tmp_path / "embedding.json"
    path.write_text(json.dumps(table))
    ref = raw - raw.mean(axis=0)
    std = raw.std(axis=0)
    std[3] = 1.0
    ref = ref / std
    for src in (str(path), table):
        got = featurize.load_elem_feats(src)
        assert got.shape == (100, 7) and got.dtype == np.float64
        assert np.array_equal(got, ref) and np.all(got[:, 3] == 0.0)
        assert np.allclose(got.mean(axis=0), 0.0, atol=1e-12) and np.allclose(np.delete(got.std(axis=0), 3), 1.0)
    assert featurize.load_elem_feats(table, symbols=("H", "O", "Fe")).shape == (3, 7)
    del table["Fe"]
    with pytest.raises(ValueError, match="Fe"):
        featurize.load_elem_feats(table)


def test_build_edos_all_has_no_cpu_fallback_and_structures_are_seeded():
    from dostransformer_amd import featurize, synth
    a, b, c = synth.edos_structures(5, seed=7), synth.edos_structures(5, seed=7), synth.edos_structures(5, seed=8)
    assert len(a) == 5
    for x, y in zip(a, b):
        assert set(x) == {"numbers", "positions", "cell", "glob", "crystal_system", "y_ft", "mp_id"}
        assert all(np.array_equal(x[k], y[k]) for k in ("numbers", "positions", "cell", "glob", "y_ft"))
        assert x["crystal_system"] == y["crystal_system"] and x["mp_id"] == y["mp_id"]
        n = len(x["numbers"])
        assert 2 <= n <= 40 and x["positions"].shape == (n, 3) and x["cell"].shape == (3, 3) and x["y_ft"].shape == (201,)
        assert x["numbers"].min() >= 1 and x["numbers"].max() <= 100 and abs(np.linalg.det(x["cell"])) > 1.0
    assert not np.array_equal(a[0]["cell"], c[0]["cell"])
    table = np.zeros((100, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        featurize.build_edos_all(a, table, device="cpu")
    assert callable(__import__("dostransformer_amd.ops", fromlist=["knn_graph"]).knn_graph)
