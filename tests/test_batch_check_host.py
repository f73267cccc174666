"""CPU-only checks of batch validation (dostransformer_amd/validate.py, csrc/validate.hip): the numpy twin of dosx_batch_check
against reports worked out by hand on a 3-crystal batch (tests/batch_check_cases.py), the text of the error, the process-wide
switch and its hooks in collate() / DeviceDataset, and the C boundary of the new entry points - exported, replayable, and refusing
bad arguments on the host with -22 before anything touches a device."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import batch_check_cases as cases
from tests.util import in_all_three_builds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host(b, **kw):
    from dostransformer_amd import validate
    return validate.check_batch_host(b["edge_index"], b["batch"], b["system"], b["num_graphs"], **kw)


def _as_batch(b):
    from dostransformer_amd.batch import CrystalBatch
    f = {"edge_index": torch.from_numpy(b["edge_index"]), "batch": torch.from_numpy(b["batch"])}
    if b["system"] is not None:
        f["system"] = torch.from_numpy(b["system"])
    return CrystalBatch(f, b["num_graphs"])


@pytest.mark.parametrize("name", [c[0] for c in cases.CASES])
def test_host_twin_reports_each_rule_at_its_first_last_and_twice(name):
    b, kw, want = cases.corrupted(name)
    got = _host(b, **kw)
    assert got.dtype == np.int32 and got.tolist() == cases.expected_words(want).tolist(), (name, got.tolist())


def test_host_twin_r6_at_the_first_crystal_and_degenerate_sizes():
    sizes, kw, want = cases.CASE_R6_FIRST
    assert _host(cases.small_batch(sizes), **kw).tolist() == cases.expected_words(want).tolist()
    clean = cases.expected_words({}).tolist()
    # E = 0: three crystals without any edge
    b = cases.small_batch()
    b["edge_index"] = np.zeros((2, 0), np.int64)
    assert _host(b, require_sorted=True).tolist() == clean
    # B = 1: one crystal, one atom, its self edge
    one = {"edge_index": np.zeros((2, 1), np.int64), "batch": np.zeros(1, np.int64), "system": np.asarray([6]), "num_graphs": 1}
    assert _host(one, require_sorted=True, n_max=1).tolist() == clean
    one["system"] = np.asarray([7])
    assert _host(one).tolist() == cases.expected_words({5: (1, 0)}).tolist()
    # nothing at all
    none = {"edge_index": np.zeros((2, 0), np.int64), "batch": np.zeros(0, np.int64), "system": None, "num_graphs": 0}
    assert _host(none).tolist() == clean


def test_check_batch_on_cpu_tensors_is_the_twin_and_names_rule_index_and_value():
    from dostransformer_amd import validate
    from dostransformer_amd._lib import DosxError
    b, kw, want = cases.corrupted("clean")
    rep = validate.check_batch(_as_batch(b), require_sorted=True, n_max=3)
    assert rep.ok and rep.words.tolist() == cases.expected_words({}).tolist() and "clean" in repr(rep)
    texts = {
        "R1-twice": ["R1", "2 violations", "edge 2: source 6 outside [0, 6)"],
        "R1-last": ["R1", "1 violation;", "edge 6: destination 6 outside [0, 6)"],
        "R2-first": ["R2", "edge 0: source 2 is in crystal 1, destination 0 in crystal 0"],
        "R3-last": ["R3", "node 5: batch 3 outside [0, 3)"],
        "R3-twice": ["R3", "2 violations", "node 3: batch 0 below batch 1 of node 2", "R2", "edge 4"],
        "R4-last": ["R4", "crystal 2: owns no node"],
        "R5-first": ["R5", "crystal 0: system 7 outside [0, 7)"],
        "R6-last": ["R6", "crystal 2: 3 atoms, n_max 2"],
        "R7-last": ["R7", "edge 6: destination 4 below destination 5 of edge 5"],
    }
    for name, parts in texts.items():
        b, kw, want = cases.corrupted(name)
        g = _as_batch(b)
        rep = validate.check_batch(g, raise_=False, **kw)
        assert not rep.ok and rep.words.tolist() == cases.expected_words(want).tolist(), name
        with pytest.raises(DosxError) as e:
            validate.check_batch(g, **kw)
        for p in parts:
            assert p in str(e.value), (name, p, str(e.value))


def test_finite_check_of_cpu_fields():
    from dostransformer_amd import synth, validate
    from dostransformer_amd._lib import DosxError
    g = synth.phonon_batch(3, 0, dtype=torch.float32)
    rep = validate.check_batch(g, finite=True, require_sorted=True)
    assert rep.ok and rep.fields == ("x", "edge_vec", "phdos")
    g.edge_vec[2, 1] = float("inf")
    g.edge_vec[4, 0] = float("nan")
    rep = validate.check_batch(g, finite=True, raise_=False)
    assert rep.nonfinite("edge_vec") == (2, 7) and rep.nonfinite("x") == (0, cases.INT32_MAX)
    assert validate.check_batch(g).ok                                    # not asked for: not looked at
    with pytest.raises(DosxError, match=r"edge_vec: 2 non-finite elements; first: element 7 = inf"):
        validate.check_batch(g, finite=True)


def test_switch_is_off_by_default_and_guards_collate_and_device_dataset():
    from dostransformer_amd import synth, validate
    from dostransformer_amd._lib import DosxError
    from dostransformer_amd.batch import collate
    assert validate.ENABLED is False and validate.FINITE is False
    gen = torch.Generator().manual_seed(3)
    crystals = [synth.phonon_crystal(gen, n_atoms=n, n_out=3, dtype=torch.float32) for n in (2, 4, 3)]
    good = collate(crystals)
    bad = [dict(c) for c in crystals]
    bad[1]["edge_index"] = bad[1]["edge_index"].clone()
    bad[1]["edge_index"][0, 5] = 4                      # a local id equal to the crystal's atom count: global node 6, crystal 2's first
    try:
        validate.enable()
        assert validate.ENABLED and not validate.FINITE
        again = collate(crystals)                       # a valid batch: the same result with the switch on
        assert all(torch.equal(again[k], good[k]) for k in ("x", "edge_index", "batch", "edge_vec", "system", "phdos"))
        with pytest.raises(DosxError, match=r"R2 .*edge 11: source 6 is in crystal 2, destination \d in crystal 1"):
            collate(bad)
        last = [dict(c) for c in crystals]
        last[2]["edge_index"] = last[2]["edge_index"].clone()
        last[2]["edge_index"][1, 0] = 3                 # the last crystal: one past the whole batch
        with pytest.raises(DosxError, match=r"R1 .*edge \d+: destination 9 outside \[0, 9\)"):
            collate(last)
        seven = [dict(c) for c in crystals]
        seven[0]["system"] = torch.tensor(7)
        with pytest.raises(DosxError, match=r"crystal 0: system 7 outside \[0, 7\)"):
            collate(seven)
        validate.enable(True, finite=True)
        nan = [dict(c) for c in crystals]
        nan[1]["x"] = nan[1]["x"].clone()
        nan[1]["x"][0, 0] = float("nan")
        with pytest.raises(DosxError, match=r"x: 1 non-finite element; first: element 236 = nan"):
            collate(nan)
        # DeviceDataset checks each crystal's LOCAL arrays before it derives anything (raises before any device is touched)
        from dostransformer_amd.loader import DeviceDataset
        with pytest.raises(DosxError, match=r"crystal 1 of the dataset: .*R1 .*edge 5: source 4 outside \[0, 4\)"):
            DeviceDataset(bad, "cpu")
    finally:
        validate.enable(False)
    assert validate.ENABLED is False and validate.FINITE is False
    collate(seven)                                      # off again: nothing is looked at


def test_graph_meta_checks_a_foreign_host_batch_once_when_the_switch_is_on():
    import types
    from dostransformer_amd import validate
    from dostransformer_amd._lib import DosxError
    from dostransformer_amd.batch import graph_meta
    b, _, _ = cases.corrupted("R5-first")
    mk = lambda d: types.SimpleNamespace(edge_index=torch.from_numpy(d["edge_index"]), batch=torch.from_numpy(d["batch"]),
                                         system=torch.from_numpy(d["system"]))
    assert graph_meta(mk(b)).num_graphs == 3            # off: metadata is derived from whatever is there
    try:
        validate.enable()
        with pytest.raises(DosxError, match="system 7"):
            graph_meta(mk(b))
        ok = mk(cases.small_batch())
        m = graph_meta(ok)
        ok.system[0] = 7                                # metadata is cached on the object: it is not derived, hence not checked, again
        assert graph_meta(ok) is m
    finally:
        validate.enable(False)


def test_new_entry_points_are_exported_replayable_and_refuse_bad_arguments_on_the_host():
    from tests.util import dosx_lib
    _lib = dosx_lib()
    lib = _lib.load()
    names = ("dosx_batch_check", "dosx_finite_check_f32", "dosx_finite_check_f64", "dosx_exchange_status", "dosx_exchange_selftest")
    thunks = open(os.path.join(ROOT, "dostransformer_amd", "csrc", "replay_thunks.inc")).read()
    for n in names:
        assert n in _lib.EXPORTS and hasattr(lib, n) and f"thunk_{n}(" in thunks, n
    assert in_all_three_builds("validate.hip")               # libdosx.so and the two diagnostic builds
    from dostransformer_amd import _abi
    assert (_abi.DOSX_CHECK_RULES, _abi.DOSX_CHECK_THREADS, _abi.DOSX_EXCHANGE_OK, _abi.DOSX_EXCHANGE_STALLED) == (7, 256, 0, 1)
    assert [f for f, _ in _lib.BatchCheck._fields_] == ["edge_index", "batch", "system", "N", "E", "B", "n_max", "prompts",
                                                        "require_sorted", "crystal_count"]

    def refused(rc, *words):
        msg = lib.dosx_last_error().decode()
        assert rc == -22 and all(w in msg for w in words), (rc, msg)

    fake = 0x1000                                        # never dereferenced: every call below is refused before any launch
    d = _lib.BatchCheck()
    d.N, d.E, d.B, d.prompts = 6, 7, 3, 7
    d.batch, d.crystal_count = fake, fake
    refused(lib.dosx_batch_check(C.byref(d), fake, None), "null edge_index", "E=7")
    d.edge_index = fake
    refused(lib.dosx_batch_check(C.byref(d), None, None), "null report")
    refused(lib.dosx_batch_check(None, fake, None), "null descriptor")
    for field in ("N", "E", "B", "n_max", "prompts"):
        keep = getattr(d, field)
        setattr(d, field, -1)
        refused(lib.dosx_batch_check(C.byref(d), fake, None), "negative size", f"{field}=-1")
        setattr(d, field, keep)
    d.batch = None
    refused(lib.dosx_batch_check(C.byref(d), fake, None), "null batch", "N=6")
    d.batch, d.crystal_count = fake, None
    refused(lib.dosx_batch_check(C.byref(d), fake, None), "null crystal_count")
    for fn, who in ((lib.dosx_finite_check_f32, "dosx_finite_check_f32"), (lib.dosx_finite_check_f64, "dosx_finite_check_f64")):
        refused(fn(fake, -1, fake, None), who, "negative size")
        refused(fn(fake, 4, None, None), who, "null report slot")
        refused(fn(None, 4, fake, None), who, "null tensor")
        refused(fn(fake + 2, 4, fake, None), who, "not aligned")
        assert fn(None, 0, fake, None) == 0                        # nothing to look at: no launch
    refused(lib.dosx_exchange_status(None, 0, None), "dosx_exchange_status", "null output")
    refused(lib.dosx_exchange_selftest(0, 0, None), "dosx_exchange_selftest", "kernel id 0")
    refused(lib.dosx_exchange_selftest(4, 0, None), "dosx_exchange_selftest", "kernel id 4")
    refused(lib.dosx_exchange_selftest(1, -1, None), "dosx_exchange_selftest", "tile -1")


def test_check_is_a_method_of_every_driver_and_a_no_op_off_the_gpu():
    """Constructor signatures stay; check() exists on the trainers and predictors (a module on the CPU has launched nothing)."""
    from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
    from dostransformer_amd.predict import Predictor, Predictor64
    from dostransformer_amd.train import Trainer
    from dostransformer_amd.train64 import GraphnetworkTrainer64, Trainer64
    for cls in (Trainer, Trainer64, GraphnetworkTrainer64, Predictor, Predictor64):
        assert callable(getattr(cls, "check")), cls
    torch.manual_seed(0)
    t = Trainer(DOSTransformer_phonon(2, 1, 118, 4, 16, "cpu", 0.0))
    assert t.check() is None
