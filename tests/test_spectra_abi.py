"""CPU-only checks of the spectra kernels' boundary: dosx_spectra_broaden and dosx_spectra_interp (csrc/spectra.hip) are declared,
replayable and prototyped, their descriptors have the stated fields, and every bad descriptor is refused with rc -22 before any
launch, with the argument named (the addresses below are never dereferenced)."""
import ctypes as C
import os

import pytest

from tests.util import dosx_lib as _lib, in_all_three_builds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ("y", "y_max", "area", "y_norm", "report")
ENTRIES = {
    "dosx_spectra_broaden": ("Spectra", ("C", "T", "S", "kind", "n_min", "n_max", "e0", "de", "cutoff"),
                             ("ptr", "e", "v", "shift", "sigma")),
    "dosx_spectra_interp": ("SpectraInterp", ("C", "T", "S", "reserved", "n_min", "n_max", "e0", "de"), ("ptr", "e", "v", "shift")),
}


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_declared_exported_replayable_and_prototyped(name):
    _l = _lib()
    lib = _l.load()
    struct, scalars, inputs = ENTRIES[name]
    header = open(os.path.join(ROOT, "include", "dosx.h")).read()
    thunks = open(os.path.join(ROOT, "dostransformer_amd", "csrc", "replay_thunks.inc")).read()
    assert f"int {name}(const Dosx{struct}* d, dosx_stream_t stream);" in header
    assert f'{{"{name}", thunk_{name}, 2, 0}}' in thunks
    ni, nf = C.c_int(0), C.c_int(0)
    assert lib.dosx_replay_op(name.encode(), C.byref(ni), C.byref(nf)) >= 0 and (ni.value, nf.value) == (2, 0)
    cls = getattr(_l, struct)
    assert getattr(lib, name).argtypes == [C.POINTER(cls), C.c_void_p]
    assert [k for k, _ in cls._fields_] == list(scalars + inputs + OUTPUTS)
    assert C.sizeof(cls) == 6 * 4 + 8 * (len(scalars) - 6) + 8 * len(inputs + OUTPUTS)
    assert in_all_three_builds("spectra.hip")
    from dostransformer_amd import _abi, ops
    assert callable(getattr(ops, name[5:]))
    assert (_abi.DOSX_SPECTRA_POINTS, _abi.DOSX_SPECTRA_CURVE) == (0, 1)


def _descriptor(_l, name):
    struct, scalars, inputs = ENTRIES[name]
    d = getattr(_l, struct)()
    d.C, d.T, d.S, d.n_min, d.n_max, d.e0, d.de = 3, 40, 201, 2, 30, -4.0, 0.04
    if "kind" in scalars:
        d.kind, d.cutoff = _l.DOSX_SPECTRA_CURVE, 6.0
    for i, k in enumerate(inputs + OUTPUTS):
        setattr(d, k, 0x10000 * (i + 1))
    return d


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_every_refusal_comes_before_any_launch(name):
    _l = _lib()
    lib = _l.load()
    fn = getattr(lib, name)
    err = lambda: lib.dosx_last_error().decode()
    broaden = name == "dosx_spectra_broaden"

    def refused(d, word):
        assert fn(C.byref(d), None) == -22
        assert name in err() and word in err(), err()

    assert fn(None, None) == -22 and name in err() and "null descriptor" in err()
    cases = [("C", 0, "C=0"), ("C", -1, "C=-1"), ("T", -1, "T=-1"), ("S", 0, "S=0"), ("S", -3, "S=-3"), ("S", 1025, "S=1025"),
             ("de", 0.0, "de=0"), ("de", -0.5, "de=-0.5"), ("de", float("nan"), "de=nan"), ("e0", float("inf"), "e0=inf"),
             ("n_min", -1, "n_min=-1"), ("n_min", 1, "n_min=1"), ("n_min", 0, "n_min=0"), ("n_max", 1, "n_max=1"),
             ("n_max", 1 << 20, "n_max=1048576")]
    if broaden:
        cases += [("cutoff", 0.0, "cutoff"), ("cutoff", -6.0, "cutoff"), ("cutoff", float("nan"), "cutoff"), ("kind", 2, "kind=2"),
                  ("kind", -1, "kind=-1")]
    for field, bad, word in cases:
        d = _descriptor(_l, name)
        setattr(d, field, bad)
        refused(d, word)
    for k in ENTRIES[name][2] + tuple(o for o in OUTPUTS if o != "y_norm"):
        d = _descriptor(_l, name)
        setattr(d, k, None)
        refused(d, f"null {k}")
    if broaden:                                                         # points may be empty, and may be as short as they like
        d = _descriptor(_l, name)
        d.kind, d.n_min, d.n_max = _l.DOSX_SPECTRA_POINTS, -1, 0
        refused(d, "n_min=-1")
        d.n_min, d.n_max = 1, 0
        refused(d, "n_max=0")


def test_python_layer_refuses_what_the_entry_points_refuse():
    import numpy as np
    from dostransformer_amd import spectra
    e, v = [np.linspace(-1.0, 1.0, 5)], [np.ones(5)]
    grid = spectra.Grid(-1.0, 0.5, 5)
    for bad, word in ((spectra.Grid(0.0, 0.1, 0), "bins=0"), (spectra.Grid(0.0, 0.1, 1025), "bins=1025"),
                      (spectra.Grid(0.0, 0.0, 5), "de=0.0"), (spectra.Grid(float("nan"), 0.1, 5), "finite")):
        with pytest.raises(ValueError, match=word):
            spectra.broaden(e, v, bad, 0.1, device="cpu")
        with pytest.raises(ValueError, match=word):
            spectra.resample(e, v, bad, device="cpu")
    for cutoff in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cutoff"):
            spectra.broaden(e, v, grid, 0.1, cutoff=cutoff, device="cpu")
    with pytest.raises(ValueError, match="crystal 1: a curve needs at least 2 samples"):
        spectra.broaden(e + [np.zeros(1)], v + [np.ones(1)], grid, 0.1, device="cpu")
    with pytest.raises(ValueError, match="kind"):
        spectra.broaden(e, v, grid, 0.1, kind="lorentz", device="cpu")
    with pytest.raises(ValueError, match="one value per crystal"):
        spectra.broaden(e, v, grid, [0.1, 0.2], device="cpu")
    with pytest.raises(ValueError, match="ptr must ascend"):
        spectra.broaden(e[0], v[0], grid, 0.1, ptr=[0, 3], device="cpu")
    assert spectra.broaden(e[:0] + [np.zeros(0)], [np.zeros(0)], grid, 0.1, kind="points", device="cpu").y.abs().sum() == 0.0
