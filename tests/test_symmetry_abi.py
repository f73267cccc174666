"""CPU-only checks of the symmetry kernels' boundary: dosx_sym_translations and dosx_sym_point_group (csrc/symmetry.hip) are
declared, replayable and prototyped, their descriptors have the stated fields, and every bad descriptor is refused with rc -22
before any launch (the addresses below are never dereferenced)."""
import ctypes as C
import os

import pytest

from tests.util import dosx_lib as _lib, in_all_three_builds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = ("cell", "frac", "species", "atom_ptr")
ENTRIES = {"dosx_sym_translations": ("SymTranslations", ("flag",)),
           "dosx_sym_point_group": ("SymPointGroup", ("n_lattice_ops", "n_ops", "ops", "hist", "code"))}


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_declared_exported_replayable_and_prototyped(name):
    _l = _lib()
    lib = _l.load()
    struct, outputs = ENTRIES[name]
    header = open(os.path.join(ROOT, "include", "dosx.h")).read()
    thunks = open(os.path.join(ROOT, "dostransformer_amd", "csrc", "replay_thunks.inc")).read()
    assert f"int {name}(const Dosx{struct}* d, dosx_stream_t stream);" in header
    assert f'{{"{name}", thunk_{name}, 2, 0}}' in thunks
    ni, nf = C.c_int(0), C.c_int(0)
    assert lib.dosx_replay_op(name.encode(), C.byref(ni), C.byref(nf)) >= 0 and (ni.value, nf.value) == (2, 0)
    cls = getattr(_l, struct)
    assert getattr(lib, name).argtypes == [C.POINTER(cls), C.c_void_p]
    assert [k for k, _ in cls._fields_] == ["C", "N", "n_min", "n_max", "symprec"] + list(INPUTS + outputs)
    assert C.sizeof(cls) == 4 * 4 + 8 + 8 * len(INPUTS + outputs)
    assert in_all_three_builds("symmetry.hip")
    from dostransformer_amd import ops
    assert callable(getattr(ops, name[5:]))


def _descriptor(_l, name):
    struct, outputs = ENTRIES[name]
    d = getattr(_l, struct)()
    d.C, d.N, d.n_min, d.n_max, d.symprec = 3, 40, 1, 30, 0.1
    for i, k in enumerate(INPUTS + outputs):
        setattr(d, k, 0x10000 * (i + 1))
    return d


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_every_refusal_comes_before_any_launch(name):
    _l = _lib()
    lib = _l.load()
    fn = getattr(lib, name)
    err = lambda: lib.dosx_last_error().decode()

    def refused(d, word):
        assert fn(C.byref(d), None) == -22
        assert name in err() and word in err(), err()

    assert fn(None, None) == -22 and name in err() and "null descriptor" in err()
    for field, bad, word in (("C", 0, "C=0"), ("C", -1, "C=-1"), ("N", 0, "N=0"), ("N", -5, "N=-5"),
                             ("n_min", 0, "empty crystal"), ("n_min", -2, "empty crystal"), ("n_max", 0, "n_max=0"),
                             ("n_max", 1 << 21, "n_max=2097152"), ("symprec", 0.0, "symprec"), ("symprec", -0.1, "symprec"),
                             ("symprec", float("nan"), "symprec")):
        d = _descriptor(_l, name)
        setattr(d, field, bad)
        refused(d, word)
    for k in INPUTS:
        d = _descriptor(_l, name)
        setattr(d, k, None)
        refused(d, "null input")
    for k in ENTRIES[name][1]:
        d = _descriptor(_l, name)
        setattr(d, k, None)
        refused(d, "null output")


def test_python_layer_refuses_a_singular_cell_and_an_empty_crystal():
    import numpy as np
    from dostransformer_amd import symmetry
    from dostransformer_amd._lib import DosxError
    good = {"cell": np.eye(3) * 3.0, "positions": np.zeros((1, 3)), "numbers": [29]}
    flat = dict(good, cell=np.array([[3.0, 0, 0], [0, 3.0, 0], [3.0, 3.0, 0]]))
    with pytest.raises(DosxError, match="crystal 2: singular cell"):
        symmetry.crystal_systems([good, good, flat], device="cpu")
    with pytest.raises(ValueError, match="entry 1: needs >= 1 atom"):
        symmetry.crystal_systems([good, dict(good, positions=np.zeros((0, 3)), numbers=[])], device="cpu")
    with pytest.raises(ValueError, match="symprec"):
        symmetry.crystal_systems([good], symprec=-1.0, device="cpu")
