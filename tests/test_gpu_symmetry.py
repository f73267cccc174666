"""dosx_sym_translations / dosx_sym_point_group on the GPU (csrc/symmetry.hip) against the numpy twin of
dostransformer_amd/symmetry.py, field by field: translation flags, operation counts, the kept matrices, the trace histogram and
the code - all exact (they are decisions, not numbers).

Condition on the inputs: the twin's margin (the smallest relative distance to symprec of any comparison, without early exits) is
at least 0.2 on every input used here, so a last-place difference between the two arithmetics cannot move a decision."""
import functools

import numpy as np
import pytest
import torch

from dostransformer_amd import featurize, symmetry
from dostransformer_amd._lib import DosxError
from tests import symmetry_cases as sc
from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu

MARGIN = 0.2
FIELDS = ("system", "n_ops", "n_lattice_ops", "n_translations", "hist", "ops")


def _compare(entries, host=None):
    host = symmetry.crystal_systems_host(entries) if host is None else host
    assert host.margin >= MARGIN, host.margin
    dev = symmetry.crystal_systems(entries, device=DEV)
    assert np.array_equal(dev.flags, host.flags)
    assert np.array_equal(dev.cells, host.cells) and np.array_equal(dev.atom_ptr, host.atom_ptr)
    for k in FIELDS:
        assert torch.equal(getattr(dev, k), getattr(host, k)), k
    assert dev.names == host.names
    return dev


@functools.lru_cache(maxsize=None)
def _forms():
    forms = sc.all_forms()
    return forms, symmetry.crystal_systems_host([f[1] for f in forms])


@functools.lru_cache(maxsize=None)
def _large():
    """sc 5x5x5 (125 atoms, 124 translations), rutile 3x3x3 (162 atoms: more than a wave of atoms and of candidates), and a crystal
    past the 1024-atom LDS staging limit: a 2x1x1 supercell of a triclinic 8x8x9 grid of one species with one foreign atom (1152
    atoms, one translation; its primitive cell keeps all 1152 as coincident pairs, so both kernels read it from global memory)."""
    grid = [[i / 8, j / 8, k / 9] for i in range(8) for j in range(8) for k in range(9)]
    cell = sc.cell_from_parameters(11.2, 14.4, 18.9, 75, 83, 98)
    big = sc.disguise(sc.supercell(sc.entry(cell, grid, [3] + [9] * 575, "grid"), (2, 1, 1)), 9)
    cube = sc.disguise(sc.supercell(sc.CASES["sc"][0], (5, 5, 5)), 7)
    rutile = sc.disguise(sc.supercell(sc.CASES["rutile"][0], (3, 3, 3)), 8)
    small = [sc.CASES[n][0] for n in ("diamond", "alpha-quartz", "triclinic", "sc")]
    entries = [big, *small[:2], cube, *small[2:], rutile]
    return entries, symmetry.crystal_systems_host(entries)


def test_all_cases_and_transforms_in_one_launch():
    forms, host = _forms()
    dev = _compare([f[1] for f in forms], host)
    assert dev.system.tolist() == [f[2] for f in forms] and dev.n_ops.tolist() == [f[3] for f in forms]
    assert dev.n_translations.tolist() == [f[4] for f in forms]
    assert len(set(np.diff(dev.atom_ptr).tolist())) > 8                  # mixed sizes
    dev.raise_if_inconsistent()


@pytest.mark.parametrize("name", ["diamond", "sc", "alpha-quartz"])
def test_one_crystal(name):
    dev = _compare([sc.CASES[name][0]])                                   # C = 1; "sc" is a one-atom crystal
    assert dev.system.tolist() == [sc.CASES[name][1]] and dev.n_ops.tolist() == [sc.CASES[name][2]]


def test_large_crystals_first_and_last_and_past_the_staging_limit():
    entries, host = _large()
    n = [len(e["numbers"]) for e in entries]
    assert n[0] == 1152 > 1024 and n[3] == 125 and n[-1] == 162 and max(n[1:3] + n[4:6]) < 10
    dev = _compare(entries, host)
    assert dev.n_translations.tolist() == [1, 0, 0, 124, 0, 0, 26]
    assert dev.system.tolist() == [sc.TRICLINIC, sc.CUBIC, sc.TRIGONAL, sc.CUBIC, sc.TRICLINIC, sc.CUBIC, sc.TETRAGONAL]
    assert dev.n_ops.tolist() == [2, 48, 6, 48, 1, 48, 16]
    assert _compare([entries[-1], entries[1], entries[0]]).n_translations.tolist() == [26, 0, 1]      # the largest one last


def test_the_ops_report_inconsistent_instead_of_triclinic():
    tiny = sc.entry(0.05 * np.eye(3), [[0, 0, 0]], [1], "tiny")            # more than 48 lattice operations at symprec 0.1
    entries = [sc.CASES["hcp"][0], tiny]
    host, dev = symmetry.crystal_systems_host(entries), symmetry.crystal_systems(entries, device=DEV)
    for k in FIELDS:
        assert torch.equal(getattr(dev, k), getattr(host, k)), k
    assert dev.system.tolist() == [sc.HEXAGONAL, sc.INCONSISTENT] and int(dev.n_lattice_ops[1]) > 48 and int(dev.n_ops[1]) == 0
    with pytest.raises(DosxError, match="crystal 1: 0 operations"):
        dev.raise_if_inconsistent()


def _structures():
    names = ("sc", "rutile", "hcp", "monoclinic", "zincblende")
    out = []
    for i, n in enumerate(names):
        e = dict(sc.CASES[n][0], mp_id=f"mp-{i}", crystal_system=symmetry.SYSTEM_NAMES[sc.CASES[n][1]], phdos=np.linspace(0.0, 1.0, 51))
        e["symbols"] = [featurize.SYMBOLS[z - 1] for z in e["numbers"]]
        out.append(e)
    return out, [sc.CASES[n][1] for n in names]


@pytest.mark.parametrize("which", ["phonon", "edos"])
def test_build_all_derive_and_check(which):
    entries, codes = _structures()
    if which == "phonon":
        build = lambda es, **kw: featurize.build_data_all(es, r_max=4.0, device=DEV, **kw)
    else:
        build = lambda es, **kw: featurize.build_edos_all(es, np.zeros((100, 4)), device=DEV, **kw)
    given = build(entries)
    checked = build(entries, crystal_system="check")
    assert [int(d["system"]) for d in given] == codes == [int(d["system"]) for d in checked]
    for a, b in zip(given, checked):                                     # nothing but the label can differ
        assert a.keys() == b.keys() and torch.equal(a["edge_index"], b["edge_index"]) and torch.equal(a["x"], b["x"])
    bare = [{k: v for k, v in e.items() if k != "crystal_system"} for e in entries]
    bare[2]["crystal_system"] = "Cubic" if which == "phonon" else "cubic"            # kept by "derive", caught by "check"
    derived = build(bare, crystal_system="derive")
    assert [int(d["system"]) for d in derived] == codes[:2] + [0] + codes[3:]
    with pytest.raises(DosxError, match=r"crystal 2 \(mp-2\): labelled Cubic, derived Hexagonal \(24 operations\)"):
        build(bare, crystal_system="check")
    tiny = dict(bare[0], cell=bare[0]["cell"] * (0.05 / 3.0))            # (its one atom sits at the origin)
    with pytest.raises(DosxError, match="crystal 1: 0 operations"):
        build([bare[0], tiny], crystal_system="derive")
