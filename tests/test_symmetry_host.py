"""The crystal-system derivation on the CPU (dostransformer_amd/symmetry.py, the numpy twin of csrc/symmetry.hip): known answers
under every transform that must not change them, operation counts, the classification table, and the ``crystal_system=`` modes of
featurize.build_*_all through the host path.

Condition on the inputs: the twin's margin - the smallest relative distance to symprec of any comparison it makes, evaluated
without early exits - is at least 0.2 on every input used here, so no decision sits near its threshold."""
import functools
import inspect

import numpy as np
import pytest

from dostransformer_amd import featurize, symmetry
from dostransformer_amd._lib import DosxError
from tests import symmetry_cases as sc

MARGIN = 0.2


@functools.lru_cache(maxsize=None)
def _forms():
    forms = sc.all_forms()
    return forms, symmetry.crystal_systems_host([f[1] for f in forms])


def test_known_answers_under_every_transform():
    forms, rep = _forms()
    assert len(forms) == 5 * len(sc.CASES) and len(sc.CASES) == 18
    assert rep.margin >= MARGIN, rep.margin
    for i, (label, _, code, n_ops, n_t) in enumerate(forms):
        assert int(rep.system[i]) == code, (label, rep.names[i])
        assert int(rep.n_ops[i]) == n_ops, (label, int(rep.n_ops[i]))
        assert int(rep.n_translations[i]) == n_t, (label, int(rep.n_translations[i]))
        assert bool(rep.consistent[i]) and rep.names[i] == symmetry.SYSTEM_NAMES[code]
    rep.raise_if_inconsistent()
    assert {f[2] for f in forms} == set(range(7))                        # every crystal system occurs


def test_operation_counts_and_kept_matrices():
    forms, rep = _forms()
    at = {f[0]: i for i, f in enumerate(forms)}
    for name, n in (("diamond", 48), ("zincblende", 24), ("alpha-quartz", 6), ("wurtzite", 12), ("hcp", 24), ("rutile", 16)):
        assert int(rep.n_ops[at[name]]) == n == sc.CASES[name][2]
    assert int(rep.n_lattice_ops[at["cubic metric, tetragonal decoration"]]) == 48          # the atoms matter, not the metric
    for i in range(len(forms)):
        n, ops = int(rep.n_ops[i]), rep.ops[i].numpy().astype(np.int64)
        assert not ops[n:].any() and n <= int(rep.n_lattice_ops[i]) <= 48
        kept = [tuple(r) for r in ops[:n]]
        assert kept == sorted(set(kept))                                  # lexicographic, no duplicate
        assert (1, 0, 0, 0, 1, 0, 0, 0, 1) in kept                        # the identity is always kept
        dets = [round(np.linalg.det(np.array(r).reshape(3, 3))) for r in kept]
        assert set(dets) <= {1, -1}
        mats = {r for r in kept}
        for r in kept[:6]:                                                # closed under products (a group)
            for s in kept[:6]:
                assert tuple((np.array(r).reshape(3, 3) @ np.array(s).reshape(3, 3)).reshape(-1)) in mats


def test_classification_table_is_complete():
    assert len(symmetry.POINT_GROUPS) == 11
    want = {"1": 6, "2": 5, "222": 4, "4": 2, "422": 2, "3": 3, "32": 3, "6": 1, "622": 1, "23": 0, "432": 0}
    assert {g: c for g, _, c in symmetry.POINT_GROUPS.values()} == want
    for (n2, n3, n4, n6), (_, order, code) in symmetry.POINT_GROUPS.items():
        assert n2 + n3 + n4 + n6 + 1 == order
        for n_ops in (order, 2 * order):
            assert symmetry.classify([n2, n3, n4, n6, 1], n_ops, order) == code
        assert symmetry.classify([n2, n3, n4, n6, 1], 3 * order, order) == symmetry.INCONSISTENT
        assert symmetry.classify([n2, n3, n4, n6, 1], order, order + 1) == symmetry.INCONSISTENT
        assert symmetry.classify([n2, n3, n4, n6, 0], order, order) == symmetry.INCONSISTENT
        assert symmetry.classify([n2, n3, n4, n6, 2], order, order) == symmetry.INCONSISTENT
    assert symmetry.SYSTEM_NAMES[:6] == tuple(featurize.CRYSTAL_SYSTEMS) and symmetry.SYSTEM_NAMES[7] == "INCONSISTENT"
    assert [featurize.CRYSTAL_SYSTEMS[n] for n in symmetry.SYSTEM_NAMES[:6]] == list(range(6))


@pytest.mark.parametrize("hist", [(2, 0, 0, 0, 1), (3, 1, 0, 0, 1), (9, 8, 5, 0, 1), (1, 2, 0, 1, 1), (0, 0, 1, 0, 1), (4, 8, 0, 0, 1)])
def test_corrupted_histogram_is_inconsistent(hist):
    assert symmetry.classify(hist, sum(hist), sum(hist)) == symmetry.INCONSISTENT


def test_inconsistent_is_reported_never_a_silent_triclinic():
    tiny = sc.entry(0.05 * np.eye(3), [[0, 0, 0]], [1], "tiny")            # every unimodular W keeps lengths below symprec
    rep = symmetry.crystal_systems_host([sc.CASES["sc"][0], tiny, tiny])
    assert rep.system.tolist() == [0, 7, 7] and rep.consistent.tolist() == [True, False, False]
    assert int(rep.n_lattice_ops[1]) > 48 and int(rep.n_ops[1]) == 0 and rep.names[1] == "INCONSISTENT"
    with pytest.raises(DosxError, match=r"2 crystals with inconsistent symmetry; first: crystal 1: 0 operations with trace "
                                        r"histogram \[0, 0, 0, 0, 0\].*match no point group at symprec 0\.1"):
        rep.raise_if_inconsistent()
    with pytest.raises(DosxError, match="crystal 2: 0 operations"):
        symmetry.resolve_labels([sc.CASES["sc"][0], sc.CASES["hcp"][0], tiny], "derive", [0, 1, 6], [True, True, False], device="cpu")


def test_displaced_atom_lowers_the_system():
    moved = sc.displaced(sc.CASES["CsCl"][0], 1, [0.3, 0.0, 0.0])
    rep = symmetry.crystal_systems_host([sc.CASES["CsCl"][0], moved, sc.disguise(moved, 3)])
    assert rep.margin >= MARGIN
    assert rep.system.tolist() == [sc.CUBIC, sc.TETRAGONAL, sc.TETRAGONAL] and rep.n_ops.tolist() == [48, 8, 8]
    assert rep.n_lattice_ops.tolist() == [48, 48, 48]
    # inside the tolerance nothing changes
    near = symmetry.crystal_systems_host([sc.displaced(sc.CASES["CsCl"][0], 1, [0.03, 0.0, 0.0])])
    assert near.system.tolist() == [sc.CUBIC] and near.margin >= MARGIN


def test_cell_algebra():
    rng = np.random.default_rng(0)
    for name, (e, _, _) in sc.CASES.items():
        red = symmetry.delaunay_reduce(sc.rebase(e, rng)["cell"])
        assert np.isclose(abs(np.linalg.det(red)), abs(np.linalg.det(e["cell"])))
        m = red @ np.linalg.inv(e["cell"])                               # the same lattice: an integer unimodular relation
        assert np.allclose(m, np.rint(m), atol=1e-9), name
        gram = red @ red.T
        assert np.sort(np.diag(gram))[-1] <= np.sort((e["cell"] ** 2).sum(1))[-1] + 1e-9
    assert symmetry.primitive_cell(np.eye(3) * 4.0, np.array([[0.5, 0.0, 0.0], [0.0, 0.5, 0.0]])) is None   # not a group: 3 of 4
    prim = symmetry.primitive_cell(np.eye(3) * 4.0, np.array([[0.5, 0.5, 0.0], [0.0, 0.5, 0.5], [0.5, 0.0, 0.5]]))
    assert np.isclose(abs(np.linalg.det(prim)), 16.0)
    with pytest.raises(DosxError, match="crystal 1: singular cell"):
        symmetry.crystal_systems_host([sc.CASES["sc"][0], dict(sc.CASES["sc"][0], cell=np.array([[1.0, 0, 0], [2.0, 0, 0], [0, 0, 1.0]]))])
    with pytest.raises(ValueError, match="symprec"):
        symmetry.crystal_systems_host([sc.CASES["sc"][0]], symprec=0.0)


def _labelled():
    names = ("sc", "rutile", "hcp", "monoclinic")
    entries = [dict(sc.CASES[n][0], mp_id=f"mp-{i}", crystal_system=symmetry.SYSTEM_NAMES[sc.CASES[n][1]]) for i, n in enumerate(names)]
    return entries, [sc.CASES[n][1] for n in names]


def test_given_is_the_default_and_changes_nothing():
    for fn in (featurize.build_data_all, featurize.build_edos_all):
        p = inspect.signature(fn).parameters
        assert p["crystal_system"].default == "given" and p["symprec"].default == 0.1
    entries, codes = _labelled()
    assert featurize._derived_systems(entries, "given", featurize.CRYSTAL_SYSTEMS, False, 0.1, "cpu") is None
    assert symmetry.resolve_labels(entries, "given", [6, 6, 6, 6], [False] * 4, device="cpu") == [6, 6, 6, 6]
    with pytest.raises(ValueError, match="'given', 'derive' or 'check'"):
        symmetry.resolve_labels(entries, "guess", codes, [True] * 4, device="cpu")


def test_derive_labels_only_the_unlabelled():
    entries, codes = _labelled()
    entries[1].pop("crystal_system")
    entries[3]["crystal_system"] = ""
    entries[0]["crystal_system"] = "Hexagonal"                           # a given label is kept, right or wrong
    for table, lower in ((featurize.CRYSTAL_SYSTEMS, False), (featurize._SYSTEM_CODES, True)):
        got = featurize._derived_systems(entries, "derive", table, lower, 0.1, "cpu")
        assert got == [1, codes[1], codes[2], codes[3]]
    assert featurize._derived_systems(entries[:1], "derive", featurize.CRYSTAL_SYSTEMS, False, 0.1, "cpu") == [1]


def test_check_raises_with_the_first_mismatch():
    entries, codes = _labelled()
    assert featurize._derived_systems(entries, "check", featurize.CRYSTAL_SYSTEMS, False, 0.1, "cpu") == codes
    assert featurize._derived_systems(entries, "check", featurize._SYSTEM_CODES, True, 0.1, "cpu") == codes
    entries[1]["crystal_system"] = "Cubic"
    entries[3]["crystal_system"] = "Orthorhombic"
    with pytest.raises(DosxError, match=r"2 crystal-system labels disagree with the structure; first: crystal 1 \(mp-1\): "
                                        r"labelled Cubic, derived Tetragonal \(16 operations\)"):
        featurize._derived_systems(entries, "check", featurize.CRYSTAL_SYSTEMS, False, 0.1, "cpu")
    entries[1].pop("crystal_system")                                     # "check" labels an unlabelled entry, and still compares the rest
    with pytest.raises(DosxError, match=r"1 crystal-system label disagree.*crystal 3 \(mp-3\): labelled Orthorhombic, derived Monoclinic \(2 operations\)"):
        featurize._derived_systems(entries, "check", featurize.CRYSTAL_SYSTEMS, False, 0.1, "cpu")


def test_cpu_device_runs_the_twin():
    entries, codes = _labelled()
    rep = symmetry.crystal_systems(entries, device="cpu")
    assert rep.system.tolist() == codes and rep.margin is None
