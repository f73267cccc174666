"""Crystal-system prompt labels derived from the structures themselves (include/dosx.h: DosxSymTranslations / DosxSymPointGroup).

The reference reads ``entry.crystal_system`` from Materials-Project metadata (`utils.py:277-290`), which comes from pymatgen /
spglib; neither is in the tree nor pinned, so the definition restated in include/dosx.h is the contract (PARITY UNPINNED at that
boundary).  In short, per crystal, all in float64 without fused multiply-adds:

(a) Delaunay-reduce the cell, atoms as fractional rows ``x`` of the reduced basis ``A`` (``r = x A``);
(b) pure translations ``t = x_j - x_ref`` among the atoms of the rarest species -> primitive lattice, reduced again;
(c) lattice operations: integer ``W`` with entries in {-1, 0, 1}, ``|det W| = 1``, that keep the lengths of the three basis
    vectors and of the three face diagonals within ``symprec``;
(d) structure operations: the ``W`` for which some ``t = x_j - x_ref W`` maps every atom onto an atom of its species;
(e) the trace histogram of the proper parts ``det(W) W`` names one of the eleven proper point groups, the group names the
    crystal system; anything else is INCONSISTENT (code 7), never a silent 6.

``crystal_systems`` runs (b) and (c)-(e) as two libdosx launches for the whole dataset (csrc/symmetry.hip) with one numpy step
between them (the O(1)-per-crystal cell algebra); ``crystal_systems_host`` is the same definition in numpy - the twin the tests
hold the kernels to, and what a CPU ``device`` runs."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import DosxError

SYSTEM_NAMES = ("Cubic", "Hexagonal", "Tetragonal", "Trigonal", "Orthorhombic", "Monoclinic", "Triclinic", "INCONSISTENT")
INCONSISTENT = 7
MAX_OPS = 48
# (2-fold, 3-fold, 4-fold, 6-fold axes' rotations) of the eleven proper point groups -> (symbol, order, crystal-system code)
POINT_GROUPS = {
    (0, 0, 0, 0): ("1", 1, 6), (1, 0, 0, 0): ("2", 2, 5), (3, 0, 0, 0): ("222", 4, 4), (1, 0, 2, 0): ("4", 4, 2),
    (5, 0, 2, 0): ("422", 8, 2), (0, 2, 0, 0): ("3", 3, 3), (3, 2, 0, 0): ("32", 6, 3), (1, 2, 0, 2): ("6", 6, 1),
    (7, 2, 0, 2): ("622", 12, 1), (3, 8, 0, 0): ("23", 12, 0), (9, 8, 6, 0): ("432", 24, 0),
}
SINGULAR_REL = 1e-12             # a cell with |det| below this times the cube of its longest edge is refused

_digits = np.array([-1, 0, 1], np.int64)
# all 3^9 matrices with entries in {-1, 0, 1}, in the lexicographic order of their nine entries (row-major)
ALL_W = np.stack(np.meshgrid(*([_digits] * 9), indexing="ij"), -1).reshape(-1, 3, 3)
_det = (ALL_W[:, 0, 0] * (ALL_W[:, 1, 1] * ALL_W[:, 2, 2] - ALL_W[:, 1, 2] * ALL_W[:, 2, 1])
        - ALL_W[:, 0, 1] * (ALL_W[:, 1, 0] * ALL_W[:, 2, 2] - ALL_W[:, 1, 2] * ALL_W[:, 2, 0])
        + ALL_W[:, 0, 2] * (ALL_W[:, 1, 0] * ALL_W[:, 2, 1] - ALL_W[:, 1, 1] * ALL_W[:, 2, 0]))
UNIMODULAR = np.flatnonzero(np.abs(_det) == 1)          # indices into ALL_W, ascending = lexicographic


def classify(hist, n_ops: int, n_proper: Optional[int] = None) -> int:
    """Step (e): the five-bin trace histogram of the distinct proper parts (traces -1, 0, 1, 2, 3), the number of kept operations
    and the number of distinct proper parts -> the crystal-system code, 7 when they name no point group."""
    h = [int(v) for v in hist]
    group = POINT_GROUPS.get(tuple(h[:4]))
    if group is None or h[4] != 1:
        return INCONSISTENT
    order = group[1]
    if (n_proper is not None and int(n_proper) != order) or int(n_ops) not in (order, 2 * order):
        return INCONSISTENT
    return group[2]


# ---- the O(1)-per-crystal cell algebra (host, both paths) ------------------------------------------------------------------
def delaunay_reduce(cell: np.ndarray) -> np.ndarray:
    """Delaunay reduction of a 3x3 cell (rows = lattice vectors): the three shortest independent vectors of the seven that the
    obtuse superbase b0..b3 (b3 = -(b0+b1+b2), every b_i.b_j <= 0) spans.  Same lattice, same handedness."""
    cell = np.asarray(cell, np.float64).reshape(3, 3)
    b = np.vstack([cell, -cell.sum(0)])
    eps = 1e-10 * float((cell * cell).sum(1).max())
    for _ in range(1000):
        for i, j in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):
            if float(b[i] @ b[j]) > eps:
                for k in range(4):
                    if k != i and k != j:
                        b[k] = b[k] + b[i]
                b[i] = -b[i]
                break
        else:
            break
    else:
        raise DosxError("Delaunay reduction did not terminate")
    cand = np.vstack([b, b[0] + b[1], b[1] + b[2], b[2] + b[0]])
    cand = cand[np.argsort((cand * cand).sum(1), kind="stable")]
    vol = abs(float(np.linalg.det(cell)))
    for i in range(5):
        for j in range(i + 1, 6):
            for k in range(j + 1, 7):
                red = cand[[i, j, k]]
                d = float(np.linalg.det(red))
                if abs(abs(d) - vol) < 1e-6 * vol:
                    return red if (d > 0) == (np.linalg.det(cell) > 0) else -red
    raise DosxError("Delaunay reduction found no basis")


def _hermite_rows(rows: np.ndarray) -> np.ndarray:
    """Row-style Hermite reduction of an integer [m, 3] generator set of full rank -> an upper-triangular 3x3 basis of its span."""
    rows = [list(map(int, r)) for r in rows]
    basis = []
    for col in range(3):
        live = [r for r in rows if r[col] != 0]
        rows = [r for r in rows if r[col] == 0]
        while len(live) > 1:
            live.sort(key=lambda r: abs(r[col]))
            p = live[0]
            rest = []
            for r in live[1:]:
                q = r[col] // p[col]
                r = [a - q * b for a, b in zip(r, p)]
                (rest if r[col] != 0 else rows).append(r)
            live = [p] + rest
        basis.append(live[0] if live else [0, 0, 0])
    return np.array(basis, np.int64)


def primitive_cell(cell: np.ndarray, translations: np.ndarray) -> Optional[np.ndarray]:
    """The Delaunay-reduced primitive lattice generated by ``cell`` (rows) and the fractional pure translations ``[n_t, 3]``; its
    volume is V / (n_t + 1).  None when the translations do not close into a group of that order."""
    m = translations.shape[0] + 1
    p = np.rint(translations * m).astype(np.int64)
    if np.abs(translations * m - p).max() > 0.25:
        return None
    h = _hermite_rows(np.vstack([p, m * np.eye(3, dtype=np.int64)]))
    if abs(int(round(np.linalg.det(h.astype(np.float64))))) != m * m:
        return None
    return delaunay_reduce((h.astype(np.float64) / m) @ cell)


# ---- the numpy twins of the two kernels ----------------------------------------------------------------------------------
def reference_atom(species: np.ndarray) -> int:
    """First atom of the rarest species, ties to the smallest species number."""
    vals, counts = np.unique(species, return_counts=True)
    return int(np.flatnonzero(species == vals[np.argmin(counts)])[0])          # (argmin: first minimum, vals ascending)


def _maps_onto(y: np.ndarray, x: np.ndarray, same: np.ndarray, A: np.ndarray, symprec: float) -> Tuple[np.ndarray, float]:
    """y [..., n, 3] moved atoms, x [n, 3]: does every atom i have an atom k of its species within symprec (periodic)?  Also the
    smallest relative distance of any same-species comparison to the threshold.  Summation order of csrc/symmetry.hip."""
    n, s2 = x.shape[0], symprec * symprec
    lands = np.zeros(y.shape[:-1], bool)
    below, above = 0.0, np.inf                          # the squared distances nearest to the threshold from either side
    rows = max(1, (1 << 21) // n)                       # bounds the [rows, n] temporaries
    for lo in range(0, n, rows):
        d = [y[..., lo:lo + rows, None, a] - x[None, :, a] for a in range(3)]
        d = [v - np.rint(v) for v in d]
        c = [(d[0] * A[0, a] + d[1] * A[1, a]) + d[2] * A[2, a] for a in range(3)]
        r2 = np.where(same[lo:lo + rows], (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2], np.inf)
        hit = r2 < s2
        lands[..., lo:lo + rows] = hit.any(-1)
        below = max(below, float(np.max(r2, where=hit, initial=0.0)))
        above = min(above, float(np.min(r2, where=~hit, initial=np.inf)))
    return lands.all(-1), min(abs(np.sqrt(below) - symprec), abs(np.sqrt(above) - symprec)) / symprec


def translations_host(cell, frac, species, atom_ptr, symprec: float = 0.1) -> Tuple[np.ndarray, float]:
    """Twin of ``dosx_sym_translations``: one byte per atom (is ``x_j - x_ref`` a pure translation), and the margin."""
    cell, frac, species = np.asarray(cell, np.float64), np.asarray(frac, np.float64), np.asarray(species)
    flag = np.zeros(frac.shape[0], np.uint8)
    margin = np.inf
    for c in range(cell.shape[0]):
        a, b = int(atom_ptr[c]), int(atom_ptr[c + 1])
        x, z = frac[a:b], species[a:b]
        ref = reference_atom(z)
        cand = np.flatnonzero((z == z[ref]) & (np.arange(b - a) != ref))
        if cand.size == 0:
            continue
        same = z[:, None] == z[None, :]
        step = max(1, min(64, (1 << 21) // ((b - a) * (b - a))))
        for lo in range(0, cand.size, step):
            js = cand[lo:lo + step]
            y = x[None, :, :] + (x[js] - x[ref])[:, None, :]
            ok, m = _maps_onto(y, x, same, cell[c], symprec)
            flag[a + js] = ok
            margin = min(margin, m)
    return flag, margin


def _lengths(v: np.ndarray) -> np.ndarray:
    return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])


def lattice_ops_host(A: np.ndarray, symprec: float) -> Tuple[np.ndarray, float]:
    """Step (c): indices into ALL_W (ascending) of the lattice operations of the basis ``A``, and the margin of the length tests."""
    W = ALL_W[UNIMODULAR].astype(np.float64)
    img = np.stack([(W[:, :, 0] * A[0, a] + W[:, :, 1] * A[1, a]) + W[:, :, 2] * A[2, a] for a in range(3)], -1)   # [m, 3 rows, 3]
    six = lambda v: np.stack([v[..., 0, :], v[..., 1, :], v[..., 2, :], v[..., 0, :] + v[..., 1, :], v[..., 0, :] + v[..., 2, :],
                              v[..., 1, :] + v[..., 2, :]], -2)
    diff = np.abs(_lengths(six(img)) - _lengths(six(A)))
    return UNIMODULAR[(diff < symprec).all(-1)], float((np.abs(diff - symprec) / symprec).min())


def point_group_host(cell, frac, species, atom_ptr, symprec: float = 0.1, margin: bool = True) -> Dict[str, object]:
    """Twin of ``dosx_sym_point_group``: n_lattice_ops [C], n_ops [C], ops [C, 48, 9] int8 (kept matrices in lexicographic order,
    zero rows after them), hist [C, 5], code [C]; and ``margin``.  With ``margin=False`` the search for a translation stops at
    the first candidate that works (same answer, no margin)."""
    cell, frac, species = np.asarray(cell, np.float64), np.asarray(frac, np.float64), np.asarray(species)
    C = cell.shape[0]
    out = {"n_lattice_ops": np.zeros(C, np.int32), "n_ops": np.zeros(C, np.int32), "ops": np.zeros((C, MAX_OPS, 9), np.int8),
           "hist": np.zeros((C, 5), np.int32), "code": np.full(C, INCONSISTENT, np.int32)}
    worst = np.inf
    for c in range(C):
        a, b = int(atom_ptr[c]), int(atom_ptr[c + 1])
        x, z, A = frac[a:b], species[a:b], cell[c]
        lat, m = lattice_ops_host(A, symprec)
        worst = min(worst, m)
        out["n_lattice_ops"][c] = lat.size
        if lat.size > MAX_OPS:
            continue                                    # more lattice operations than any point group has: INCONSISTENT
        ref = reference_atom(z)
        cand = np.flatnonzero(z == z[ref])
        same = z[:, None] == z[None, :]
        kept = []
        for w in lat:
            Wf = ALL_W[w].astype(np.float64)
            mv = lambda v: (v[..., 0:1] * Wf[0] + v[..., 1:2] * Wf[1]) + v[..., 2:3] * Wf[2]
            xw = mv(x)
            t = x[cand] - mv(x[ref])
            found = False
            step = max(1, min(64, (1 << 21) // ((b - a) * (b - a)))) if margin else 1
            for lo in range(0, cand.size, step):
                ok, m = _maps_onto(xw[None, :, :] + t[lo:lo + step, None, :], x, same, A, symprec)
                found = found or bool(ok.any())
                if margin:
                    worst = min(worst, m)
                elif found:
                    break
            if found:
                kept.append(int(w))
        out["n_ops"][c] = len(kept)
        ops = ALL_W[kept].reshape(-1, 9)
        out["ops"][c, :len(kept)] = ops
        proper = np.unique(ops * _det[kept][:, None], axis=0) if kept else np.zeros((0, 9), np.int64)
        trace = proper[:, 0] + proper[:, 4] + proper[:, 8]
        for k in range(5):
            out["hist"][c, k] = int((trace == k - 1).sum())
        out["code"][c] = classify(out["hist"][c], len(kept), proper.shape[0])
    out["margin"] = worst if margin else None
    return out


# ---- entries -> report -----------------------------------------------------------------------------------------------------
class SymmetryReport:
    """What ``crystal_systems`` found.  ``system [C]`` int64 (the reference's codes 0..6, 7 = INCONSISTENT), ``names``, ``n_ops``
    (structure operations kept), ``n_lattice_ops``, ``n_translations`` (pure translations of the given cell: 0 for a primitive
    one), ``consistent [C]`` bool, ``hist [C, 5]`` (trace histogram), ``ops [C, 48, 9]``; ``margin`` from the host twin only."""

    def __init__(self, system, n_ops, n_lattice_ops, n_translations, hist, ops, symprec, margin=None):
        self.system = torch.as_tensor(np.asarray(system), dtype=torch.int64)
        self.n_ops = torch.as_tensor(np.asarray(n_ops), dtype=torch.int64)
        self.n_lattice_ops = torch.as_tensor(np.asarray(n_lattice_ops), dtype=torch.int64)
        self.n_translations = torch.as_tensor(np.asarray(n_translations), dtype=torch.int64)
        self.hist = torch.as_tensor(np.asarray(hist), dtype=torch.int64)
        self.ops = torch.as_tensor(np.asarray(ops), dtype=torch.int8)
        self.consistent = self.system != INCONSISTENT
        self.names = [SYSTEM_NAMES[int(s)] for s in self.system]
        self.symprec = float(symprec)
        self.margin = margin

    def describe(self, c: int) -> str:
        return (f"crystal {c}: {int(self.n_ops[c])} operations with trace histogram {self.hist[c].tolist()} "
                f"({int(self.n_lattice_ops[c])} lattice operations, {int(self.n_translations[c])} translations) "
                f"match no point group at symprec {self.symprec:g}")

    def raise_if_inconsistent(self) -> None:
        bad = torch.nonzero(~self.consistent).reshape(-1)
        if bad.numel():
            n = int(bad.numel())
            raise DosxError(f"{n} crystal{'s' if n != 1 else ''} with inconsistent symmetry; first: {self.describe(int(bad[0]))}")


def _prepare(entries: Sequence):
    """entries -> (reduced cells [C,3,3], Cartesian positions list, species [N] int32, atom_ptr [C+1])."""
    from .featurize import _Z_OF, _get
    cells, pos, spec = [], [], []
    for c, e in enumerate(entries):
        z = np.asarray(e["numbers"], np.int64) if isinstance(e, dict) and "numbers" in e else \
            np.array([_Z_OF.get(s, -1) + 1 for s in _get(e, "symbols")], np.int64)
        p = np.asarray(_get(e, "positions"), np.float64).reshape(-1, 3)
        A = np.asarray(_get(e, "cell"), np.float64).reshape(3, 3)
        if z.ndim != 1 or z.shape[0] != p.shape[0] or p.shape[0] == 0:
            raise ValueError(f"entry {c}: needs >= 1 atom and one species per position")
        if z.min() < 0 or z.max() >= 1 << 20:
            raise ValueError(f"entry {c}: unknown species")
        edge = float(np.sqrt((A * A).sum(1).max()))
        if not np.isfinite(A).all() or abs(float(np.linalg.det(A))) < SINGULAR_REL * edge ** 3:
            raise DosxError(f"crystal {c}: singular cell (|det| = {abs(float(np.linalg.det(A))):g}, longest edge {edge:g})")
        cells.append(delaunay_reduce(A))
        pos.append(p)
        spec.append(z.astype(np.int32))
    n = np.array([p.shape[0] for p in pos], np.int64)
    return np.stack(cells), pos, np.concatenate(spec), np.concatenate([[0], np.cumsum(n)]).astype(np.int32)


def _fractional(cells, pos):
    return np.concatenate([p @ np.linalg.inv(A) for p, A in zip(pos, cells)])


def _run(entries, symprec, translations, point_group, margin):
    symprec = float(symprec)
    if not symprec > 0.0:
        raise ValueError(f"symprec must be positive ({symprec})")
    entries = list(entries)
    if not entries:
        return SymmetryReport(*[np.zeros(0, np.int64)] * 4, np.zeros((0, 5)), np.zeros((0, MAX_OPS, 9)), symprec)
    cells, pos, species, ptr = _prepare(entries)
    C = cells.shape[0]
    frac = _fractional(cells, pos)
    flag, m1 = translations(cells, frac, species, ptr, symprec)
    # the one host step between the launches: primitive lattices of the crystals that have translations
    n_t = np.zeros(C, np.int64)
    closed = np.ones(C, bool)
    prim = cells.copy()
    for c in np.flatnonzero(np.add.reduceat(flag.astype(np.int64), ptr[:-1].astype(np.int64))):
        a, b = int(ptr[c]), int(ptr[c + 1])
        js = np.flatnonzero(flag[a:b])
        n_t[c] = js.size
        t = frac[a + js] - frac[a + reference_atom(species[a:b])]
        red = primitive_cell(cells[c], t - np.rint(t))
        if red is None:
            closed[c] = False
        else:
            prim[c] = red
    pg = point_group(prim, _fractional(prim, pos), species, ptr, symprec)
    code = np.where(closed, pg["code"], INCONSISTENT)
    m = None if not margin else min(m1, pg["margin"])
    rep = SymmetryReport(code, pg["n_ops"], pg["n_lattice_ops"], n_t, pg["hist"], pg["ops"], symprec, m)
    # what the first stage said and the second saw, for the tests that hold the kernels to the twin: translation flags per atom,
    # the reduced primitive cells and atom_ptr
    rep.flags, rep.cells, rep.atom_ptr = flag, prim, ptr
    return rep


def crystal_systems_host(entries: Sequence, symprec: float = 0.1, margin: bool = True) -> SymmetryReport:
    """The definition in numpy.  ``report.margin``: the smallest relative distance to ``symprec`` of any comparison made,
    evaluated without early exits (None with ``margin=False``, which stops each search at its first success)."""
    return _run(entries, symprec, translations_host,
                lambda *a: point_group_host(*a, margin=margin), margin)


def crystal_systems(entries: Sequence, symprec: float = 0.1, device="cuda:0") -> SymmetryReport:
    """Crystal systems of ``entries`` (the forms ``featurize.build_data_all`` / ``build_edos_all`` take: ``cell``, Cartesian
    ``positions``, ``symbols`` or ``numbers``): two libdosx launches for the whole dataset on a GPU ``device``, the numpy twin on a
    CPU one."""
    dev = torch.device(device)
    if dev.type != "cuda":
        return crystal_systems_host(entries, symprec, margin=False)
    from . import ops

    def launch(fn, cells, frac, species, ptr, s):
        n = np.diff(ptr)
        return fn(*(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (cells, frac, species, ptr)), s,
                  n_min=int(n.min()), n_max=int(n.max()))

    def translations(*a):
        return launch(ops.sym_translations, *a).cpu().numpy(), None

    def point_group(*a):
        return {k: v.cpu().numpy() for k, v in launch(ops.sym_point_group, *a).items()}

    return _run(entries, symprec, translations, point_group, False)


def resolve_labels(entries: Sequence, mode: str, codes: Sequence[int], given: Sequence[bool], symprec: float = 0.1,
                   device="cuda:0") -> List[int]:
    """The ``crystal_system=`` modes of ``featurize.build_*_all``.  ``codes``: the labels read from the entries (6 where there is
    none), ``given``: which entries carry one.  "given": ``codes``; "derive": derived labels where none is given; "check": all
    derived, a mismatch with a given label raises.  An INCONSISTENT crystal raises in both."""
    if mode == "given":
        return list(codes)
    if mode not in ("derive", "check"):
        raise ValueError(f"crystal_system must be 'given', 'derive' or 'check', got {mode!r}")
    entries = list(entries)
    which = [c for c in range(len(entries)) if mode == "check" or not given[c]]
    if not which:
        return list(codes)
    rep = crystal_systems([entries[c] for c in which], symprec=symprec, device=device)
    bad = torch.nonzero(~rep.consistent).reshape(-1)
    if bad.numel():
        n, k = int(bad.numel()), int(bad[0])
        raise DosxError(f"{n} crystal{'s' if n != 1 else ''} with inconsistent symmetry; first: "
                        f"{rep.describe(k).replace(f'crystal {k}:', f'crystal {which[k]}:', 1)}")
    out = list(codes)
    wrong = []
    for k, c in enumerate(which):
        derived = int(rep.system[k])
        if given[c] and derived != out[c]:
            wrong.append((c, k, derived))
        out[c] = derived
    if mode == "check" and wrong:
        c, k, derived = wrong[0]
        mp_id = entries[c].get("mp_id", f"entry-{c}") if isinstance(entries[c], dict) else getattr(entries[c], "mp_id", f"entry-{c}")
        raise DosxError(f"{len(wrong)} crystal-system label{'s' if len(wrong) != 1 else ''} disagree with the structure; first: "
                        f"crystal {c} ({mp_id}): labelled {SYSTEM_NAMES[codes[c]]}, "
                        f"derived {SYSTEM_NAMES[derived]} ({int(rep.n_ops[k])} operations)")
    return out
