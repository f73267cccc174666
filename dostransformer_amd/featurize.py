"""Phonon input featurisation on the GPU (counterpart of `utils.py:249-303` build_data).

The reference builds one PyG ``Data`` per crystal on the host: ASE's periodic ``neighbor_list("ijS", cutoff=r_max,
self_interaction=True)`` (`utils.py:267`), ``edge_vec = pos[dst] - pos[src] + shift @ lattice`` (`:271-273`), node
features ``x = diag(atomic mass)[Z-1]`` (`:259-260,293`), ``z = one_hot(Z-1)``, the crystal-system code
(`:277-290`) and the target ``phdos``.  Here the neighbour search of the WHOLE dataset is one libdosx call pair
(``ops.neighbor_list``: one GPU thread per ordered atom pair, exact minimal image boxes, no ASE); the rest is index
arithmetic.  ``build_data_all`` returns host crystal dicts in the schema ``batch.collate`` / ``loader.DeviceDataset``
consume, so a dataset goes  structures -> build_data_all -> DeviceDataset -> Trainer  without ASE or PyG.

Entries may be the reference's pandas rows (``entry.structure`` an ASE ``Atoms``: ``.symbols``, ``.positions``,
``.cell.array``; ``entry.phdos``, ``entry.crystal_system``, ``entry.mp_id``) or plain dicts with the keys
``symbols, positions, cell, phdos, crystal_system, mp_id``.

Electron-DOS input featurisation (counterpart of `data/mat2graph.py:33-47,81-107,120-243`): ``build_edos_all`` turns
structures into the crystal graphs of ``synth.edos_crystal`` — the 12 nearest periodic neighbours inside 8 Å of every atom
with their 41 Gaussian distance features, all from ONE ``ops.knn_graph`` launch (pymatgen's ``get_all_neighbors``, the sort,
the cut and ``GaussianDistance.expand`` of the reference; no pymatgen / mendeleev / sklearn / ASE) — and ``load_elem_feats``
standardises an element-embedding table the way sklearn's ``scale`` does.  structures -> build_edos_all -> DeviceDataset ->
Trainer / Predictor.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import json
import re

import numpy as np
import torch

from . import ops, spectra
from ._lib import DosxError
from .synth import E_BINS

SYMBOLS = ("H He Li Be B C N O F Ne Na Mg Al Si P S Cl Ar K Ca Sc Ti V Cr Mn Fe Co Ni Cu Zn Ga Ge As Se Br Kr Rb Sr Y Zr "
           "Nb Mo Tc Ru Rh Pd Ag Cd In Sn Sb Te I Xe Cs Ba La Ce Pr Nd Pm Sm Eu Gd Tb Dy Ho Er Tm Yb Lu Hf Ta W Re Os Ir Pt "
           "Au Hg Tl Pb Bi Po At Rn Fr Ra Ac Th Pa U Np Pu Am Cm Bk Cf Es Fm Md No Lr Rf Db Sg Bh Hs Mt Ds Rg Cn Nh Fl Mc "
           "Lv Ts Og").split()
# Standard atomic weights, IUPAC 2016 (the table ASE ships as ase.data.atomic_masses and `Atom(Z).mass` returns,
# `utils.py:254-257`); ASE is not available here to pin them — pass ``masses=`` to override.
ATOMIC_MASSES = (
    1.008, 4.002602, 6.94, 9.0121831, 10.81, 12.011, 14.007, 15.999, 18.998403163, 20.1797, 22.98976928, 24.305,
    26.9815385, 28.085, 30.973761998, 32.06, 35.45, 39.948, 39.0983, 40.078, 44.955908, 47.867, 50.9415, 51.9961,
    54.938044, 55.845, 58.933194, 58.6934, 63.546, 65.38, 69.723, 72.630, 74.921595, 78.971, 79.904, 83.798, 85.4678,
    87.62, 88.90584, 91.224, 92.90637, 95.95, 97.90721, 101.07, 102.90550, 106.42, 107.8682, 112.414, 114.818, 118.710,
    121.760, 127.60, 126.90447, 131.293, 132.90545196, 137.327, 138.90547, 140.116, 140.90766, 144.242, 144.91276,
    150.36, 151.964, 157.25, 158.92535, 162.500, 164.93033, 167.259, 168.93422, 173.054, 174.9668, 178.49, 180.94788,
    183.84, 186.207, 190.23, 192.217, 195.084, 196.966569, 200.592, 204.38, 207.2, 208.98040, 208.98243, 209.98715,
    222.01758, 223.01974, 226.02541, 227.02775, 232.0377, 231.03588, 238.02891, 237.04817, 244.06421, 243.06138,
    247.07035, 247.07031, 251.07959, 252.0830, 257.09511, 258.09843, 259.1010, 262.110, 267.122, 268.126, 271.134,
    270.133, 269.1338, 278.156, 281.165, 281.166, 285.177, 286.182, 289.190, 289.194, 293.204, 293.208, 294.214)
# `utils.py:277-290`
CRYSTAL_SYSTEMS = {"Cubic": 0, "Hexagonal": 1, "Tetragonal": 2, "Trigonal": 3, "Orthorhombic": 4, "Monoclinic": 5}
_Z_OF = {s: i for i, s in enumerate(SYMBOLS)}


def _get(entry, key):
    if isinstance(entry, dict):
        return entry[key]
    st = getattr(entry, "structure", None)
    if key == "symbols":
        return list(st.symbols)
    if key == "positions":
        return np.asarray(st.positions)
    if key == "cell":
        return np.asarray(getattr(st.cell, "array", st.cell))
    return getattr(entry, key)


def _derived_systems(entries, mode: str, table: Dict[str, int], lower: bool, symprec: float, device) -> Optional[List[int]]:
    """The ``crystal_system=`` modes of ``build_data_all`` / ``build_edos_all``: None for "given" (the labels are read entry by
    entry as before), else one code per entry from ``symmetry.resolve_labels`` ("derive": where the entry carries no label,
    "check": everywhere, a mismatch or an INCONSISTENT crystal raises)."""
    if mode == "given":
        return None
    from . import symmetry

    def name(e):
        v = e.get("crystal_system") if isinstance(e, dict) else getattr(e, "crystal_system", None)
        return None if v is None or str(v) == "" else (str(v).lower() if lower else v)

    names = [name(e) for e in entries]
    return symmetry.resolve_labels(entries, mode, [table.get(v, 6) for v in names], [v is not None for v in names],
                                   symprec=symprec, device=device)


def _field(entry, key):
    """``entry[key]`` / ``entry.key``, None when the entry has none."""
    return entry.get(key) if isinstance(entry, dict) else getattr(entry, key, None)


def _raw_targets(which: List[int], energies, values, targets, kind: str, dev, shift=None, normalize: bool = True):
    """One ``spectra.broaden`` launch for the entries ``which``; a spectrum that cannot be turned into a target raises, with the
    entry's index in place of its position in the launch."""
    if targets.on_uncovered not in ("raise", "keep"):
        raise ValueError(f"on_uncovered must be 'raise' or 'keep', got {targets.on_uncovered!r}")
    res = spectra.broaden(energies, values, targets.grid, targets.sigma, shift=shift, kind=kind, cutoff=targets.cutoff,
                          normalize=normalize, device=dev)
    try:
        res.report.raise_if_bad(uncovered=targets.on_uncovered == "raise")
    except DosxError as err:
        raise DosxError(re.sub(r"crystal (\d+):", lambda m: f"crystal {which[int(m.group(1))]}:", str(err), count=1)) from None
    return res


def build_data_all(entries: Sequence, r_max: float = 5.0, device="cuda:0", masses: Optional[Sequence[float]] = None,
                   dtype: torch.dtype = torch.float64, crystal_system: str = "given", symprec: float = 0.1,
                   targets=None) -> List[Dict[str, object]]:
    """`utils.py:249-303` for a whole dataset at once.  Returns one dict per entry with the reference's ``Data``
    fields: pos, lattice, symbol, x, z, edge_index (row 0 = central atom, row 1 = neighbour), edge_shift, edge_vec,
    edge_len (rounded to 2 decimals, `:276`), phdos [1,51], system, mp_id — host tensors, ``dtype`` floating point.
    ``crystal_system``: "given" reads ``entry.crystal_system`` (an unknown name is code 6, as in the reference); "derive" labels
    the entries that carry none from their structure (``symmetry.crystal_systems`` at ``symprec``); "check" derives every label
    and raises on the first that disagrees.  Both raise on a crystal whose operations match no point group.
    ``targets``: a ``spectra.PhononTargets(grid, sigma)`` builds ``phdos [1, grid.bins]`` for every entry that carries none, from
    its ``frequencies`` (mode frequencies, with optional ``weights``: points) or from ``dos = {"energies", "densities"}`` (a
    tabulated curve), one ``spectra.broaden`` launch per kind.  A spectrum with non-finite or unsorted samples raises; a curve
    that ends inside the window raises unless ``on_uncovered="keep"``, and such an entry's dict says so in ``covered`` (a bool
    tensor, present on built entries only).  An entry with a finished ``phdos`` keeps it; None (default) reads ``entry.phdos``
    as before."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("build_data_all runs the neighbour search on an MI355X through libdosx (no CPU fallback)")
    entries = list(entries)
    if not entries:
        return []
    derived = _derived_systems(entries, crystal_system, CRYSTAL_SYSTEMS, False, symprec, dev)
    mass = torch.tensor(ATOMIC_MASSES if masses is None else list(masses), dtype=torch.float64)
    if mass.numel() != len(SYMBOLS):
        raise ValueError(f"masses must have {len(SYMBOLS)} entries")
    sym = [list(_get(e, "symbols")) for e in entries]
    pos = [np.asarray(_get(e, "positions"), np.float64).reshape(-1, 3) for e in entries]
    cell = np.stack([np.asarray(_get(e, "cell"), np.float64).reshape(3, 3) for e in entries])
    n = np.array([p.shape[0] for p in pos], np.int64)
    for s, p in zip(sym, pos):
        if len(s) != p.shape[0] or p.shape[0] == 0:
            raise ValueError("every entry needs >= 1 atom and one symbol per position")
    atom_ptr = np.concatenate([[0], np.cumsum(n)])
    nl = ops.neighbor_list(torch.from_numpy(np.concatenate(pos)).to(dev), torch.from_numpy(cell).to(dev),
                           torch.from_numpy(atom_ptr.astype(np.int32)).to(dev), float(r_max), self_interaction=True)
    src, dst = nl["src"].cpu().long(), nl["dst"].cpu().long()
    shift, vec, eptr = nl["shift"].cpu(), nl["edge_vec"].cpu(), nl["edge_ptr"].cpu().tolist()
    eye = torch.eye(len(SYMBOLS), dtype=dtype)
    built = {}                                      # entry index -> (phdos [S] float64, covered), from raw spectra
    if targets is not None:
        raw = [c for c, e in enumerate(entries) if _field(e, "phdos") is None]
        modes = [c for c in raw if _field(entries[c], "frequencies") is not None]
        curves = [c for c in raw if c not in modes and _field(entries[c], "dos") is not None]
        if len(modes) + len(curves) != len(raw):
            missing = next(c for c in raw if c not in modes and c not in curves)
            raise ValueError(f"entry {missing}: no phdos, no frequencies and no dos to build one from")
        if modes:
            freq = [np.asarray(_field(entries[c], "frequencies"), np.float64).reshape(-1) for c in modes]
            wts = [np.ones_like(f) if _field(entries[c], "weights") is None else
                   np.asarray(_field(entries[c], "weights"), np.float64).reshape(-1) for c, f in zip(modes, freq)]
            res = _raw_targets(modes, freq, wts, targets, "points", dev, normalize=targets.normalize)
            rows = (res.y_norm if targets.normalize else res.y).cpu()
            built.update({c: (rows[k].clone(), res.report.covered[k].clone()) for k, c in enumerate(modes)})
        if curves:
            dos = [_field(entries[c], "dos") for c in curves]
            res = _raw_targets(curves, [d["energies"] for d in dos], [d["densities"] for d in dos], targets, "curve", dev,
                               normalize=targets.normalize)
            rows = (res.y_norm if targets.normalize else res.y).cpu()
            built.update({c: (rows[k].clone(), res.report.covered[k].clone()) for k, c in enumerate(curves)})
    out = []
    for c, e in enumerate(entries):
        z = torch.tensor([_Z_OF[s] for s in sym[c]], dtype=torch.int64)
        a, b = eptr[c], eptr[c + 1]
        ev = vec[a:b]
        x = torch.zeros(len(z), len(SYMBOLS), dtype=dtype)
        x[torch.arange(len(z)), z] = mass[z].to(dtype)
        system = CRYSTAL_SYSTEMS.get(_get(e, "crystal_system"), 6) if derived is None else derived[c]
        out.append({
            "pos": torch.from_numpy(pos[c]).to(dtype), "lattice": torch.from_numpy(cell[c]).to(dtype).unsqueeze(0),
            "symbol": sym[c], "x": x, "z": eye[z],
            "edge_index": torch.stack([src[a:b], dst[a:b]], 0),
            "edge_shift": shift[a:b].to(dtype), "edge_vec": ev.to(dtype),
            "edge_len": torch.from_numpy(np.around(ev.norm(dim=1).numpy(), decimals=2)),
            "phdos": (built[c][0] if c in built else torch.as_tensor(np.asarray(_get(e, "phdos"), np.float64))).reshape(1, -1).to(dtype),
            "system": torch.tensor(system), "mp_id": _get(e, "mp_id"),
        })
        if c in built:
            out[-1]["covered"] = built[c][1]
    return out


# `data/mat2graph.py:94-107` (lower-case names there; matched case-insensitively here)
_SYSTEM_CODES = {k.lower(): v for k, v in CRYSTAL_SYSTEMS.items()}


def load_elem_feats(path_or_mapping, symbols: Sequence[str] = tuple(SYMBOLS[:100])) -> np.ndarray:
    """`data/mat2graph.py:33-47`: a JSON file (or a dict) ``{symbol: vector}`` -> the ``[len(symbols), F]`` float64 table of
    the first 100 elements, column-standardised like sklearn's ``scale`` (mean 0, population standard deviation 1; a
    zero-variance column is divided by 1).  No table ships with the package (the matscholar embedding is the reference's
    asset)."""
    if isinstance(path_or_mapping, dict):
        embs = path_or_mapping
    else:
        with open(path_or_mapping) as f:
            embs = json.load(f)
    missing = [s for s in symbols if s not in embs]
    if missing:
        raise ValueError(f"element table has no entry for {missing[:5]}{' ...' if len(missing) > 5 else ''}")
    tab = np.vstack([np.asarray(embs[s], np.float64) for s in symbols])
    std = tab.std(axis=0)
    std[std < 10 * np.finfo(np.float64).eps] = 1.0
    return (tab - tab.mean(axis=0)) / std


def build_edos_all(entries: Sequence[dict], elem_feats, radius: float = 8.0, max_num_nbr: int = 12, step: float = 0.2,
                   device="cuda:0", normalize_target: bool = True, crystal_system: str = "given",
                   symprec: float = 0.1, targets=None) -> List[Dict[str, object]]:
    """`data/mat2graph.py:81-107,120-243` for a whole dataset at once.  ``entries``: dicts with ``numbers`` (Z) or
    ``symbols``, ``positions`` (Cartesian), ``cell`` (rows = lattice vectors) and optionally ``glob`` ([energy_per_atom,
    formation_energy_per_atom]), ``crystal_system`` (name, any case), ``y_ft``, ``y``, ``mp_id``.  ``elem_feats [Zmax, F]``:
    the standardised element table (``load_elem_feats``).  Returns one host dict per entry in the schema of
    ``synth.edos_crystal``: x [n+1, F] fp32 (last row = the zero prompt node, `:155-158`, in no edge), edge_index
    [2, K*n] int64 (row 0 = atom i K times, row 1 = its neighbours by rank; a padded rank points at atom 0, `:222-227`),
    edge_attr [K*n, G] fp32, glob [2], system, y_ft [201] (divided by its maximum when ``normalize_target``, `:86-88`; zeros
    when the entry has none), y_max, mp_id, pos — and y when the entry has one.  The order inside a distance tie is the key of
    include/dosx.h (DosxKnn); the reference leaves it to pymatgen.  ``crystal_system`` / ``symprec``: as in ``build_data_all``
    ("given", "derive" or "check").  ``targets``: a ``spectra.EdosTargets(grid, sigma)`` builds the targets of every entry that
    has ``dos = {"energies", "densities", "efermi"}`` and no ``y_ft``, relative to ``efermi`` on ``grid``: ``y_ft`` = the curve
    broadened by ``sigma`` (``spectra.broaden``; over its maximum when ``normalize_target``) with that maximum as ``y_max``, and
    ``y`` = the raw curve resampled (``spectra.resample``; likewise over its maximum) - one launch each for the whole dataset.  A
    spectrum with non-finite or unsorted samples raises; one that ends inside the window raises unless ``on_uncovered="keep"``,
    and the entry's dict says so in ``covered`` (a bool tensor, present on built entries only).  None (default): as before."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("build_edos_all runs the neighbour selection on an MI355X through libdosx (no CPU fallback)")
    entries = list(entries)
    if not entries:
        return []
    derived = _derived_systems(entries, crystal_system, _SYSTEM_CODES, True, symprec, dev)
    table = torch.as_tensor(np.asarray(elem_feats, np.float64))
    if table.dim() != 2:
        raise ValueError("elem_feats must be a [Z, F] table")
    K = int(max_num_nbr)
    numbers, pos = [], []
    for c, e in enumerate(entries):
        z = np.asarray(e["numbers"], np.int64) if "numbers" in e else \
            np.array([_Z_OF.get(s, -1) + 1 for s in e["symbols"]], np.int64)
        p = np.asarray(e["positions"], np.float64).reshape(-1, 3)
        if z.ndim != 1 or z.shape[0] != p.shape[0] or p.shape[0] == 0:
            raise ValueError(f"entry {c}: needs >= 1 atom and one atomic number per position")
        if z.min() < 1 or z.max() > table.shape[0]:
            raise ValueError(f"entry {c}: atomic number outside the element table (1..{table.shape[0]})")
        numbers.append(z)
        pos.append(p)
    cell = np.stack([np.asarray(e["cell"], np.float64).reshape(3, 3) for e in entries])
    n = np.array([p.shape[0] for p in pos], np.int64)
    atom_ptr = np.concatenate([[0], np.cumsum(n)])
    centers = np.arange(0.0, radius + step, step)                   # GaussianDistance(0, radius, step).filter, `:171,215`
    kg = ops.knn_graph(torch.from_numpy(np.concatenate(pos)).to(dev), torch.from_numpy(cell).to(dev),
                       torch.from_numpy(atom_ptr.astype(np.int32)).to(dev), radius=float(radius), k=K,
                       centers=torch.from_numpy(centers).to(dev), var=float(step))
    nbr = kg["nbr_idx"].cpu().long()
    attr = kg["edge_attr"].cpu()
    built = {}                                      # entry index -> (y_ft, y_max, y, covered), from raw spectra
    if targets is not None:
        raw = [c for c, e in enumerate(entries) if e.get("y_ft") is None and e.get("dos") is not None]
        if raw:
            dos = [entries[c]["dos"] for c in raw]
            es, vs, ef = [d["energies"] for d in dos], [d["densities"] for d in dos], [float(d["efermi"]) for d in dos]
            smooth = _raw_targets(raw, es, vs, targets, "curve", dev, shift=ef, normalize=normalize_target)
            plain = spectra.resample(es, vs, targets.grid, shift=ef, normalize=normalize_target, device=dev)
            y_ft = (smooth.y_norm if normalize_target else smooth.y).float().cpu()
            y_raw = (plain.y_norm if normalize_target else plain.y).float().cpu()
            y_top = smooth.y_max.float().cpu()
            built.update({c: (y_ft[k].clone(), y_top[k].clone(), y_raw[k].clone(), smooth.report.covered[k].clone())
                          for k, c in enumerate(raw)})
    out = []
    for c, e in enumerate(entries):
        a, b, nc = int(atom_ptr[c]), int(atom_ptr[c + 1]), int(n[c])
        x = torch.zeros(nc + 1, table.shape[1], dtype=torch.float32)
        x[:nc] = table[torch.from_numpy(numbers[c] - 1)].float()
        has_y = e.get("y_ft") is not None
        y_ft = torch.tensor(np.asarray(e["y_ft"]), dtype=torch.float32).reshape(-1) if has_y else torch.zeros(E_BINS)
        y_max = y_ft.max() if has_y else torch.tensor(0.0)
        if c in built:                              # (already normalised by the launch that made it)
            y_ft, y_max = built[c][0], built[c][1]
        item = {
            "x": x,
            "edge_index": torch.stack([torch.arange(nc).repeat_interleave(K), nbr[a:b].reshape(-1)], 0),
            "edge_attr": attr[a * K:b * K].clone(),
            "glob": torch.tensor(np.asarray(e["glob"], np.float64), dtype=torch.float32).reshape(2) if e.get("glob") is not None
            else torch.zeros(2),
            "system": torch.tensor(_SYSTEM_CODES.get(str(e.get("crystal_system", "")).lower(), 6) if derived is None else derived[c]),
            "y_ft": y_ft / y_max if has_y and normalize_target else y_ft,
            "y_max": y_max,
            "mp_id": e.get("mp_id", f"entry-{c}"),
            "pos": torch.from_numpy(pos[c]).float(),
        }
        if c in built:
            item["y"], item["covered"] = built[c][2], built[c][3]
        elif e.get("y") is not None:
            y = torch.tensor(np.asarray(e["y"]), dtype=torch.float32).reshape(-1)
            item["y"] = y / y.max() if normalize_target else y
        out.append(item)
    return out
