"""DOS targets from raw spectra (include/dosx.h: DosxSpectra / DosxSpectraInterp).

The reference reads finished targets from a prepared pickle (`data/mat2graph.py:81-92`: the smoothed ``densities_total_1_ft`` and
the raw ``densities_total_1``, both already aligned to the Fermi level, cut to the window and resampled) and never shows how they
are made, so the definition restated in include/dosx.h is the contract.  In short, per crystal, all in float64 with one rounding
per operation as written:

``broaden``   ``y[s] = sum_i (w_i * g) * exp(-0.5 * x * x)``, ``x = (E_s - (e_i - shift)) / sigma``, over the samples with
              ``|x| <= cutoff`` in ascending ``i``; ``g = 1 / (sigma * sqrt(2 pi))``; ``w_i = v_i`` for points (mode frequencies
              with q-point weights) and ``v_i`` times its trapezoid interval for a tabulated curve.
``resample``  linear interpolation of a tabulated curve at ``E_s``, zero outside the curve.

Both return the rows with their maximum, their area, optionally the rows over their maximum, and a report that says which
crystals could not be done honestly: a spectrum that ends inside the window (``covered``), non-finite samples (``bad``), energies
that do not ascend (``unsorted``).  ``broaden`` / ``resample`` run one libdosx launch for the whole dataset (csrc/spectra.hip) on a
GPU ``device``; ``broaden_host`` / ``resample_host`` are the same definition in numpy - the twin the tests hold the kernels to,
and what a CPU ``device`` runs."""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _abi
from ._lib import DosxError

MAX_BINS = 1024
MAX_SAMPLES = 1 << 20
SQRT_2PI = 2.5066282746310002                 # the double nearest sqrt(2 pi), as in csrc/spectra.hip
KINDS = {"points": _abi.DOSX_SPECTRA_POINTS, "curve": _abi.DOSX_SPECTRA_CURVE}


class Grid(NamedTuple):
    """The target grid ``E_s = e0 + de * s``, ``s < bins``.  ``unit`` only labels messages."""
    e0: float
    de: float
    bins: int
    unit: str = "eV"

    @classmethod
    def linspace(cls, lo: float, hi: float, bins: int, unit: str = "eV") -> "Grid":
        """The grid of ``numpy.linspace(lo, hi, bins)`` (first and step; the last point is ``lo + de * (bins - 1)``)."""
        if int(bins) < 2:
            raise ValueError(f"Grid.linspace needs at least 2 bins, got {bins}")
        return cls(float(lo), (float(hi) - float(lo)) / (int(bins) - 1), int(bins), unit)

    def energies(self) -> np.ndarray:
        return self.e0 + self.de * np.arange(self.bins, dtype=np.float64)

    def check(self) -> "Grid":
        if not 1 <= int(self.bins) <= MAX_BINS:
            raise ValueError(f"grid: bins={self.bins} outside [1, {MAX_BINS}]")
        if not (np.isfinite(self.e0) and np.isfinite(self.de)):
            raise ValueError(f"grid: e0={self.e0} de={self.de} must be finite")
        if not (self.de > 0.0 or self.bins == 1):
            raise ValueError(f"grid: de={self.de} must be positive")
        return self


class SpectraReport:
    """What a ``broaden`` / ``resample`` call found, per crystal (host tensors): ``n_inside`` samples inside the window (widened by
    ``cutoff * sigma`` for ``broaden``), ``covered`` (a curve reaches both ends of the window; always true for points), ``bad``
    (non-finite samples, a non-finite shift, a sigma that is not a positive finite number; -1: the crystal's range was not what
    the caller stated), ``unsorted`` (pairs of a curve that do not ascend); ``first`` / ``last``: the shifted ends of each
    spectrum as given (NaN for an empty one)."""

    def __init__(self, report, first, last, grid: Grid, kind: str):
        report = torch.as_tensor(np.asarray(report), dtype=torch.int64).reshape(-1, 4)
        self.n_inside, self.bad, self.unsorted = report[:, 0], report[:, 2], report[:, 3]
        self.covered = report[:, 1] != 0
        self.first = torch.as_tensor(np.asarray(first, np.float64))
        self.last = torch.as_tensor(np.asarray(last, np.float64))
        self.grid, self.kind = grid, kind
        self.refused = (self.bad != 0) | ((self.unsorted != 0) if kind == "curve" else torch.zeros_like(self.covered))

    def describe(self, c: int) -> Optional[str]:
        """Why crystal ``c`` is not an honest target, or None."""
        g, u = self.grid, self.grid.unit
        if int(self.bad[c]) < 0:
            return f"crystal {c}: its sample range is not what the caller stated (n_min, n_max, ptr)"
        if int(self.bad[c]) > 0:
            return f"crystal {c}: {int(self.bad[c])} non-finite sample(s), shift or non-positive sigma"
        if self.kind == "curve" and int(self.unsorted[c]) > 0:
            return f"crystal {c}: energies do not ascend strictly ({int(self.unsorted[c])} pair(s))"
        if not bool(self.covered[c]):
            lo, hi = g.e0, g.e0 + g.de * float(g.bins - 1)
            if float(self.last[c]) < hi:
                return f"crystal {c}: spectrum ends at {float(self.last[c]):.2f} {u}, window reaches {hi:.2f} {u}"
            return f"crystal {c}: spectrum starts at {float(self.first[c]):.2f} {u}, window starts at {lo:.2f} {u}"
        return None

    def raise_if_bad(self, uncovered: bool = True) -> None:
        """Raises a ``DosxError`` that names the first offending crystal and the reason; ``uncovered=False`` lets a spectrum that
        ends inside the window pass (its bins beyond the end are what the definition gives: zero, or the tail of the last
        samples)."""
        wrong = self.refused | (~self.covered if uncovered else torch.zeros_like(self.covered))
        idx = torch.nonzero(wrong).reshape(-1)
        if idx.numel():
            n = int(idx.numel())
            raise DosxError(f"{n} spectr{'a' if n != 1 else 'um'} cannot be turned into targets; first: {self.describe(int(idx[0]))}")


class SpectraResult(NamedTuple):
    """``y [C, bins]``, ``y_max [C]``, ``area [C]`` float64 tensors on the device that computed them, ``y_norm [C, bins]``
    (``y / y_max``, zeros where ``y_max <= 0``; None unless asked for) and the ``SpectraReport``."""
    y: torch.Tensor
    y_max: torch.Tensor
    area: torch.Tensor
    y_norm: Optional[torch.Tensor]
    report: SpectraReport


class EdosTargets(NamedTuple):
    """``featurize.build_edos_all(..., targets=EdosTargets(grid, sigma))``: an entry with ``dos = {"energies", "densities",
    "efermi"}`` and no ``y_ft`` gets ``y_ft`` = the curve broadened by ``sigma`` and ``y`` = the curve resampled, both on ``grid``
    relative to ``efermi``.  ``on_uncovered``: "raise" on a spectrum that ends inside the window, or "keep" it."""
    grid: Grid
    sigma: float
    cutoff: float = 6.0
    on_uncovered: str = "raise"


class PhononTargets(NamedTuple):
    """``featurize.build_data_all(..., targets=PhononTargets(grid, sigma))``: an entry without ``phdos`` gets it from its
    ``frequencies`` (with optional ``weights``; points) or from ``dos = {"energies", "densities"}`` (a curve)."""
    grid: Grid
    sigma: float
    normalize: bool = True
    cutoff: float = 6.0
    on_uncovered: str = "raise"


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def _flatten(energies, values, ptr, kind: str):
    """Lists of per-crystal arrays, or flat arrays plus ``ptr`` -> (ptr [C+1] int32, e [T], v [T] float64)."""
    if kind not in KINDS:
        raise ValueError(f"kind must be 'curve' or 'points', got {kind!r}")
    if ptr is None:
        es = [np.asarray(a, np.float64).reshape(-1) for a in energies]
        vs = [np.asarray(a, np.float64).reshape(-1) for a in values]
        if len(es) != len(vs) or any(a.shape != b.shape for a, b in zip(es, vs)):
            raise ValueError("energies and values must be lists of equally long arrays, one pair per crystal")
        ptr = np.concatenate([[0], np.cumsum([a.shape[0] for a in es])]).astype(np.int64)
        e = np.concatenate(es) if es else np.zeros(0)
        v = np.concatenate(vs) if vs else np.zeros(0)
    else:
        e, v = np.asarray(energies, np.float64).reshape(-1), np.asarray(values, np.float64).reshape(-1)
        ptr = np.asarray(ptr, np.int64).reshape(-1)
        if e.shape != v.shape or ptr.size < 1 or ptr[0] != 0 or ptr[-1] != e.shape[0] or (np.diff(ptr) < 0).any():
            raise ValueError("ptr must ascend from 0 to len(energies) == len(values)")
    n = np.diff(ptr)
    if n.size == 0:
        raise ValueError("no crystals")
    if kind == "curve" and n.min() < 2:
        raise ValueError(f"crystal {int(np.argmin(n))}: a curve needs at least 2 samples, got {int(n.min())}")
    if n.max() >= MAX_SAMPLES:
        raise ValueError(f"crystal {int(np.argmax(n))}: {int(n.max())} samples, the limit is {MAX_SAMPLES - 1}")
    return ptr.astype(np.int32), np.ascontiguousarray(e), np.ascontiguousarray(v)


def _per_crystal(x, C: int, name: str, default: float = 0.0) -> np.ndarray:
    """A scalar or one value per crystal -> [C] float64."""
    if x is None:
        return np.full(C, default, np.float64)
    a = np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x, np.float64)
    if a.ndim == 0:
        return np.full(C, float(a), np.float64)
    if a.shape != (C,):
        raise ValueError(f"{name} must be a scalar or one value per crystal ({C}), got shape {a.shape}")
    return np.ascontiguousarray(a)


def _ends(ptr, e, shift):
    """The shifted first and last sample of every crystal (NaN for an empty one), for the report's messages."""
    n = np.diff(ptr)
    first, last = np.full(n.shape, np.nan), np.full(n.shape, np.nan)
    has = n > 0
    first[has] = e[ptr[:-1][has]] - shift[has]
    last[has] = e[ptr[1:][has] - 1] - shift[has]
    return first, last


def _cutoff(cutoff: float) -> float:
    cutoff = float(cutoff)
    if not (cutoff > 0.0 and np.isfinite(cutoff)):
        raise ValueError(f"cutoff must be positive and finite ({cutoff})")
    return cutoff


# ---- the numpy twins of the two kernels ------------------------------------------------------------------------------------
def _finish_rows(y: np.ndarray, report: np.ndarray, refused: np.ndarray, de: float, normalize: bool):
    """The shared epilogue: NaN rows for refused crystals, y_max, area = de * (ascending sum), y_norm."""
    y[refused] = np.nan
    y_max = y.max(axis=1)
    area = de * np.cumsum(y, axis=1)[:, -1]             # cumsum adds in ascending s, one rounding per addition
    y_norm = None
    if normalize:
        with np.errstate(invalid="ignore", divide="ignore"):
            y_norm = np.where((y_max > 0.0)[:, None], y / y_max[:, None], 0.0)
        y_norm[refused] = np.nan
    return y, y_max, area, y_norm


def _weights(e: np.ndarray, v: np.ndarray, curve: bool) -> np.ndarray:
    if not curve:
        return v
    left = np.concatenate([e[:1], e[:-1]])              # e_{i-1}, e_0 for the first sample
    right = np.concatenate([e[1:], e[-1:]])             # e_{i+1}, e_{n-1} for the last one
    return v * (0.5 * (right - left))


def broaden_rows_host(ptr, e, v, shift, sigma, grid: Grid, cutoff: float, kind: str, normalize: bool = False,
                      details: bool = False, vectorized: bool = False):
    """Twin of ``dosx_spectra_broaden`` on flat numpy inputs: ``(y, y_max, area, y_norm, report [C, 4])``; with ``details`` also
    ``A [C, bins]`` = the sum of ``|t_i|`` over the kept terms and ``n_kept [C, bins]`` (what the tests' error bar is made of).
    ``vectorized`` forms every crystal's ``[n, bins]`` term matrix at once and lets numpy sum it (pairwise, so the last bits may
    differ from the contract's ascending order): the fast form, for timing."""
    curve = kind == "curve"
    E = grid.energies()
    C, S = len(ptr) - 1, grid.bins
    y, A, n_kept = np.zeros((C, S)), np.zeros((C, S)), np.zeros((C, S), np.int64)
    report = np.zeros((C, 4), np.int32)
    with np.errstate(all="ignore"):
        for c in range(C):
            ec_raw, vc = e[ptr[c]:ptr[c + 1]], v[ptr[c]:ptr[c + 1]]
            sg, sh = sigma[c], shift[c]
            ec = ec_raw - sh
            reach = cutoff * sg
            lo, hi = E[0] - reach, E[-1] + reach
            g = 1.0 / (sg * SQRT_2PI)
            wg = _weights(ec_raw, vc, curve) * g
            report[c, 0] = int(((lo <= ec) & (ec <= hi)).sum())
            report[c, 1] = int(ec[0] <= E[0] and ec[-1] >= E[-1]) if curve else 1
            report[c, 2] = int((~(np.isfinite(ec_raw) & np.isfinite(vc))).sum()) + int(not (sg > 0.0 and np.isfinite(sg))) \
                + int(not np.isfinite(sh))
            report[c, 3] = int((ec_raw[1:] <= ec_raw[:-1]).sum()) if curve else 0
            if vectorized:
                x = (E[None, :] - ec[:, None]) / sg
                t = np.where(np.abs(x) <= cutoff, wg[:, None] * np.exp(-0.5 * (x * x)), 0.0)
                y[c] = t.sum(0)
                continue
            for i in range(ec.shape[0]):
                x = (E - ec[i]) / sg
                keep = np.abs(x) <= cutoff
                t = wg[i] * np.exp(-0.5 * (x[keep] * x[keep]))
                y[c, keep] += t
                if details:
                    A[c, keep] += np.abs(t)
                    n_kept[c, keep] += 1
    refused = (report[:, 2] != 0) | (report[:, 3] != 0)
    out = _finish_rows(y, report, refused, grid.de, normalize) + (report,)
    return out + (A, n_kept) if details else out


def interp_rows_host(ptr, e, v, shift, grid: Grid, normalize: bool = False):
    """Twin of ``dosx_spectra_interp`` on flat numpy inputs: ``(y, y_max, area, y_norm, report [C, 4])``."""
    E = grid.energies()
    C, S = len(ptr) - 1, grid.bins
    y = np.zeros((C, S))
    report = np.zeros((C, 4), np.int32)
    with np.errstate(all="ignore"):
        for c in range(C):
            ec_raw, vc = e[ptr[c]:ptr[c + 1]], v[ptr[c]:ptr[c + 1]]
            sh = shift[c]
            ec = ec_raw - sh
            n = ec.shape[0]
            report[c, 0] = int(((E[0] <= ec) & (ec <= E[-1])).sum())
            report[c, 1] = int(ec[0] <= E[0] and ec[-1] >= E[-1])
            report[c, 2] = int((~(np.isfinite(ec_raw) & np.isfinite(vc))).sum()) + int(not np.isfinite(sh))
            report[c, 3] = int((ec_raw[1:] <= ec_raw[:-1]).sum())
            if report[c, 2] or report[c, 3]:
                continue                                            # (searchsorted needs ascending finite ec)
            inside = (E >= ec[0]) & (E <= ec[-1])
            j = np.searchsorted(ec, E[inside], side="right") - 1    # the last index with ec_j <= E_s
            at_end = j == n - 1
            jj = np.where(at_end, n - 2, j)
            val = vc[jj] + (vc[jj + 1] - vc[jj]) * ((E[inside] - ec[jj]) / (ec[jj + 1] - ec[jj]))
            y[c, inside] = np.where(at_end, vc[n - 1], val)
    refused = (report[:, 2] != 0) | (report[:, 3] != 0)
    return _finish_rows(y, report, refused, grid.de, normalize) + (report,)


# ---- the public interface --------------------------------------------------------------------------------------------------
def _result(rows, ptr, e, shift, grid, kind, device) -> SpectraResult:
    y, y_max, area, y_norm, report = rows[:5]
    t = lambda a: None if a is None else (a if isinstance(a, torch.Tensor) else torch.from_numpy(a).to(device))
    rep = report.cpu().numpy() if isinstance(report, torch.Tensor) else report
    return SpectraResult(t(y), t(y_max), t(area), t(y_norm), SpectraReport(rep, *_ends(ptr, e, shift), grid, kind))


def broaden_host(energies, values, grid: Grid, sigma, shift=None, kind: str = "curve", cutoff: float = 6.0,
                 normalize: bool = False, ptr=None) -> SpectraResult:
    """The definition of ``broaden`` in numpy."""
    return broaden(energies, values, grid, sigma, shift, kind, cutoff, normalize, device="cpu", ptr=ptr)


def resample_host(energies, values, grid: Grid, shift=None, normalize: bool = False, ptr=None) -> SpectraResult:
    """The definition of ``resample`` in numpy."""
    return resample(energies, values, grid, shift, normalize, device="cpu", ptr=ptr)


def broaden(energies, values, grid: Grid, sigma, shift=None, kind: str = "curve", cutoff: float = 6.0, normalize: bool = False,
            device="cuda:0", ptr=None) -> SpectraResult:
    """Gaussian broadening of raw spectra onto ``grid``.  ``energies`` / ``values``: lists of per-crystal arrays, or flat arrays
    plus ``ptr [C+1]``.  ``kind="curve"``: ``values`` is a density tabulated on strictly ascending ``energies`` (trapezoid
    weights); ``kind="points"``: delta peaks of weight ``values`` (any order, none allowed).  ``sigma`` (the Gaussian's standard
    deviation) and ``shift`` (subtracted from the energies: the Fermi level) are a scalar or one value per crystal.  Terms beyond
    ``cutoff`` standard deviations are dropped.  One launch for all crystals on a GPU ``device``, the numpy twin on a CPU one."""
    grid = Grid(*grid).check()
    cutoff = _cutoff(cutoff)
    ptr, e, v = _flatten(energies, values, ptr, kind)
    C = ptr.shape[0] - 1
    sg, sh = _per_crystal(sigma, C, "sigma"), _per_crystal(shift, C, "shift")
    dev = torch.device(device)
    if dev.type != "cuda":
        return _result(broaden_rows_host(ptr, e, v, sh, sg, grid, cutoff, kind, normalize), ptr, e, sh, grid, kind, dev)
    from . import ops
    n = np.diff(ptr)
    up = lambda a: torch.from_numpy(a).to(dev)
    out = ops.spectra_broaden(up(ptr), up(e), up(v), up(sh), up(sg), grid.e0, grid.de, grid.bins, int(n.min()), int(n.max()),
                              kind=KINDS[kind], cutoff=cutoff, normalize=normalize)
    return _result((out["y"], out["y_max"], out["area"], out.get("y_norm"), out["report"]), ptr, e, sh, grid, kind, dev)


def resample(energies, values, grid: Grid, shift=None, normalize: bool = False, device="cuda:0", ptr=None) -> SpectraResult:
    """Linear interpolation of tabulated curves at the points of ``grid`` (zero outside each curve); arguments as ``broaden``."""
    grid = Grid(*grid).check()
    ptr, e, v = _flatten(energies, values, ptr, "curve")
    sh = _per_crystal(shift, ptr.shape[0] - 1, "shift")
    dev = torch.device(device)
    if dev.type != "cuda":
        return _result(interp_rows_host(ptr, e, v, sh, grid, normalize), ptr, e, sh, grid, "curve", dev)
    from . import ops
    n = np.diff(ptr)
    up = lambda a: torch.from_numpy(a).to(dev)
    out = ops.spectra_interp(up(ptr), up(e), up(v), up(sh), grid.e0, grid.de, grid.bins, int(n.min()), int(n.max()),
                             normalize=normalize)
    return _result((out["y"], out["y_max"], out["area"], out.get("y_norm"), out["report"]), ptr, e, sh, grid, "curve", dev)
