"""Tables of linear functionals of a density of states, ``F_k(p) = sum_s table[k,s] p_s`` (include/dosx.h: dosx_loss_rows_fn, the
trainers' ``functionals=...``; dosx_eval_functionals, ``evaluate.functionals_per_crystal``): the cumulative DOS, moments, the
states in an energy window and the harmonic heat capacity.  Pure torch on the CPU in float64: they run once, in front of training
or evaluation."""
from __future__ import annotations

from typing import Optional, Sequence

import torch

C2 = 1.438776877                   # the second radiation constant h c / k_B in cm K: x = C2 nu / T for a wavenumber nu in cm^-1


class Functionals:
    """A table ``[K,S]`` (float64, on the host) with the names of its ``K`` rows, and optional ``ratios`` - ``(name, numerator row,
    denominator row)``, rows by name or index - for reporting only (a band centre is first moment / zeroth moment): the loss
    never sees a ratio, ``evaluate.functionals_per_crystal`` forms them in float64 from the table's values."""

    def __init__(self, table, names: Optional[Sequence[str]] = None, ratios=()):
        t = table if torch.is_tensor(table) else torch.as_tensor(table, dtype=torch.float64)
        t = t.detach().to("cpu", torch.float64).clone()
        if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError(f"Functionals: the table must be 2-D [K,S] with K, S >= 1, got shape {tuple(t.shape)}")
        if not bool(torch.isfinite(t).all()):
            raise ValueError("Functionals: every entry of the table must be finite")
        K = int(t.shape[0])
        names = [f"f{k}" for k in range(K)] if names is None else [str(n) for n in names]
        if len(names) != K:
            raise ValueError(f"Functionals: {len(names)} names for {K} rows")
        if len(set(names)) != K:
            raise ValueError("Functionals: the row names must be distinct")
        self.table, self.names = t, names
        self.ratios = []
        for r in ratios:
            name, num, den = r
            self.ratios.append((str(name), self._row(num), self._row(den)))

    def _row(self, r) -> int:
        if isinstance(r, str):
            if r not in self.names:
                raise ValueError(f"Functionals: no row named {r!r} (rows: {self.names})")
            return self.names.index(r)
        k = int(r)
        if not 0 <= k < len(self.names):
            raise ValueError(f"Functionals: row {k} of {len(self.names)}")
        return k

    @property
    def K(self) -> int:
        return int(self.table.shape[0])

    @property
    def S(self) -> int:
        return int(self.table.shape[1])

    def scaled(self, factor: float) -> "Functionals":
        """The same functionals times ``factor`` - under ``"sq"`` the term scales with its square, under ``"abs"`` with it: what a
        schedule hands to ``trainer.set_functionals``."""
        return Functionals(self.table * float(factor), self.names, self.ratios)

    def __repr__(self) -> str:
        return f"Functionals(K={self.K}, S={self.S}, names={self.names[:4]}{'...' if self.K > 4 else ''})"


def _grid(who: str, energies, de):
    e = torch.as_tensor(energies, dtype=torch.float64).detach().to("cpu").reshape(-1)
    if e.numel() < 1 or not bool(torch.isfinite(e).all()):
        raise ValueError(f"functionals.{who}: the grid must hold at least one finite value")
    if de is None:
        if e.numel() < 2:
            raise ValueError(f"functionals.{who}: a one-point grid has no spacing - pass de")
        de = float((e[-1] - e[0]) / (e.numel() - 1))
    de = float(de)
    if not 0.0 < abs(de) < float("inf"):
        raise ValueError(f"functionals.{who}: the bin width de must be finite and non-zero, got {de}")
    return e, de


def cumulative(S: int, de: float = 1.0) -> Functionals:
    """``[S,S]`` lower-triangular ``de``: row k is the cumulative DOS up to and including bin k (``torch.cumsum(p) * de``).  In the
    loss ``"sq"`` is then the Cramer distance between the two cumulative curves, ``"abs"`` their Wasserstein-1 distance."""
    S = int(S)
    if S < 1:
        raise ValueError(f"functionals.cumulative: S must be positive, got {S}")
    if not 0.0 < abs(float(de)) < float("inf"):
        raise ValueError(f"functionals.cumulative: de must be finite and non-zero, got {de}")
    return Functionals(torch.tril(torch.ones(S, S, dtype=torch.float64)) * float(de), [f"cdf{k}" for k in range(S)])


def moments(energies, orders=(0, 1, 2), de: Optional[float] = None) -> Functionals:
    """Row n: ``E_s^n de`` - the raw moments ``int E^n g(E) dE`` on the grid ``energies`` (``de`` default: its mean spacing).  With
    orders 0 and 1 the ratio ``centre = m1 / m0`` is declared (the band centre, or the mean frequency of a phonon DOS)."""
    e, de = _grid("moments", energies, de)
    orders = [int(n) for n in orders]
    if not orders or min(orders) < 0 or len(set(orders)) != len(orders):
        raise ValueError(f"functionals.moments: orders must be distinct integers >= 0, got {orders}")
    names = [f"m{n}" for n in orders]
    ratios = [("centre", "m1", "m0")] if 0 in orders and 1 in orders else []
    return Functionals(torch.stack([e ** n * de for n in orders]), names, ratios)


def window(energies, lo: float, hi: float, de: Optional[float] = None) -> Functionals:
    """One row: ``de`` on the bins with ``lo <= E_s <= hi`` - the states in an energy window, e.g. around the Fermi level."""
    e, de = _grid("window", energies, de)
    lo, hi = float(lo), float(hi)
    if not lo <= hi:
        raise ValueError(f"functionals.window: lo={lo} must not exceed hi={hi}")
    return Functionals((((e >= lo) & (e <= hi)).to(torch.float64) * de)[None, :], [f"window[{lo:g},{hi:g}]"])


def heat_capacity(wavenumbers_cm1, temperatures, de: Optional[float] = None) -> Functionals:
    """Row per temperature T (in K): ``x^2 e^x / (e^x - 1)^2 de`` with ``x = 1.438776877 nu_s / T`` for the phonon grid ``nu`` in
    cm^-1 - the harmonic ``C_V(T)`` per mode in units of k_B, integrated over the DOS.  Written with ``expm1`` as
    ``x^2 / (expm1(x) (1 - exp(-x)))``, with the limit 1 at ``x -> 0`` (``nu = 0``, or T large)."""
    nu, de = _grid("heat_capacity", wavenumbers_cm1, de)
    T = torch.as_tensor(temperatures, dtype=torch.float64).detach().to("cpu").reshape(-1)
    if T.numel() < 1 or not bool(torch.isfinite(T).all()) or not bool((T > 0).all()):
        raise ValueError("functionals.heat_capacity: temperatures must be finite and > 0")
    if bool((nu < 0).any()):
        raise ValueError("functionals.heat_capacity: wavenumbers must be >= 0")
    x = C2 * nu[None, :] / T[:, None]
    small = x < 1e-8                                        # the series 1 - x^2 / 12 + ... is 1 to float64 here
    xs = torch.where(small, torch.ones_like(x), x)
    w = xs * xs / (torch.expm1(xs) * (-torch.expm1(-xs)))   # e^x / (e^x - 1)^2 = 1 / ((e^x - 1) (1 - e^-x)); x large: 0, never inf / inf
    w = torch.where(small, torch.ones_like(x), w)
    return Functionals(w * de, [f"cv[{float(t):g}K]" for t in T])


def stack(*parts: Functionals) -> Functionals:
    """The rows of several tables over the same grid, one after another; names and ratios kept (names must stay distinct)."""
    if not parts:
        raise ValueError("functionals.stack: nothing to stack")
    parts = [p if isinstance(p, Functionals) else Functionals(p) for p in parts]
    S = parts[0].S
    if any(p.S != S for p in parts):
        raise ValueError(f"functionals.stack: the tables have {[p.S for p in parts]} bins")
    names, ratios, off = [], [], 0
    for p in parts:
        names += p.names
        ratios += [(n, a + off, b + off) for n, a, b in p.ratios]
        off += p.K
    return Functionals(torch.cat([p.table for p in parts]), names, ratios)


def as_functionals(fn) -> Functionals:
    """A ``Functionals`` as it is, a ``[K,S]`` tensor (or nested list) wrapped into one."""
    return fn if isinstance(fn, Functionals) else Functionals(fn)

