"""Tables of linear functionals of a density of states, ``F_k(p) = sum_s table[k,s] p_s`` (include/dosx.h: dosx_loss_rows_fn, the
trainers' ``functionals=...``; dosx_eval_functionals, ``evaluate.functionals_per_crystal``): the cumulative DOS, moments, the
states in an energy window and the harmonic heat capacity.  Pure torch on the CPU in float64: they run once, in front of training
or evaluation.

Normalised rows (include/dosx.h: dosx_loss_rows_fn_norm): rows marked as divided by ONE common denominator functional ``D(p) =
sum_s denominator[s] p_s`` with a floor, ``u_k = F_k(p) / max(D(p), floor) - F_k(t) / max(D(t), floor)`` - ``centre`` (a band
centre or mean frequency ``m1 / m0``), ``normalised_cumulative`` (the cumulative curve of the DOS as a shape), or ``normalised``
over any table (``heat_capacity`` over ``m0``: C_V per mode).  A purely normalised objective leaves the SCALE of the prediction
free - ``p`` and ``2 p`` have the same ratios -: the pointwise term of the loss, or a plain ``m0`` row stacked next to the
normalised ones, carries the scale."""
from __future__ import annotations

import struct
from typing import Optional, Sequence

import torch

C2 = 1.438776877                   # the second radiation constant h c / k_B in cm K: x = C2 nu / T for a wavenumber nu in cm^-1


class Functionals:
    """A table ``[K,S]`` (float64, on the host) with the names of its ``K`` rows, and optional ``ratios`` - ``(name, numerator row,
    denominator row)``, rows by name or index - for reporting only (a band centre is first moment / zeroth moment): the loss
    never sees a ratio, ``evaluate.functionals_per_crystal`` forms them in float64 from the table's values.

    ``denominator`` (``[S]``), ``norm_rows`` (a set of rows, by name or index) and ``floor`` (finite, > 0, in the units of ``D``):
    the rows of ``norm_rows`` enter the loss divided by ``max(sum_s denominator[s] p_s, floor)`` on the prediction's and on the
    target's side (module docstring).  All three are given together or not at all; the other rows stay plain.  Rows so marked alone
    leave the scale of the prediction free - keep the pointwise term, or a plain ``m0`` row, next to them."""

    def __init__(self, table, names: Optional[Sequence[str]] = None, ratios=(), denominator=None, norm_rows=(), floor=None):
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
        rows = frozenset(self._row(r) for r in norm_rows)
        if not rows:
            if denominator is not None or floor is not None:
                raise ValueError("Functionals: denominator / floor without norm_rows - there is no row they could apply to")
            self.denominator, self.norm_rows, self.floor = None, rows, None
            return
        if denominator is None or floor is None:
            raise ValueError("Functionals: normalised rows need both a denominator [S] and a floor")
        d = denominator if torch.is_tensor(denominator) else torch.as_tensor(denominator, dtype=torch.float64)
        d = d.detach().to("cpu", torch.float64).clone()
        if d.dim() != 1 or d.numel() != t.shape[1]:
            raise ValueError(f"Functionals: the denominator must be [S] = [{int(t.shape[1])}], got shape {tuple(d.shape)}")
        if not bool(torch.isfinite(d).all()):
            raise ValueError("Functionals: every entry of the denominator must be finite")
        floor = float(floor)
        if not 0.0 < floor < float("inf"):
            raise ValueError(f"Functionals: the floor must be finite and > 0 (in the units of the denominator), got {floor}")
        self.denominator, self.norm_rows, self.floor = d, rows, floor

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

    @property
    def K_norm(self) -> int:
        return len(self.norm_rows)

    def _marks(self) -> dict:
        return {"denominator": self.denominator, "norm_rows": sorted(self.norm_rows), "floor": self.floor}

    def scaled(self, factor: float) -> "Functionals":
        """The same functionals times ``factor`` - under ``"sq"`` the term scales with its square, under ``"abs"`` with it: what a
        schedule hands to ``trainer.set_functionals``.  The ROWS are scaled, normalised ones too (their ratios scale with them);
        the denominator and the floor stay."""
        return Functionals(self.table * float(factor), self.names, self.ratios, **self._marks())

    def device_layout(self):
        """``(table, perm, K_norm)`` as the loss entries take them: the plain rows first and the ``K_norm`` normalised rows last,
        each group in its own order; ``perm[i]`` is the row of ``self.table`` that stands at row ``i`` of the returned table."""
        perm = [k for k in range(self.K) if k not in self.norm_rows] + sorted(self.norm_rows)
        return self.table[perm].contiguous(), perm, self.K_norm

    def __repr__(self) -> str:
        norm = f", K_norm={self.K_norm}, floor={self.floor:g}" if self.norm_rows else ""
        return f"Functionals(K={self.K}, S={self.S}, names={self.names[:4]}{'...' if self.K > 4 else ''}{norm})"


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


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def normalised(fn, by, floor: float) -> Functionals:
    """Every row of ``fn`` divided by the functional ``by`` - a one-row ``Functionals``, an ``[S]`` vector, or the name of a row of
    ``fn`` (that row is then normalised like the others: identically 1 where the floor is not reached) - with ``floor`` (required,
    finite, > 0, in the units of ``by``'s values: below it the denominator is the constant ``floor``).  ``normalised(heat_capacity(
    nu, T), moments(nu, (0,)), floor)`` is C_V per mode.  The result leaves the scale of the prediction free: train it next to the
    pointwise term or stack a plain ``m0`` row onto it."""
    fn = as_functionals(fn)
    if fn.norm_rows:
        raise ValueError("functionals.normalised: the table already has normalised rows - one denominator per table")
    if isinstance(by, str):
        den = fn.table[fn._row(by)]
    elif isinstance(by, Functionals):
        if by.K != 1 or by.norm_rows:
            raise ValueError(f"functionals.normalised: the denominator must be ONE plain row, got {by!r}")
        den = by.table[0]
    else:
        den = torch.as_tensor(by, dtype=torch.float64).detach().to("cpu").reshape(-1) if not torch.is_tensor(by) else by
    return Functionals(fn.table, fn.names, fn.ratios, denominator=den, norm_rows=range(fn.K), floor=floor)


def centre(energies, floor: float, de: Optional[float] = None) -> Functionals:
    """One normalised row ``centre = m1 / m0 = sum_s E_s p_s de / max(sum_s p_s de, floor)``: the band centre of an electronic DOS,
    the mean frequency of a phonon DOS.  ``floor`` is in the units of ``m0`` (states).  The row alone leaves the scale of the
    prediction free: the pointwise term, or a plain ``moments(energies, (0,))`` row, carries it."""
    e, de = _grid("centre", energies, de)
    return Functionals((e * de)[None, :], ["centre"], denominator=torch.full_like(e, de), norm_rows=(0,), floor=floor)


def normalised_cumulative(S: int, floor: float, de: float = 1.0) -> Functionals:
    """``[S - 1, S]``: the cumulative DOS up to and including bins ``0 .. S - 2`` over the total - the cumulative curve of the DOS
    as a SHAPE (``"sq"``: the Cramer distance between the two normalised curves, ``"abs"``: their Wasserstein-1 distance).  The last
    row of ``cumulative(S)`` would be total / total, identically 1 on both sides, and is left out: under ``"abs"`` it would add
    the sign of rounding noise.  The scale of the prediction is free under these rows: keep the pointwise term or a plain ``m0``."""
    S = int(S)
    if S < 2:
        raise ValueError(f"functionals.normalised_cumulative: S must be at least 2 (a one-bin ratio is a constant), got {S}")
    c = cumulative(S, de)
    return Functionals(c.table[:S - 1], [f"ncdf{k}" for k in range(S - 1)], denominator=c.table[S - 1], norm_rows=range(S - 1),
                       floor=floor)


def stack(*parts: Functionals) -> Functionals:
    """The rows of several tables over the same grid, one after another; names, ratios and the normalised marks kept (names must
    stay distinct).  Plain parts stand next to normalised ones; two normalised parts must share ONE denominator and ONE floor,
    compared bit for bit."""
    if not parts:
        raise ValueError("functionals.stack: nothing to stack")
    parts = [p if isinstance(p, Functionals) else Functionals(p) for p in parts]
    S = parts[0].S
    if any(p.S != S for p in parts):
        raise ValueError(f"functionals.stack: the tables have {[p.S for p in parts]} bins")
    names, ratios, rows, off, first = [], [], [], 0, None
    for p in parts:
        names += p.names
        ratios += [(n, a + off, b + off) for n, a, b in p.ratios]
        if p.norm_rows:
            if first is None:
                first = p
            elif not _same_bits(first.denominator, p.denominator):
                raise ValueError("functionals.stack: two parts are normalised by different denominators - a table has one")
            elif struct.pack("<d", first.floor) != struct.pack("<d", p.floor):
                raise ValueError(f"functionals.stack: two parts are normalised with different floors ({first.floor!r} and "
                                 f"{p.floor!r}) - a table has one")
            rows += [k + off for k in p.norm_rows]
        off += p.K
    marks = {} if first is None else {"denominator": first.denominator, "norm_rows": rows, "floor": first.floor}
    return Functionals(torch.cat([p.table for p in parts]), names, ratios, **marks)


def as_functionals(fn) -> Functionals:
    """A ``Functionals`` as it is, a ``[K,S]`` tensor (or nested list) wrapped into one."""
    return fn if isinstance(fn, Functionals) else Functionals(fn)

