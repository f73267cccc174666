"""Normalised functionals without a GPU: the builders of dostransformer_amd/functionals.py against closed forms, the marks through
``stack`` / ``scaled`` / ``device_layout``, the generated binding of dosx_loss_rows_fn_norm / _f64 and their descriptor forms
against the header's argument lists, every refusal of include/dosx.h (-22, a message that starts with the entry's name, before any
launch), and the trainers' constructor and ``set_functionals`` refusals."""
import ctypes as C
import math
import os

import pytest
import torch

from tests.test_loss_functional_abi import B, BW, DPG, DPS, FN, K, LOSSP, PER, PG, PS, S, W, WI, Y
from tests.test_loss_rows_abi import _trainers
from tests.util import dosx_lib as _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEN = 12 << 20                         # never dereferenced, 1 MiB behind the other fake operands
LITERAL = {"dosx_loss_rows_fn_norm": (C.c_float, "dosx_loss_rows_fn", 4), "dosx_loss_rows_fn_norm_f64": (C.c_double, "dosx_loss_rows_fn_f64", 8)}
DESC = {"dosx_loss_rows_fn_norm_desc": (C.c_float, "dosx_loss_rows_w", 4), "dosx_loss_rows_fn_norm_desc_f64": (C.c_double, "dosx_loss_rows_w_f64", 8)}


def _F():
    from dostransformer_amd import functionals
    return functionals


# ---- the builders -----------------------------------------------------------------------------------------------------------------
def test_centre_is_first_moment_over_zeroth():
    F = _F()
    e = torch.linspace(-3.0, 5.0, 41, dtype=torch.float64)
    fn = F.centre(e, 1e-3)
    de = 8.0 / 40
    assert (fn.K, fn.S, fn.K_norm, fn.floor, fn.names) == (1, 41, 1, 1e-3, ["centre"]) and fn.norm_rows == frozenset({0})
    assert torch.equal(fn.table[0], e * de) and torch.equal(fn.denominator, torch.full((41,), de, dtype=torch.float64))
    # a peak that is symmetric about a grid point: that point, whatever the peak's weight
    for j, amp in ((10, 1.0), (27, 7.0)):
        mu = float(e[j])
        p = amp * torch.exp(-0.5 * ((e - mu) / 0.4) ** 2) * ((e - mu).abs() < 1.1)
        assert abs(float(p @ fn.table[0]) / float(p @ fn.denominator) - mu) < 1e-12
    assert torch.equal(F.centre(e, 1e-3, de=0.5).denominator, torch.full((41,), 0.5, dtype=torch.float64))
    assert torch.equal(F.centre(e, 1e-3).table, F.moments(e, orders=(1,)).table)
    for bad in (0.0, -1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="floor"):
            F.centre(e, bad)
    with pytest.raises(TypeError):
        F.centre(e)                                              # the floor is required


def test_normalised_cumulative_has_s_minus_1_rows_over_the_total():
    F = _F()
    g = torch.Generator().manual_seed(0)
    for S_, de in ((2, 1.0), (7, 0.25), (51, 1.0 / 51)):
        fn = F.normalised_cumulative(S_, 1e-6, de)
        assert fn.table.shape == (S_ - 1, S_) and fn.K_norm == fn.K == S_ - 1 and fn.norm_rows == frozenset(range(S_ - 1))
        assert torch.equal(fn.table, F.cumulative(S_, de).table[:S_ - 1]) and torch.equal(fn.denominator, F.cumulative(S_, de).table[S_ - 1])
        p = torch.rand(3, S_, generator=g, dtype=torch.float64) + 0.1
        got = (p @ fn.table.T) / (p @ fn.denominator)[:, None]
        want = (torch.cumsum(p, 1) / p.sum(1, keepdim=True))[:, :S_ - 1]
        assert torch.allclose(got, want, rtol=1e-13, atol=0)
        assert bool((got < 1).all())                             # the row that is identically 1 is left out
    for bad in (1, 0, -3):
        with pytest.raises(ValueError, match="at least 2"):
            F.normalised_cumulative(bad, 1e-3)


def test_normalised_by_a_row_a_vector_or_a_name():
    F = _F()
    nu = torch.linspace(0.0, 400.0, 21, dtype=torch.float64)
    cv, m0 = F.heat_capacity(nu, [50.0, 300.0]), F.moments(nu, orders=(0,))
    a = F.normalised(cv, m0, 1e-2)
    b = F.normalised(cv, m0.table[0], 1e-2)
    assert a.K_norm == 2 and a.names == cv.names and torch.equal(a.table, cv.table) and torch.equal(a.denominator, m0.table[0])
    assert torch.equal(a.denominator, b.denominator) and a.floor == b.floor == 1e-2
    c = F.normalised(F.moments(nu, orders=(0, 1, 2)), "m0", 1e-2)
    assert c.K_norm == 3 and torch.equal(c.denominator, m0.table[0]) and c.ratios == [("centre", 1, 0)]
    with pytest.raises(ValueError, match="ONE plain row"):
        F.normalised(cv, cv, 1e-2)
    with pytest.raises(ValueError, match="ONE plain row"):
        F.normalised(cv, F.centre(nu, 1e-2), 1e-2)
    with pytest.raises(ValueError, match="already"):
        F.normalised(a, m0, 1e-2)
    with pytest.raises(ValueError, match="no row named"):
        F.normalised(cv, "m0", 1e-2)
    with pytest.raises(ValueError, match=r"\[S\]"):
        F.normalised(cv, torch.ones(20), 1e-2)
    with pytest.raises(ValueError, match="finite"):
        F.normalised(cv, torch.full((21,), math.nan), 1e-2)
    for bad in (0.0, -1e-3, math.inf, math.nan):
        with pytest.raises(ValueError, match="floor"):
            F.normalised(cv, m0, bad)


def test_the_constructor_takes_the_three_marks_together():
    F = _F()
    t = torch.ones(3, 4)
    for kw in (dict(denominator=torch.ones(4)), dict(floor=1e-3), dict(denominator=torch.ones(4), floor=1e-3)):
        with pytest.raises(ValueError, match="without norm_rows"):
            F.Functionals(t, **kw)
    for kw in (dict(norm_rows=[1]), dict(norm_rows=[1], floor=1e-3), dict(norm_rows=[1], denominator=torch.ones(4))):
        with pytest.raises(ValueError, match="both a denominator"):
            F.Functionals(t, **kw)
    with pytest.raises(ValueError, match="row 3"):
        F.Functionals(t, denominator=torch.ones(4), norm_rows=[3], floor=1e-3)
    fn = F.Functionals(t, ["a", "b", "c"], denominator=[1, 2, 3, 4], norm_rows=["c", 0], floor=1)
    assert fn.norm_rows == frozenset({0, 2}) and fn.K_norm == 2 and fn.floor == 1.0 and fn.denominator.dtype == torch.float64
    plain = F.Functionals(t)
    assert plain.denominator is None and plain.floor is None and plain.norm_rows == frozenset() and plain.K_norm == 0


def test_stack_keeps_the_marks_and_refuses_two_denominators():
    F = _F()
    e = torch.linspace(0.0, 1.0, 11, dtype=torch.float64)
    m, c, n = F.moments(e, orders=(0, 2)), F.centre(e, 1e-3), F.normalised_cumulative(11, 1e-3, 0.1)
    assert torch.equal(c.denominator.view(torch.int64), n.denominator.view(torch.int64))     # 0.1 both ways, bit for bit
    st = F.stack(m, c, F.window(e, 0.2, 0.4), n)
    assert st.K == 2 + 1 + 1 + 10 and st.norm_rows == frozenset({2} | set(range(4, 14))) and st.K_norm == 11
    assert st.floor == 1e-3 and torch.equal(st.denominator, c.denominator)
    assert st.names[2] == "centre" and st.names[4] == "ncdf0"
    assert F.stack(m, F.window(e, 0.2, 0.4)).K_norm == 0
    with pytest.raises(ValueError, match="different floors"):
        F.stack(c, F.normalised_cumulative(11, 2e-3, 0.1))
    with pytest.raises(ValueError, match="different floors"):
        F.stack(c, F.normalised_cumulative(11, math.nextafter(1e-3, 1.0), 0.1))
    with pytest.raises(ValueError, match="different denominators"):
        F.stack(c, F.normalised_cumulative(11, 1e-3, math.nextafter(0.1, 1.0)))
    with pytest.raises(ValueError, match="different denominators"):
        F.stack(c, F.normalised(m, torch.linspace(1.0, 2.0, 11), 1e-3))
    # scaled(): the rows only
    sc = st.scaled(3.0)
    assert torch.equal(sc.table, st.table * 3.0) and torch.equal(sc.denominator, st.denominator)
    assert (sc.norm_rows, sc.floor, sc.names) == (st.norm_rows, st.floor, st.names)
    assert "K_norm=11" in repr(st) and "K_norm" not in repr(m)


def test_device_layout_puts_the_normalised_rows_last():
    F = _F()
    e = torch.linspace(0.0, 1.0, 11, dtype=torch.float64)
    st = F.stack(F.centre(e, 1e-3), F.moments(e, orders=(0, 2)), F.normalised_cumulative(11, 1e-3, 0.1), F.window(e, 0.2, 0.4))
    table, perm, K_norm = st.device_layout()
    assert K_norm == 11 and perm == [1, 2, 13] + [0] + list(range(3, 13)) and sorted(perm) == list(range(14))
    assert torch.equal(table, st.table[perm]) and table.is_contiguous()
    assert all(p not in st.norm_rows for p in perm[:3]) and all(p in st.norm_rows for p in perm[3:])
    plain = F.cumulative(5)
    table, perm, K_norm = plain.device_layout()
    assert K_norm == 0 and perm == list(range(5)) and torch.equal(table, plain.table)


def test_the_docstrings_say_that_the_scale_is_free():
    F = _F()
    for f in (F.centre, F.normalised_cumulative, F.normalised, F.Functionals):
        assert "scale" in f.__doc__ and ("pointwise" in f.__doc__ or "m0" in f.__doc__), f


# ---- the binding ------------------------------------------------------------------------------------------------------------------
def test_normalised_symbols_declared_exported_and_prototyped():
    _l = _lib()
    lib = _l.load()
    header = open(os.path.join(ROOT, "include", "dosx.h")).read()
    from dostransformer_amd import _abi
    for n, (scalar, linear, _) in LITERAL.items():
        assert f"int {n}(" in header, n
        assert hasattr(lib, n), n
        sig = _l._SIGS[n]
        other = C.c_double if scalar is C.c_float else C.c_float
        assert len(sig) == 25 and sig.count(scalar) == 4 and sig.count(other) == 0, n                # beta, delta, lam, den_floor
        # every argument of the linear entry up to lam, then fn_den, K_norm, den_floor, then the stream
        assert list(sig[:21]) == list(_l._SIGS[linear][:21]), n
        assert list(sig[21:]) == [C.c_void_p, C.c_int, scalar, C.c_void_p], n
        assert list(getattr(lib, n).argtypes) == list(sig)
        # 21 integer-class arguments do not fit a recorded call (include/dosx.h: DosxCall): the descriptor forms are the replayable ones
        assert lib.dosx_replay_op(n.encode(), None, None) == -1, n
    for n, (scalar, weighted, _) in DESC.items():
        assert f"int {n}(" in header, n
        assert hasattr(lib, n), n
        sig = _l._SIGS[n]
        # every argument of the weighted entry up to bin_w, then the descriptor, then the stream
        assert list(sig[:17]) == list(_l._SIGS[weighted][:17]) and len(sig) == 19, n
        assert sig[17]._type_ is _abi.FnNorm and sig[18] is C.c_void_p, n
        ni, nf = C.c_int(0), C.c_int(0)
        assert lib.dosx_replay_op(n.encode(), C.byref(ni), C.byref(nf)) >= 0 and (ni.value, nf.value) == (17, 2), n
    assert [f[0] for f in _abi.FnNorm._fields_] == ["fn_w", "fn_den", "K", "K_norm", "fn_kind", "reserved", "lam", "den_floor"]
    assert C.sizeof(_abi.FnNorm) == 48


def _caller(lib, name):
    """call(a) with a = the literal entry's 24 arguments in front of the stream, through the literal entry or its descriptor form"""
    from dostransformer_amd import _abi
    fn = getattr(lib, name)
    if name in LITERAL:
        return lambda a: fn(*a, None)

    def call(a):
        d = _abi.FnNorm()
        d.fn_w, d.K, d.fn_kind, d.lam, d.fn_den, d.K_norm, d.den_floor = a[17:24]
        return fn(*a[:17], C.byref(d), None)
    return call


@pytest.mark.parametrize("name", list(LITERAL) + list(DESC))
def test_normalised_loss_argument_validation_needs_no_gpu(name):
    lib = _lib().load()
    err = lambda: lib.dosx_last_error().decode()
    esize = {**LITERAL, **DESC}[name][2]
    call = _caller(lib, name)
    # 0 pg, 1 ps, 2 y, 3 B, 4 S, 5 B_global, 6 kind, 7 clamp_target, 8 beta, 9 delta, 10 dpg, 11 dps, 12 per_crystal, 13 loss,
    # 14 w, 15 w_index, 16 bin_w, 17 fn_w, 18 K, 19 fn_kind, 20 lam, 21 fn_den, 22 K_norm, 23 den_floor
    ok = [PG, PS, Y, B, S, B, 0, 0, 1.0, 0.0, DPG, DPS, PER, LOSSP, W, WI, BW, FN, K, 0, 0.5, DEN, 3, 1e-3]

    def refused(a, *words):
        assert call(a) == -22, a
        e = err()
        assert e.startswith(name + ":") and all(w in e for w in words), e

    # ---- what dosx_loss_rows_fn refuses, under this entry's name: with rows to normalise and with none -----------------------------
    for tail in ((DEN, 3, 1e-3), (DEN, K, 1e-3), (None, 0, 1e-3)):
        base = ok[:21] + list(tail)
        for i in (0, 2, 10, 13):
            a = list(base)
            a[i] = None
            refused(a, "NULL")
        for i in (1, 11):
            a = list(base)
            a[i] = None
            refused(a, "ps", "dps")
        for i, word in ((3, "B="), (4, "S="), (5, "B_global=")):
            a = list(base)
            a[i] = 0
            refused(a, word + "0")
        a = list(base)
        a[6] = 4
        refused(a, "kind=4")
        a = list(base)
        a[6], a[9] = 3, 0.0
        refused(a, "HUBER", "delta")
        a = list(base)
        a[14] = None
        refused(a, "w_index", "NULL")
        a = list(base)
        a[16] = PG + esize
        refused(a, "bin_w", "inside")
        for k in (0, 513):
            a = list(base)
            a[18], a[22] = k, min(a[22], max(k, 0))
            refused(a, "K=" + str(k))
        a = list(base)
        a[4] = 513
        refused(a, "S=513")
        a = list(base)
        a[19] = 2
        refused(a, "fn_kind=2")
        for lam in (-1e-3, math.inf, math.nan):
            a = list(base)
            a[20] = lam
            refused(a, "lam")
        a = list(base)
        a[17] = Y + esize
        refused(a, "fn_w", "inside")
    # ---- K_norm outside 0 .. K ----------------------------------------------------------------------------------------------------
    for kn in (-1, -7, K + 1, 1 << 20):
        a = list(ok)
        a[22] = kn
        refused(a, "K_norm=" + str(kn))
    a = list(ok)
    a[17], a[22] = None, -1                                       # (without a table too)
    refused(a, "K_norm=-1")
    # ---- rows to normalise without a denominator row ----------------------------------------------------------------------------
    for kn in (1, K):
        a = list(ok)
        a[21], a[22] = None, kn
        refused(a, "fn_den", "NULL")
    # ---- den_floor not finite or <= 0 (with rows to normalise and with none) -------------------------------------------------------
    for floor in (0.0, -1e-3, -math.inf, math.inf, math.nan):
        for kn in (3, 0):
            a = list(ok)
            a[22], a[23] = kn, floor
            refused(a, "den_floor")
    # ---- fn_den inside a [B,S] operand: at its first, a middle and its last element, and a row that ENDS inside it -----------------
    n = B * S
    for op in (PG, PS, Y, DPG, DPS):
        for off in (0, (n // 2) * esize, (n - 1) * esize, -(S - 1) * esize):
            a = list(ok)
            a[21] = op + off
            refused(a, "fn_den", "inside")
    a = list(ok)                                                  # (one output: ps and dps both NULL - their addresses are no operands)
    a[1] = a[11] = None
    a[21] = PG + esize
    refused(a, "fn_den", "inside")
    if name in DESC:
        assert getattr(lib, name)(*ok[:17], None, None) == -22 and err().startswith(name + ":") and "descriptor" in err()


# ---- the trainers' constructors ---------------------------------------------------------------------------------------------
def test_trainers_take_normalised_functionals_and_refuse_another_count_or_floor():
    F = _F()
    e = (torch.arange(51, dtype=torch.float64) + 0.5) / 51
    fn = F.stack(F.moments(e, orders=(0,), de=1.0 / 51), F.centre(e, 1e-3, de=1.0 / 51), F.normalised_cumulative(51, 1e-3, 1.0 / 51))
    assert (fn.K, fn.K_norm) == (52, 51)
    for cls, model in _trainers():
        m = model()
        with pytest.raises(ValueError, match='loss="crystal_rmse"'):
            cls(m, functionals=fn)
        tr = cls(m, loss="crystal_rmse", functionals=fn, functional_kind="abs", functional_weight=0.25)
        assert tr.functionals is fn and tr.functionals.K_norm == 51 and tr._fn_dev is None       # (on the host until the first step)
        hyper = tr.state_dict()["hyper"]
        assert not any("functional" in k for k in hyper)
        # what the device buffer will hold: the table with the plain row first, the denominator behind it
        host = tr._fn_host(fn)
        assert host.shape == (53, 51) and host.dtype == tr._dtype
        assert torch.equal(host[:52], fn.device_layout()[0].to(tr._dtype)) and torch.equal(host[52], fn.denominator.to(tr._dtype))
        assert torch.equal(tr._fn_host(F.cumulative(51)), F.cumulative(51).table.to(tr._dtype))
        # set_functionals: rows and denominator may change; K, K_norm and the floor may not
        other = F.Functionals(fn.table * 2.0, fn.names, denominator=fn.denominator * 3.0, norm_rows=fn.norm_rows, floor=1e-3)
        tr.set_functionals(other)
        assert tr.functionals is other
        tr.set_functionals(fn.scaled(0.5))
        with pytest.raises(ValueError, match="recorded launches hold its shape"):
            tr.set_functionals(F.normalised_cumulative(51, 1e-3, 1.0 / 51))
        with pytest.raises(ValueError, match="table has 51"):
            tr.set_functionals(F.Functionals(fn.table, fn.names, denominator=fn.denominator, norm_rows=range(2, 52), floor=1e-3))
        with pytest.raises(ValueError, match="table has 51"):
            tr.set_functionals(fn.table)
        with pytest.raises(ValueError, match="floor 0.002"):
            tr.set_functionals(F.Functionals(fn.table, fn.names, denominator=fn.denominator, norm_rows=fn.norm_rows, floor=2e-3))
        with pytest.raises(ValueError, match=r"\[K,51\]"):
            tr.set_functionals(F.normalised_cumulative(50, 1e-3))
        # a plain trainer refuses a table that gained normalised rows
        plain = cls(m, loss="mse", functionals=F.cumulative(51))
        with pytest.raises(ValueError, match="normalised rows"):
            plain.set_functionals(F.normalised(F.cumulative(51), "cdf50", 1e-3))


def test_evaluation_refuses_a_table_with_normalised_rows():
    from dostransformer_amd import evaluate
    F = _F()
    with pytest.raises(ValueError, match="normalised rows"):
        evaluate.functionals_per_crystal(None, F.centre(torch.linspace(0.0, 1.0, 5), 1e-3))
