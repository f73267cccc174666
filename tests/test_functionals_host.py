"""dostransformer_amd/functionals.py without a GPU: the builders against closed forms, what the ``Functionals`` constructor
checks, and the trainers' constructor refusals for ``functionals=`` / ``functional_kind=`` / ``functional_weight=``."""
import math

import pytest
import torch

from tests.test_loss_rows_abi import _phonon, _trainers


def _F():
    from dostransformer_amd import functionals
    return functionals


# ---- the builders -----------------------------------------------------------------------------------------------------------------
def test_cumulative_is_cumsum():
    F = _F()
    g = torch.Generator().manual_seed(0)
    for S, de in ((1, 1.0), (7, 0.25), (51, 1.0), (201, 0.125)):
        fn = F.cumulative(S, de)
        assert fn.table.shape == (S, S) and fn.table.dtype == torch.float64 and fn.K == S == fn.S and len(fn.names) == S
        p = torch.rand(3, S, generator=g, dtype=torch.float64)
        assert torch.allclose(p @ fn.table.T, torch.cumsum(p, 1) * de, rtol=1e-14, atol=0)
    assert torch.equal(F.cumulative(4).table, torch.tril(torch.ones(4, 4, dtype=torch.float64)))
    for bad in (0, -2):
        with pytest.raises(ValueError, match="S must be positive"):
            F.cumulative(bad)
    for bad in (0.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="de"):
            F.cumulative(5, bad)


def test_moments_of_a_delta_are_powers_of_its_energy():
    F = _F()
    e = torch.linspace(-3.0, 5.0, 33, dtype=torch.float64)
    de = float(e[1] - e[0])
    fn = F.moments(e, orders=(0, 1, 2, 3))
    assert fn.names == ["m0", "m1", "m2", "m3"] and fn.ratios == [("centre", 1, 0)]
    for s in (0, 11, 32):
        delta = torch.zeros(33, dtype=torch.float64)
        delta[s] = 1.0 / de                                    # a unit of states in bin s
        got = fn.table @ delta
        want = torch.stack([e[s] ** n for n in range(4)])
        assert torch.allclose(got, want, rtol=1e-13, atol=1e-13), (s, got, want)
    assert F.moments(e, orders=(2,)).ratios == []
    assert torch.equal(F.moments(e, orders=(1,), de=2.0).table[0], e * 2.0)
    with pytest.raises(ValueError, match="orders"):
        F.moments(e, orders=(0, 0))
    with pytest.raises(ValueError, match="orders"):
        F.moments(e, orders=(-1,))
    with pytest.raises(ValueError, match="pass de"):
        F.moments([1.0])


def test_window_counts_the_bins_inside():
    F = _F()
    e = torch.arange(10, dtype=torch.float64)
    fn = F.window(e, 2.0, 4.5)
    assert fn.K == 1 and fn.table[0].tolist() == [0, 0, 1, 1, 1, 0, 0, 0, 0, 0]
    assert F.window(e, 2.0, 2.0, de=0.5).table[0].tolist() == [0, 0, 0.5, 0, 0, 0, 0, 0, 0, 0]
    with pytest.raises(ValueError, match="lo="):
        F.window(e, 3.0, 2.0)


def test_heat_capacity_weights():
    F = _F()
    # x = 1 exactly: nu = T / c2
    T = 300.0
    nu = torch.tensor([0.0, T / F.C2, 1000.0, 4000.0], dtype=torch.float64)
    fn = F.heat_capacity(nu, [T], de=1.0)
    w = fn.table[0]
    assert fn.names == ["cv[300K]"]
    assert float(w[0]) == 1.0                                                  # finite at nu = 0: the limit
    assert math.isclose(float(w[1]), math.e / (math.e - 1.0) ** 2, rel_tol=1e-14)
    x = F.C2 * 1000.0 / T
    assert math.isclose(float(w[2]), x * x * math.exp(x) / (math.exp(x) - 1.0) ** 2, rel_tol=1e-13)
    assert bool(torch.isfinite(w).all()) and bool((w[1:] < 1.0).all()) and bool((w > 0).all())
    # tends to 1 as T grows (1 - x^2 / 12), monotonically; finite for x in the hundreds (no inf / inf)
    hot = F.heat_capacity(nu, [1e3, 1e5, 1e7, 1e12], de=1.0).table
    assert bool((hot[1:] >= hot[:-1]).all()) and bool((hot <= 1.0).all())
    assert torch.allclose(hot[2], 1.0 - (F.C2 * nu / 1e7) ** 2 / 12.0, rtol=0, atol=1e-12) and bool((hot[3] == 1.0).all())
    cold = F.heat_capacity(nu, [0.5], de=1.0).table[0]
    assert bool(torch.isfinite(cold).all()) and float(cold[0]) == 1.0 and float(cold[3]) == 0.0
    # de scales the rows; the default is the grid's mean spacing
    assert torch.equal(F.heat_capacity(nu, [T], de=2.0).table, 2.0 * fn.table)
    assert torch.equal(F.heat_capacity(torch.arange(5.0) * 3.0, [T]).table, F.heat_capacity(torch.arange(5.0) * 3.0, [T], de=3.0).table)
    for bad in ([0.0], [-1.0], [math.nan], []):
        with pytest.raises(ValueError, match="temperatures"):
            F.heat_capacity(nu, bad, de=1.0)
    with pytest.raises(ValueError, match="wavenumbers"):
        F.heat_capacity([-1.0, 1.0], [T])


def test_stack_keeps_names_and_moves_ratios():
    F = _F()
    e = torch.linspace(0.0, 1.0, 6, dtype=torch.float64)
    a, b = F.cumulative(6, 0.2), F.moments(e)
    st = F.stack(a, b, F.window(e, 0.2, 0.6))
    assert st.K == 6 + 3 + 1 and st.S == 6 and st.names[:6] == a.names and st.names[6:9] == b.names
    assert torch.equal(st.table[:6], a.table) and torch.equal(st.table[6:9], b.table)
    assert st.ratios == [("centre", 7, 6)]
    with pytest.raises(ValueError, match="bins"):
        F.stack(a, F.cumulative(5))
    with pytest.raises(ValueError, match="distinct"):
        F.stack(a, a)
    with pytest.raises(ValueError, match="nothing"):
        F.stack()


def test_constructor_checks_shape_and_finiteness():
    F = _F()
    fn = F.Functionals([[1.0, 2.0], [3.0, 4.0], [0.0, 0.0]], ratios=[("q", "f1", 0)])
    assert fn.table.dtype == torch.float64 and fn.names == ["f0", "f1", "f2"] and fn.ratios == [("q", 1, 0)]
    assert torch.equal(fn.scaled(0.5).table, fn.table * 0.5) and fn.scaled(0.5).ratios == fn.ratios
    src = torch.ones(2, 3)
    kept = F.Functionals(src)
    src.zero_()
    assert bool((kept.table == 1).all())                                           # a copy, not a view of the caller's tensor
    for bad in (torch.ones(4), torch.ones(2, 3, 4), torch.ones(0, 4), torch.ones(4, 0)):
        with pytest.raises(ValueError, match="2-D"):
            F.Functionals(bad)
    for v in (math.nan, math.inf, -math.inf):
        t = torch.ones(2, 3)
        t[1, 2] = v
        with pytest.raises(ValueError, match="finite"):
            F.Functionals(t)
    with pytest.raises(ValueError, match="names"):
        F.Functionals(torch.ones(2, 3), names=["a"])
    with pytest.raises(ValueError, match="distinct"):
        F.Functionals(torch.ones(2, 3), names=["a", "a"])
    with pytest.raises(ValueError, match="no row named"):
        F.Functionals(torch.ones(2, 3), ratios=[("q", "zz", 0)])
    with pytest.raises(ValueError, match="row 2"):
        F.Functionals(torch.ones(2, 3), ratios=[("q", 0, 2)])


# ---- the trainers' constructors ---------------------------------------------------------------------------------------------
def test_trainers_take_functionals_with_a_per_crystal_loss_only():
    F = _F()
    cdf = F.cumulative(51)
    for cls, model in _trainers():
        m = model()
        for kw in (dict(functionals=cdf), dict(functionals=cdf.table), dict(functionals=cdf, functional_kind="abs")):
            with pytest.raises(ValueError, match='loss="crystal_rmse"'):
                cls(m, **kw)
        tr = cls(m, loss="crystal_rmse", functionals=cdf.table.float(), functional_kind="abs", functional_weight=0.25)
        assert isinstance(tr.functionals, F.Functionals) and tr.functionals.table.dtype == torch.float64
        assert (tr.functionals.K, tr.functionals.S, tr.functional_kind, tr.functional_weight) == (51, 51, "abs", 0.25)
        hyper = tr.state_dict()["hyper"]
        assert not any("functional" in k for k in hyper) and not any("functional" in k for k in tr.state_dict())
        assert cls(m, loss="mse", functionals=cdf, functional_weight=0).functional_weight == 0.0
        tr = cls(m, loss="mae")
        assert tr.functionals is None
        assert cls(m).functionals is None
        with pytest.raises(ValueError, match="set_functionals"):
            tr.set_functionals(cdf)
        for kw in (dict(functional_kind="abs"), dict(functional_weight=0.5)):       # nothing they could apply to
            with pytest.raises(ValueError, match="without functionals"):
                cls(m, loss="mse", **kw)


def test_trainers_refuse_bad_functionals():
    F = _F()
    for cls, model in _trainers():
        m = model()
        for bad, word in ((torch.ones(3, 50), r"\[K,51\]"), (torch.ones(3, 52), r"\[K,51\]"), (torch.ones(51), "2-D"),
                          (torch.ones(513, 51), "at most 512"), (torch.full((2, 51), math.nan), "finite"),
                          (torch.full((2, 51), math.inf), "finite")):
            with pytest.raises(ValueError, match=word):
                cls(m, loss="mse", functionals=bad)
        assert cls(m, loss="mse", functionals=torch.ones(512, 51)).functionals.K == 512
        for kind in ("l2", "SQ", None, 0):
            with pytest.raises(ValueError, match="functional_kind"):
                cls(m, loss="mse", functionals=torch.ones(2, 51), functional_kind=kind)
        for lam in (-1e-3, math.inf, math.nan):
            with pytest.raises(ValueError, match="functional_weight"):
                cls(m, loss="mse", functionals=torch.ones(2, 51), functional_weight=lam)
        # set_functionals: the same shape, checked like the constructor's, held on the host until the first step
        tr = cls(m, loss="mse", functionals=F.cumulative(51))
        tr.set_functionals(F.cumulative(51).scaled(2.0))
        assert float(tr.functionals.table[50, 0]) == 2.0
        for bad, word in ((torch.ones(50, 51), "recorded launches hold its shape"), (torch.ones(51, 50), r"\[K,51\]"),
                          (torch.full((51, 51), math.nan), "finite")):
            with pytest.raises(ValueError, match=word):
                tr.set_functionals(bad)


def test_a_wide_model_is_refused_by_its_bin_count():
    """S beyond 512 in the loss: refused at construction, by the model's own output width."""
    from dostransformer_amd.train import Trainer
    m = _phonon()
    S = int(m._cfg.S)
    assert S == 51
    with pytest.raises(ValueError, match=r"\[K,51\]"):
        Trainer(m, loss="mse", functionals=torch.ones(4, 600))


def test_trainer_refuses_functionals_under_data_parallelism():
    from dostransformer_amd._lib import DosxError
    from dostransformer_amd.train import Trainer
    from tests.gpu_util import _FakeDist
    F = _F()
    with pytest.raises(DosxError, match="single-GPU mode: not with dist"):
        Trainer(_phonon(), dist=_FakeDist(None), functionals=F.cumulative(51))
    with pytest.raises(DosxError, match="single-GPU mode: not with dist"):
        Trainer(_phonon(), dist=_FakeDist(None), loss="mse", functionals=F.cumulative(51))
