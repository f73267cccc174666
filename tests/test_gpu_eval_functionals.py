"""dosx_eval_functionals / dosx_eval_functionals_f64 (csrc/loss_functional.hip) and evaluate.functionals_per_crystal on a real
MI355X against float64 numpy on the same inputs: out[b,0,k] = F_k(pred_b) scale_b, out[b,1,k] = F_k(y_b) scale_b.

The bar: 1e-13 of sum_s |W[k,s] p_s| (times |scale_b|) - float64 products and sums, at most ceil(600 / 64) = 10 additions per
lane and 6 reduction levels, each at most 2^-53 of that magnitude: 16 x 1.1e-16 = 1.8e-15, far inside."""
import numpy as np
import pytest
import torch

from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu

DTYPES = {"f32": torch.float32, "f64": torch.float64}
SENT = -7.25


def _ops():
    from dostransformer_amd import ops
    return ops


def _inputs(B, S, K, dt, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: (2.0 * torch.rand(*s, generator=g, dtype=torch.float64) - 1.0).to(dt)
    return r(B, S), r(B, S), r(K, S), (0.5 + 4.0 * torch.rand(B, generator=g, dtype=torch.float64))


def _host(pred, y, tab, scale):
    """float64 numpy: (values [B,2,K], magnitudes [B,2,K])"""
    p, t, w = (x.double().numpy() for x in (pred, y, tab))
    s = np.ones(p.shape[0]) if scale is None else scale.numpy()
    val = np.stack([p @ w.T, t @ w.T], 1) * s[:, None, None]
    mag = np.stack([np.abs(p) @ np.abs(w).T, np.abs(t) @ np.abs(w).T], 1) * np.abs(s)[:, None, None]
    return val, mag


@pytest.mark.parametrize("dtn", list(DTYPES))
@pytest.mark.parametrize("K", [1, 65])
@pytest.mark.parametrize("S", [1, 63, 64, 65, 201, 600])
def test_eval_functionals_against_float64_numpy(S, K, dtn):
    dt = DTYPES[dtn]
    o = _ops()
    for B in (0, 1, 5):
        pred, y, tab, scale = _inputs(B, S, K, dt, 1000 * S + 10 * K + B)
        for sc in (None, scale):
            # the output inside a larger sentinel-filled buffer: nothing is written around it
            buf = torch.full((B + 2, 2, K), SENT, dtype=torch.float64, device=DEV)
            out = buf[1:B + 1]
            o.eval_functionals(pred.to(DEV), y.to(DEV), tab.to(DEV), out, scale=None if sc is None else sc.to(DEV))
            torch.cuda.synchronize()
            assert bool((buf[0] == SENT).all()) and bool((buf[B + 1] == SENT).all())
            if B == 0:
                continue
            val, mag = _host(pred, y, tab, sc)
            err = np.abs(out.cpu().numpy() - val)
            worst = float((err / mag).max())
            print(f"eval_functionals[{dtn},B{B},S{S},K{K},{'scale' if sc is not None else 'plain'}]: worst error / sum|W p| {worst:.2e}")
            assert worst <= 1e-13
        if B:                                                 # the scale is applied: a row's values are its unscaled ones times it
            a = torch.empty(B, 2, K, dtype=torch.float64, device=DEV)
            o.eval_functionals(pred.to(DEV), y.to(DEV), tab.to(DEV), a)
            assert torch.equal(out, a * scale.to(DEV)[:, None, None])


def test_a_rows_values_do_not_depend_on_the_batch():
    o = _ops()
    pred, y, tab, _ = _inputs(9, 201, 7, torch.float32, 5)
    big, one = torch.empty(9, 2, 7, dtype=torch.float64, device=DEV), torch.empty(1, 2, 7, dtype=torch.float64, device=DEV)
    o.eval_functionals(pred.to(DEV), y.to(DEV), tab.to(DEV), big)
    o.eval_functionals(pred[8:].to(DEV), y[8:].to(DEV), tab.to(DEV), one)
    assert torch.equal(big[8:], one)


def test_wrapper_checks_its_operands():
    o = _ops()
    pred, y, tab, scale = (x.to(DEV) for x in _inputs(3, 51, 4, torch.float32, 1))
    out = torch.empty(3, 2, 4, dtype=torch.float64, device=DEV)
    with pytest.raises(TypeError, match="table"):
        o.eval_functionals(pred, y, tab.double(), out)
    with pytest.raises(TypeError, match="out"):
        o.eval_functionals(pred, y, tab, out.float())
    with pytest.raises(TypeError, match="scale"):
        o.eval_functionals(pred, y, tab, out, scale=scale.float())
    with pytest.raises(TypeError, match="y"):
        o.eval_functionals(pred, y.cpu(), tab, out)
    for bad in (dict(table=tab[:, :50]), dict(out=out[:, :1]), dict(out=out[:2]), dict(scale=scale[:2])):
        kw = {**dict(table=tab, out=out, scale=scale), **bad}
        with pytest.raises(ValueError, match="want"):
            o.eval_functionals(pred, y, kw["table"], kw["out"], scale=kw["scale"])
    with pytest.raises(ValueError, match="contiguous"):
        o.eval_functionals(pred, y, torch.empty(4, 102, device=DEV)[:, ::2], out)


@pytest.mark.parametrize("dtn", list(DTYPES))
def test_functionals_per_crystal_values_errors_and_ratios_against_the_host(dtn):
    """A PerCrystalResult with device-resident preds / y (what test_per_crystal leaves behind), moments + a heat-capacity row:
    pred / y / mae against float64 numpy, the declared ratio centre = m1 / m0 formed from them, and the scale applied to the
    values and not to the ratio."""
    from dostransformer_amd import evaluate, functionals as F
    dt = DTYPES[dtn]
    C, S = 7, 201
    g = torch.Generator().manual_seed(3)
    preds = (0.1 + torch.rand(C, S, generator=g, dtype=torch.float64)).to(dt)              # positive: m0 > 0
    ys = (0.1 + torch.rand(C, S, generator=g, dtype=torch.float64)).to(dt)
    scale = 0.5 + 4.0 * torch.rand(C, generator=g, dtype=torch.float64)
    e = torch.linspace(-5.0, 5.0, S, dtype=torch.float64)
    fn = F.stack(F.moments(e, orders=(0, 1, 2)), F.heat_capacity(torch.linspace(0.0, 900.0, S), [100.0, 300.0]))
    assert fn.names[:3] == ["m0", "m1", "m2"] and fn.ratios == [("centre", 1, 0)]
    res = evaluate.PerCrystalResult(0.0, 0.0, 0.0, 0.0, torch.zeros(C, 4, dtype=torch.float64, device=DEV), preds.to(DEV),
                                    ys.to(DEV), None, None)
    tab = fn.table.to(dt)                                                  # what the kernel reads
    for sc in (None, scale):
        got = evaluate.functionals_per_crystal(res, fn, scale=sc)
        val, mag = _host(preds, ys, tab, sc)
        assert got.names == fn.names and got.ratio_names == ["centre"]
        assert got.pred.shape == (C, fn.K) and got.pred.is_cuda and got.pred.dtype == torch.float64
        assert float((np.abs(got.pred.cpu().numpy() - val[:, 0]) / mag[:, 0]).max()) <= 1e-13
        assert float((np.abs(got.y.cpu().numpy() - val[:, 1]) / mag[:, 1]).max()) <= 1e-13
        mae = np.abs(val[:, 0] - val[:, 1]).mean(0)
        assert np.allclose(np.array(got.mae), mae, rtol=1e-10, atol=0)
        rp, ry = val[:, 0, 1] / val[:, 0, 0], val[:, 1, 1] / val[:, 1, 0]
        assert got.ratio_pred.shape == (C, 1)
        # m1 sums terms of both signs: the quotient's error is the numerator's bar over m0
        tol = 2e-13 * (mag[:, 0, 1] / np.abs(val[:, 0, 0]) + np.abs(rp))
        assert bool((np.abs(got.ratio_pred[:, 0].cpu().numpy() - rp) <= tol).all())
        tol = 2e-13 * (mag[:, 1, 1] / np.abs(val[:, 1, 0]) + np.abs(ry))
        assert bool((np.abs(got.ratio_y[:, 0].cpu().numpy() - ry) <= tol).all())
        assert abs(got.ratio_mae[0] - float(np.abs(rp - ry).mean())) <= 1e-10
    with pytest.raises(ValueError, match="columns"):
        evaluate.functionals_per_crystal(res, F.cumulative(51))
    with pytest.raises(ValueError, match="scales"):
        evaluate.functionals_per_crystal(res, fn, scale=scale[:3])
    none = evaluate.functionals_per_crystal(res, F.cumulative(S))          # no ratios declared: empty, not an error
    assert none.ratio_names == [] and none.ratio_mae == [] and none.ratio_pred.shape == (C, 0)
