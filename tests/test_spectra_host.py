"""The numpy twin of the spectra kernels (dostransformer_amd/spectra.py: broaden_host, resample_host) against known answers: a
constant density, the area of one peak, a straight line, a moved origin; then the report, its messages and the argument forms."""
import math

import numpy as np
import pytest
import torch

from dostransformer_amd import spectra
from dostransformer_amd._lib import DosxError
from tests import spectra_ref as ref

U = 2.0 ** -53


def _theta_and_tails(sigma, h, cutoff):
    """The two terms of the error of a Gaussian sum on a lattice of spacing h cut at `cutoff` standard deviations: the ripple of
    the theta function (Poisson summation: the first harmonic, 2 exp(-2 pi^2 sigma^2 / h^2)) and the two cut tails."""
    return 2.0 * math.exp(-2.0 * math.pi ** 2 * sigma ** 2 / h ** 2) + math.erfc(cutoff / math.sqrt(2.0))


def test_a_constant_density_stays_constant():
    d0, sigma, cutoff = 3.25, 0.125, 6.0
    e = np.arange(-6.0, 6.0 + 1e-9, sigma)                       # h = sigma, 2.0 beyond the window > cutoff * sigma = 0.75
    grid = spectra.Grid.linspace(-4.0, 4.0, 81)                  # de = 0.1: the bins fall at every offset between two samples
    res = spectra.broaden_host([e], [np.full_like(e, d0)], grid, sigma, cutoff=cutoff)
    err = float((res.y[0] / d0 - 1.0).abs().max())
    bound = _theta_and_tails(sigma, sigma, cutoff) + 32 * U      # 13 kept terms: a few roundings
    print(f"constant density: max relative error {err:.3e}, bound {bound:.3e}")
    assert 0.0 < err <= bound < 8e-9
    assert bool(res.report.covered[0]) and int(res.report.n_inside[0]) == 2 * (32 + 6) + 1
    assert float(res.y_max[0]) == float(res.y[0].max())


def test_one_point_has_area_one():
    sigma, cutoff = 0.125, 6.0
    grid = spectra.Grid(-12.5, 0.125, 201)                       # de = sigma, the point 100 bins from either end
    res = spectra.broaden_host([[0.03]], [[1.0]], grid, sigma, kind="points", cutoff=cutoff)
    err = abs(float(res.area[0]) - 1.0)
    bound = _theta_and_tails(sigma, grid.de, cutoff) + 201 * U
    print(f"one point: |area - 1| = {err:.3e}, bound {bound:.3e}")
    assert 0.0 < err <= bound < 8e-9
    assert int((res.y[0] != 0).sum()) == 12                       # bins within 6 sigma = 0.75 of 0.03: offsets -0.72 .. 0.655


def test_resampling_a_line_is_exact_when_everything_is_binary():
    a, b = 1.5, -2.0
    e = np.cumsum(np.tile([0.25, 0.5, 1.0, 0.125], 8)) - 7.0      # -6.75 .. 8.0, spacings powers of two
    grid = spectra.Grid(-4.0, 0.125, 65)
    res = spectra.resample_host([e], [a + b * e], grid)
    assert np.array_equal(res.y[0].numpy(), a + b * grid.energies())
    assert bool(res.report.covered[0]) and float(res.y_max[0]) == a + b * -4.0
    assert float(res.area[0]) == 0.125 * float(np.cumsum(a + b * grid.energies())[-1])
    # a curve that ends on a grid point gives that point's value there and zero beyond it
    cut = spectra.resample_host([e[e <= 1.25]], [a + b * e[e <= 1.25]], grid)
    E = grid.energies()
    assert e[e <= 1.25][-1] == 1.25 and np.array_equal(cut.y[0].numpy(), np.where(E <= 1.25, a + b * E, 0.0))
    assert not bool(cut.report.covered[0]) and int(cut.report.n_inside[0]) == int(((e >= -4.0) & (e <= 1.25)).sum())


def test_shift_is_a_moved_origin():
    rng = np.random.default_rng(3)
    e = np.sort(rng.choice(np.arange(-512, 512), 200, replace=False)) / 64.0          # exact in binary, and so is e - 0.375
    v = rng.normal(0.5, 1.0, 200)
    grid = spectra.Grid.linspace(-4.0, 4.0, 201)
    for kind in ("curve", "points"):
        moved = spectra.broaden_host([e - 0.375], [v], grid, 0.17, kind=kind)
        shifted = spectra.broaden_host([e], [v], grid, 0.17, shift=0.375, kind=kind)
        assert torch.equal(moved.y, shifted.y) and torch.equal(moved.area, shifted.area)
        assert torch.equal(moved.report.n_inside, shifted.report.n_inside)
    assert torch.equal(spectra.resample_host([e - 0.375], [v], grid).y, spectra.resample_host([e], [v], grid, shift=0.375).y)


def test_the_ordered_and_the_vectorized_twin_agree():
    args, _ = ref.mixed_case("curve", 201)
    y, _, _, _, report, A, n_kept = ref.twin_rows(args)
    ptr, e, v = spectra._flatten(args["energies"], args["values"], args["ptr"], "curve")
    fast = spectra.broaden_rows_host(ptr, e, v, args["shift"], args["sigma"], args["grid"], 6.0, "curve", vectorized=True)
    assert np.array_equal(fast[4], report)
    assert (np.abs(fast[0] - y) <= U * (2 * n_kept + 2) * A).all() and (fast[0][n_kept == 0] == 0.0).all()


def _one(e, v, **kw):
    return spectra.broaden_host([np.asarray(e, np.float64)], [np.asarray(v, np.float64)], spectra.Grid(-4.0, 0.125, 65), 0.25, **kw)


def test_report_fields_and_messages():
    e = np.linspace(-6.0, 6.0, 97)
    good = _one(e, np.ones(97))
    assert (int(good.report.bad[0]), int(good.report.unsorted[0]), bool(good.report.covered[0])) == (0, 0, True)
    assert int(good.report.n_inside[0]) == int(((e >= -5.5) & (e <= 5.5)).sum())
    good.report.raise_if_bad()

    short = _one(e[e <= 2.3125], np.ones(97)[e <= 2.3125])               # a curve that ends inside the window
    assert not bool(short.report.covered[0]) and torch.isfinite(short.y).all()
    with pytest.raises(DosxError, match=r"1 spectrum cannot .* crystal 0: spectrum ends at 2.25 eV, window reaches 4.00 eV"):
        short.report.raise_if_bad()
    short.report.raise_if_bad(uncovered=False)
    late = _one(e[e >= -1.0], np.ones(97)[e >= -1.0])
    with pytest.raises(DosxError, match=r"crystal 0: spectrum starts at -1.00 eV, window starts at -4.00 eV"):
        late.report.raise_if_bad()

    v = np.ones(97)
    v[40] = np.nan
    nan = _one(e, v, normalize=True)                                      # a NaN density
    assert int(nan.report.bad[0]) == 1 and int(nan.report.unsorted[0]) == 0
    assert torch.isnan(nan.y).all() and torch.isnan(nan.y_norm).all() and torch.isnan(nan.y_max).all() and torch.isnan(nan.area).all()
    with pytest.raises(DosxError, match=r"crystal 0: 1 non-finite sample"):
        nan.report.raise_if_bad(uncovered=False)

    tie = e.copy()
    tie[11] = tie[10]                                                     # an equal pair of energies
    tied = _one(tie, np.ones(97))
    assert int(tied.report.unsorted[0]) == 1 and int(tied.report.bad[0]) == 0 and torch.isnan(tied.y).all()
    with pytest.raises(DosxError, match=r"crystal 0: energies do not ascend strictly \(1 pair"):
        tied.report.raise_if_bad()
    again = spectra.resample_host([tie], [np.ones(97)], spectra.Grid(-4.0, 0.125, 65))
    assert int(again.report.unsorted[0]) == 1 and torch.isnan(again.y).all()
    assert torch.isfinite(_one(tie, np.ones(97), kind="points").y).all()   # points may repeat and come in any order

    for sigma in (0.0, -0.1, float("nan"), float("inf")):                  # sigma lives with the data, not with the refusals
        res = spectra.broaden_host([e], [np.ones(97)], spectra.Grid(-4.0, 0.125, 65), sigma)
        assert int(res.report.bad[0]) == 1 and torch.isnan(res.y).all()


def test_one_bad_crystal_leaves_the_others_alone():
    args, outside = ref.mixed_case("curve", 51)
    clean = spectra.broaden_host(**args, normalize=True)
    assert not clean.report.refused.any() and int(clean.report.n_inside[outside]) == 0 and float(clean.y[outside].abs().max()) == 0.0
    assert float(clean.y_max[outside]) == 0.0 and float(clean.y_norm[outside].abs().max()) == 0.0
    dirty = dict(args, values=args["values"].copy())
    dirty["values"][args["ptr"][1]] = np.inf
    res = spectra.broaden_host(**dirty, normalize=True)
    keep = torch.arange(len(args["ptr"]) - 1) != 1
    assert res.report.refused.tolist() == (~keep).tolist() and torch.isnan(res.y[1]).all()
    assert torch.equal(res.y[keep], clean.y[keep]) and torch.equal(res.y_norm[keep], clean.y_norm[keep])
    with pytest.raises(DosxError, match="crystal 1: 1 non-finite"):
        res.report.raise_if_bad(uncovered=False)


def test_scalar_and_per_crystal_arguments_and_both_input_forms():
    rng = np.random.default_rng(5)
    es = [np.sort(rng.uniform(-6, 6, n)) for n in (40, 2, 300)]
    vs = [rng.normal(size=e.shape) for e in es]
    grid = spectra.Grid.linspace(-4.0, 4.0, 51)
    a = spectra.broaden_host(es, vs, grid, 0.2, shift=0.3, normalize=True)
    b = spectra.broaden_host(es, vs, grid, [0.2] * 3, shift=np.full(3, 0.3), normalize=True)
    ptr = np.concatenate([[0], np.cumsum([e.shape[0] for e in es])])
    c = spectra.broaden_host(np.concatenate(es), np.concatenate(vs), grid, torch.tensor(0.2, dtype=torch.float64), shift=torch.full((3,), 0.3,
                             dtype=torch.float64), normalize=True, ptr=ptr)
    for r in (b, c):
        assert torch.equal(a.y, r.y) and torch.equal(a.y_norm, r.y_norm) and torch.equal(a.area, r.area) and torch.equal(a.y_max, r.y_max)
    assert a.y.dtype == torch.float64 and a.y.shape == (3, 51) and a.y_norm.shape == (3, 51)
    assert spectra.broaden_host(es, vs, grid, 0.2).y_norm is None
    ra, rb = spectra.resample_host(es, vs, grid, shift=0.3), spectra.resample_host(np.concatenate(es), np.concatenate(vs), grid,
                                                                                   shift=[0.3] * 3, ptr=ptr)
    assert torch.equal(ra.y, rb.y)
    # y_norm is y over its maximum, and zero where the maximum is not positive
    neg = spectra.broaden_host([es[0]], [-np.abs(vs[0])], grid, 0.2, normalize=True)
    assert float(neg.y_max[0]) <= 0.0 and float(neg.y_norm.abs().max()) == 0.0
    assert torch.equal(a.y_norm, a.y / a.y_max[:, None])
    assert spectra.Grid.linspace(-4.0, 4.0, 51).energies()[-1] == -4.0 + 0.16 * 50.0
