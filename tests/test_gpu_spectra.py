"""dosx_spectra_broaden / dosx_spectra_interp on the GPU (csrc/spectra.hip) against the numpy twin of dostransformer_amd/spectra.py,
one mixed launch per case.

The bar for ``broaden`` (derived, not measured): the arguments of ``exp`` are the same bits on both sides, so a term differs by
its exp's last place and one product rounding, at most 4u|t_i| (u = 2^-53); each of the n_kept - 1 additions can round
differently by 2uA, A = sum |t_i| as the twin computes it.  Hence |y_gpu - y_twin| <= u (2 n_kept + 2) A, and a bin with no kept
term is exactly 0.0.  ``interp`` has no transcendental: bitwise.  Largest measured ratio to the bar: see README.md ("DOS targets
from raw spectra")."""
import functools

import numpy as np
import pytest
import torch

from dostransformer_amd import spectra
from tests import spectra_ref as ref
from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def _case(kind, bins):
    args, outside = ref.mixed_case(kind, bins)
    return args, outside, ref.twin_rows(args)


def _ratio(y_gpu, twin):
    """The largest |y_gpu - y_twin| over the bar; bins without a kept term must be exactly 0.0."""
    y, _, _, _, _, A, n_kept = twin
    y_gpu = y_gpu.cpu().numpy()
    assert np.isfinite(y_gpu).all()
    empty = n_kept == 0
    assert (y_gpu[empty] == 0.0).all() and (y[empty] == 0.0).all()
    bar = U * (2 * n_kept + 2) * A
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(bar > 0, np.abs(y_gpu - y) / bar, np.where(y_gpu == y, 0.0, np.inf))
    return float(r.max())


def _check_derived(res, grid, twin_report):
    """y_max, y_norm and area against the GPU's own rows; the report against the twin's."""
    y = res.y.cpu()
    assert torch.equal(res.y_max.cpu(), y.max(dim=1).values)
    y_max = res.y_max.cpu()[:, None]
    assert torch.equal(res.y_norm.cpu(), torch.where(y_max > 0, y / y_max, torch.zeros_like(y)))
    ordered = grid.de * np.cumsum(y.numpy(), axis=1)[:, -1]
    slack = grid.bins * U * grid.de * np.abs(y.numpy()).sum(1)
    assert (np.abs(res.area.cpu().numpy() - ordered) <= slack).all()
    rep = res.report
    got = torch.stack([rep.n_inside, rep.covered.long(), rep.bad, rep.unsorted], 1)
    assert torch.equal(got, torch.as_tensor(twin_report, dtype=torch.int64))


@pytest.mark.parametrize("bins", ref.BINS)
@pytest.mark.parametrize("kind", ["curve", "points"])
def test_broaden_meets_the_bar(kind, bins):
    args, outside, twin = _case(kind, bins)
    sizes = np.diff(args["ptr"]).tolist()
    want = set((ref.POINT_SIZES if kind == "points" else ref.SIZES) if bins in ref.FULL_BINS else (2, 257))
    assert want <= set(sizes) and len(set(args["sigma"])) == len(sizes) and (args["values"] < 0).any()
    res = spectra.broaden(**args, normalize=True, device=DEV)
    worst = _ratio(res.y, twin)
    print(f"broaden[{kind}, S={bins}]: largest |y_gpu - y_twin| / bar = {worst:.3f}")
    assert worst <= 1.0
    _check_derived(res, args["grid"], twin[4])
    assert int(res.report.n_inside[outside]) == 0 and float(res.y[outside].abs().max()) == 0.0 and float(res.y_max[outside]) == 0.0
    assert not res.report.refused.any() and (~res.report.covered).any() == (kind == "curve")
    again = spectra.broaden(**args, normalize=True, device=DEV)                 # determinism: bitwise from run to run
    for k in ("y", "y_max", "area", "y_norm"):
        assert torch.equal(getattr(res, k), getattr(again, k)), k


def test_the_keep_test_at_its_edge():
    """x == 6.0 exactly is kept, the next double beyond it is dropped: e0 = -4, de = 0.125, sigma = 0.5, a point 3.0 below bin 40."""
    grid = spectra.Grid(-4.0, 0.125, 65)
    s, at = 40, -2.0
    assert grid.energies()[s] == 1.0 and (1.0 - at) / 0.5 == 6.0 and (1.0 - np.nextafter(at, -np.inf)) / 0.5 > 6.0
    es, vs = [np.array([at]), np.array([np.nextafter(at, -np.inf)])], [np.ones(1), np.ones(1)]
    host = spectra.broaden_host(es, vs, grid, 0.5, kind="points", cutoff=6.0)
    res = spectra.broaden(es, vs, grid, 0.5, kind="points", cutoff=6.0, device=DEV)
    peak = 1.0 / (0.5 * spectra.SQRT_2PI)
    assert float(host.y[0, s]) > 1e-8 * peak and float(host.y[1, s]) == 0.0 and float(host.y[1, s - 1]) > 0.0
    y = res.y.cpu()
    assert float(y[1, s]) == 0.0 and float(y[0, s + 1]) == 0.0
    assert abs(float(y[0, s]) - float(host.y[0, s])) <= U * 4 * abs(float(host.y[0, s]))        # n_kept = 1, A = |t|
    assert ((y - host.y).abs() <= U * 4 * host.y.abs()).all() and torch.equal(y == 0, host.y == 0)


@pytest.mark.parametrize("bins", ref.BINS)
def test_interp_is_bitwise_the_twin(bins):
    args = ref.interp_case(bins)
    host = spectra.resample_host(**args, normalize=True)
    res = spectra.resample(**args, normalize=True, device=DEV)
    assert not host.report.refused.any() and torch.isfinite(host.y).all()
    assert torch.equal(res.y.cpu(), host.y)
    for k in ("y_max", "area", "y_norm"):
        assert torch.equal(getattr(res, k).cpu(), getattr(host, k)), k
    _check_derived(res, args["grid"], torch.stack([host.report.n_inside, host.report.covered.long(), host.report.bad,
                                                   host.report.unsorted], 1))
    if bins >= 9:                                        # the curve whose ends are grid points: both hit, zero on either side
        E, a, b = args["grid"].energies(), bins // 8, bins - 1 - bins // 8
        e, v = args["energies"][args["ptr"][-2]:], args["values"][args["ptr"][-2]:]
        assert e[0] == E[a] and e[-1] == E[b]
        row = res.y[-1].cpu().numpy()
        assert row[a] == v[0] and row[b] == v[-1] and (row[:a] == 0.0).all() and (row[b + 1:] == 0.0).all()
    assert (host.y == 0).any() or bins == 1              # some bins lie outside some curve


@pytest.mark.parametrize("which", ["broaden", "resample"])
def test_bad_crystals_get_nan_rows_and_leave_the_rest_alone(which):
    args, _, _ = _case("curve", 201)
    args = {k: v for k, v in args.items() if which == "broaden" or k in ("energies", "values", "ptr", "grid", "shift")}
    run = (lambda a: spectra.broaden(**a, normalize=True, device=DEV)) if which == "broaden" else \
        (lambda a: spectra.resample(**a, normalize=True, device=DEV))
    clean = run(args)
    ptr = args["ptr"]
    sizes = np.diff(ptr)
    k, m = int(np.flatnonzero(sizes == 257)[0]), int(np.flatnonzero(sizes == 64)[0])
    dirty = dict(args, energies=args["energies"].copy(), values=args["values"].copy())
    dirty["values"][ptr[k] + 200] = np.nan                               # a NaN sample in crystal k
    dirty["energies"][ptr[m] + 31] = dirty["energies"][ptr[m] + 30]      # an unsorted curve in crystal m
    res = run(dirty)
    rest = torch.ones(len(sizes), dtype=torch.bool)
    rest[[k, m]] = False
    for name in ("y", "y_norm"):
        got, want = getattr(res, name).cpu(), getattr(clean, name).cpu()
        assert torch.isnan(got[k]).all() and torch.isnan(got[m]).all() and torch.equal(got[rest], want[rest]), name
    for name in ("y_max", "area"):
        got, want = getattr(res, name).cpu(), getattr(clean, name).cpu()
        assert torch.isnan(got[[k, m]]).all() and torch.equal(got[rest], want[rest]), name
    rep = res.report
    assert rep.bad.tolist() == [int(c == k) for c in range(len(sizes))]
    assert rep.unsorted.tolist() == [int(c == m) for c in range(len(sizes))]
    assert torch.equal(rep.n_inside[rest], clean.report.n_inside[rest]) and torch.equal(rep.covered, clean.report.covered)
    assert rep.refused.tolist() == (~rest).tolist()
    host = spectra.broaden_host(**dirty) if which == "broaden" else spectra.resample_host(**dirty)
    for name in ("n_inside", "covered", "bad", "unsorted"):
        assert torch.equal(getattr(rep, name), getattr(host.report, name)), name


def test_a_bad_sigma_lives_on_the_device():
    args, _, _ = _case("points", 51)
    sigma = args["sigma"].copy()
    sigma[0], sigma[2] = 0.0, np.nan
    res = spectra.broaden(**dict(args, sigma=sigma), device=DEV)
    clean = spectra.broaden(**args, device=DEV)
    assert res.report.bad.tolist() == [1, 0, 1] + [0] * (len(sigma) - 3)
    assert torch.isnan(res.y[[0, 2]]).all() and torch.equal(res.y[[1] + list(range(3, len(sigma)))], clean.y[[1] + list(range(3, len(sigma)))])
