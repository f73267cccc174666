"""Targets built from raw spectra inside featurize.build_edos_all / build_data_all (``targets=``): what lands in the crystal dicts is
what spectra.broaden / spectra.resample return, the default is untouched, an uncovered spectrum is reported, and the crystals
train."""
import functools

import numpy as np
import pytest
import torch

from dostransformer_amd import featurize, spectra, synth
from dostransformer_amd._lib import DosxError
from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu

E_GRID = spectra.Grid.linspace(-8.0, 6.0, synth.E_BINS)             # inside every synthetic spectrum (efermi - 11 .. efermi + 9)
PH_GRID = spectra.Grid.linspace(0.0, 7.5, synth.PH_BINS, unit="THz")  # inside every synthetic phonon curve (0 .. >= 9.6)


@functools.lru_cache(maxsize=None)
def _edos():
    finished = synth.edos_structures(8, seed=11)
    table = np.random.default_rng(0).normal(size=(100, synth.E_ATOM_FEATS))
    return finished, synth.raw_edos(finished, seed=12), table


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if torch.is_tensor(a[k]):
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


def test_edos_targets_are_the_launches_results():
    finished, raw, table = _edos()
    tg = spectra.EdosTargets(E_GRID, 0.3)
    cs = featurize.build_edos_all(raw, table, device=DEV, targets=tg)
    dos = [e["dos"] for e in raw]
    es, vs, ef = [d["energies"] for d in dos], [d["densities"] for d in dos], [d["efermi"] for d in dos]
    smooth = spectra.broaden(es, vs, E_GRID, 0.3, shift=ef, normalize=True, device=DEV)
    plain = spectra.resample(es, vs, E_GRID, shift=ef, normalize=True, device=DEV)
    assert smooth.report.covered.all() and not smooth.report.refused.any()
    for c, item in enumerate(cs):
        assert item["y_ft"].dtype == torch.float32 and item["y_ft"].shape == (synth.E_BINS,)
        assert torch.equal(item["y_ft"], smooth.y_norm[c].float().cpu()) and float(item["y_ft"].max()) == 1.0
        assert torch.equal(item["y_max"], smooth.y_max[c].float().cpu()) and float(item["y_max"]) > 0.0
        assert torch.equal(item["y"], plain.y_norm[c].float().cpu()) and bool(item["covered"])
    unscaled = featurize.build_edos_all(raw[:2], table, device=DEV, targets=tg, normalize_target=False)
    assert torch.equal(unscaled[0]["y_ft"], smooth.y[0].float().cpu()) and torch.equal(unscaled[1]["y"], plain.y[1].float().cpu())
    # the host twin sees the same spectra the same way (the kernels' own bar is in test_gpu_spectra.py)
    host = spectra.broaden_host(es, vs, E_GRID, 0.3, shift=ef, normalize=True)
    assert torch.allclose(smooth.y_norm.cpu(), host.y_norm, rtol=0, atol=1e-12)


def test_default_and_finished_targets_are_untouched():
    finished, raw, table = _edos()
    plain = featurize.build_edos_all(finished, table, device=DEV)
    same = featurize.build_edos_all(finished, table, device=DEV, targets=spectra.EdosTargets(E_GRID, 0.3))
    for a, b in zip(plain, same):                        # an entry that carries a finished target keeps it
        _same(a, b)
    none = featurize.build_edos_all(raw, table, device=DEV)               # and raw spectra without `targets` are not looked at
    assert all(not bool(c["y_ft"].any()) and float(c["y_max"]) == 0.0 and "y" not in c and "covered" not in c for c in none)
    mixed = featurize.build_edos_all([finished[0], raw[1]], table, device=DEV, targets=spectra.EdosTargets(E_GRID, 0.3))
    _same(mixed[0], plain[0])
    assert float(mixed[1]["y_ft"].max()) == 1.0 and "y" in mixed[1]


def test_an_uncovered_spectrum_raises_or_is_kept_with_its_report():
    _, raw, table = _edos()
    short = dict(raw[2], dos=dict(raw[2]["dos"]))
    keep = short["dos"]["energies"] <= short["dos"]["efermi"] + 2.3125
    short["dos"]["energies"], short["dos"]["densities"] = short["dos"]["energies"][keep], short["dos"]["densities"][keep]
    entries = [raw[0], raw[1], short]
    with pytest.raises(DosxError, match=r"crystal 2: spectrum ends at 2.3\d eV, window reaches 6.00 eV"):
        featurize.build_edos_all(entries, table, device=DEV, targets=spectra.EdosTargets(E_GRID, 0.3))
    cs = featurize.build_edos_all(entries, table, device=DEV, targets=spectra.EdosTargets(E_GRID, 0.3, on_uncovered="keep"))
    assert [bool(c["covered"]) for c in cs] == [True, True, False]
    assert torch.isfinite(cs[2]["y_ft"]).all() and not bool(cs[2]["y"][torch.from_numpy(E_GRID.energies() > 2.4)].any())
    nan = dict(raw[1], dos=dict(raw[1]["dos"], densities=raw[1]["dos"]["densities"].copy()))
    nan["dos"]["densities"][7] = np.nan
    with pytest.raises(DosxError, match=r"crystal 1: 1 non-finite sample"):                  # never kept
        featurize.build_edos_all([raw[0], nan], table, device=DEV, targets=spectra.EdosTargets(E_GRID, 0.3, on_uncovered="keep"))
    with pytest.raises(ValueError, match="on_uncovered"):
        featurize.build_edos_all(entries, table, device=DEV, targets=spectra.EdosTargets(E_GRID, 0.3, on_uncovered="drop"))


def test_edos_crystals_from_raw_spectra_train():
    from dostransformer_amd.embedder_eDOS.DOSTransformer import DOSTransformer
    from dostransformer_amd.loader import DeviceDataset
    from dostransformer_amd.train import Trainer
    _, raw, table = _edos()
    cs = featurize.build_edos_all(raw, table, device=DEV, targets=spectra.EdosTargets(E_GRID, 0.3))
    torch.manual_seed(0)
    model = DOSTransformer(1, 1, synth.E_ATOM_FEATS, synth.E_BOND_FEATS, 2, 64, DEV, 0.0).to(DEV)
    ds = DeviceDataset(cs, DEV)
    loss = Trainer(model, lr=1e-3).step_dataset(ds, np.arange(8), n_max=int(ds.n_nodes.max()))
    assert bool(torch.isfinite(loss).all())


def test_phonon_targets_from_modes_and_from_curves():
    from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
    from dostransformer_amd.loader import DeviceDataset
    from dostransformer_amd.train import Trainer
    finished = synth.phonon_structures(8, seed=21)
    raw = synth.raw_phonon(finished, seed=22)
    assert all(("frequencies" in e) != ("dos" in e) and "phdos" not in e for e in raw) and "weights" in raw[0]
    tg = spectra.PhononTargets(PH_GRID, 0.3)
    build = lambda es, **kw: featurize.build_data_all(es, r_max=4.0, device=DEV, dtype=torch.float32, **kw)
    cs = build(raw, targets=tg)
    modes, curves = raw[0::2], raw[1::2]
    pts = spectra.broaden([e["frequencies"] for e in modes], [e["weights"] for e in modes], PH_GRID, 0.3, kind="points",
                          normalize=True, device=DEV)
    crv = spectra.broaden([e["dos"]["energies"] for e in curves], [e["dos"]["densities"] for e in curves], PH_GRID, 0.3,
                          normalize=True, device=DEV)
    assert crv.report.covered.all() and not crv.report.refused.any() and not pts.report.refused.any()
    for c, item in enumerate(cs):
        want = (pts if c % 2 == 0 else crv).y_norm[c // 2]
        assert item["phdos"].shape == (1, synth.PH_BINS) and torch.equal(item["phdos"][0], want.float().cpu())
        assert float(item["phdos"].max()) == 1.0 and bool(item["covered"])
    raw_rows = build(raw[:2], targets=spectra.PhononTargets(PH_GRID, 0.3, normalize=False))
    assert torch.equal(raw_rows[0]["phdos"][0], pts.y[0].float().cpu()) and torch.equal(raw_rows[1]["phdos"][0], crv.y[0].float().cpu())
    no_weights = build([{k: v for k, v in raw[0].items() if k != "weights"}], targets=spectra.PhononTargets(PH_GRID, 0.3, normalize=False))
    ones = spectra.broaden([raw[0]["frequencies"]], [np.ones_like(raw[0]["frequencies"])], PH_GRID, 0.3, kind="points", device=DEV)
    assert torch.equal(no_weights[0]["phdos"][0], ones.y[0].float().cpu())
    # the default and finished targets are untouched; an entry with nothing to build from is named
    plain = build(finished)
    for a, b in zip(plain, build(finished, targets=tg)):
        _same(a, b)
    with pytest.raises(ValueError, match="entry 1: no phdos, no frequencies and no dos"):
        build([raw[0], {k: v for k, v in raw[1].items() if k != "dos"}], targets=tg)
    with pytest.raises(DosxError, match=r"crystal 1: spectrum ends at \d+\.\d\d THz, window reaches 40.00 THz"):
        build(raw, targets=spectra.PhononTargets(spectra.Grid.linspace(0.0, 40.0, synth.PH_BINS, unit="THz"), 0.3))
    torch.manual_seed(0)
    model = DOSTransformer_phonon(2, 1, synth.PH_ATOM_FEATS, synth.PH_BOND_FEATS, 32, DEV, 0.0).to(DEV)
    ds = DeviceDataset(cs, DEV)
    loss = Trainer(model, lr=1e-3).step(next(iter(ds.batches(8))))
    assert bool(torch.isfinite(loss).all())
