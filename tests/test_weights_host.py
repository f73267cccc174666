"""CPU-only checks of the weights the weighted losses take: ``weights.balanced`` / ``weights.fermi_window`` (pure torch),
``DeviceDataset``'s weight table and ``set_weights`` (checked on the host, written in place), and the refusals of the three
trainers' ``sample_weights=`` / ``bin_weights=`` arguments, all of which are raised at construction."""
import math

import pytest
import torch

from tests.test_loss_rows_abi import _phonon, _trainers


# ---- weights.balanced -------------------------------------------------------------------------------------------------------
def test_balanced_is_inverse_frequency_with_mean_one():
    from dostransformer_amd import weights
    systems = torch.tensor([0] * 6 + [2] * 3 + [6] * 1)                      # classes 1, 3, 4, 5 do not occur
    w = weights.balanced(systems)
    assert w.dtype == torch.float64 and w.shape == (10,)
    assert abs(float(w.mean()) - 1.0) <= 1e-15
    # inverse proportionality: w_c count[system_c] is one number, and every class that occurs carries the same total weight
    prod = w * torch.tensor([6.0] * 6 + [3.0] * 3 + [1.0])
    assert float((prod - prod[0]).abs().max()) <= 1e-15 * float(prod[0])
    totals = [float(w[:6].sum()), float(w[6:9].sum()), float(w[9:].sum())]
    assert max(totals) - min(totals) <= 1e-14
    assert abs(totals[0] - 10.0 / 3.0) <= 1e-14                              # three classes occur, the absent four get nothing
    # the absent classes are ignored: the same crystals under more (or just enough) classes get the same weights
    assert torch.equal(w, weights.balanced(systems, n_classes=9))
    assert torch.equal(w, weights.balanced(systems.tolist()))
    assert torch.equal(w, weights.balanced(systems.to(torch.int32)))


def test_balanced_power():
    from dostransformer_amd import weights
    systems = torch.tensor([1, 1, 1, 1, 5])
    assert torch.equal(weights.balanced(systems, power=0), torch.ones(5, dtype=torch.float64))
    half = weights.balanced(systems, power=0.5)
    assert abs(float(half.mean()) - 1.0) <= 1e-15
    assert abs(float(half[4] / half[0]) - 2.0) <= 1e-15                      # (4 / 1) ** 0.5
    full = weights.balanced(systems, power=1.0)
    assert abs(float(full[4] / full[0]) - 4.0) <= 1e-15
    one = weights.balanced(torch.tensor([3, 3, 3]))                           # one class: nothing to balance
    assert torch.equal(one, torch.ones(3, dtype=torch.float64))


def test_balanced_refusals():
    from dostransformer_amd import weights
    for bad in ([], [7], [-1, 0], [0.5, 1.0]):
        with pytest.raises(ValueError, match="weights.balanced"):
            weights.balanced(torch.tensor(bad))
    with pytest.raises(ValueError, match="power"):
        weights.balanced(torch.tensor([0, 1]), power=math.inf)


# ---- weights.fermi_window ---------------------------------------------------------------------------------------------------
def test_fermi_window():
    from dostransformer_amd import weights
    S, center, width = 201, 100, 8.0
    v = weights.fermi_window(S, center, width)
    assert v.dtype == torch.float64 and v.shape == (S,)
    assert float(v[center]) == 1.0 and int(v.argmax()) == center
    assert torch.equal(v[:center], v[center + 1:].flip(0))                   # symmetric about the centre bin
    assert abs(float(v[center + 8]) - math.exp(-0.5)) <= 1e-15               # one width out
    assert bool((v[1:center + 1] >= v[:center]).all()) and float(v.min()) >= 0.0
    f = weights.fermi_window(S, center, width, floor=0.25)
    assert float(f[center]) == 1.0 and abs(float(f[0]) - 0.25) <= 1e-12
    assert float((f - (0.25 + 0.75 * v)).abs().max()) <= 1e-15
    assert torch.equal(weights.fermi_window(S, center, width, floor=1.0), torch.ones(S, dtype=torch.float64))
    frac = weights.fermi_window(4, 1.5, 1.0)                                  # a centre between two bins
    assert float(frac[1]) == float(frac[2]) > float(frac[0]) == float(frac[3])
    for kw in (dict(S=0, center=0, width=1.0), dict(S=5, center=2, width=0.0), dict(S=5, center=2, width=math.inf),
               dict(S=5, center=2, width=1.0, floor=-0.1), dict(S=5, center=2, width=1.0, floor=1.5),
               dict(S=5, center=math.nan, width=1.0)):
        with pytest.raises(ValueError, match="weights.fermi_window"):
            weights.fermi_window(**kw)


# ---- DeviceDataset ----------------------------------------------------------------------------------------------------------
def _crystals(n=5, weights=None):
    from dostransformer_amd import synth
    cs = synth.phonon_crystals(n, 91, torch.float32)
    if weights is not None:
        for c, w in zip(cs, weights):
            c["weight"] = w
    return cs


def test_dataset_keeps_weights_and_the_host_collate_hands_them_out():
    from dostransformer_amd.batch import collate, split_crystals
    from dostransformer_amd.loader import DeviceDataset
    ws = [2.0, 0.5, 0.0, 1.0, torch.tensor(3.0)]
    cs = _crystals(5, ws)
    ds = DeviceDataset(cs, "cpu")
    assert ds.weights.dtype == torch.float32 and ds.weights.tolist() == [2.0, 0.5, 0.0, 1.0, 3.0]
    assert ds._graph["weight"] is ds.weights                                  # a graph-level table: what collate() selects from
    assert ds._f32_tables()["weight"] is ds.weights                           # fp32 dataset: the resident table itself
    assert DeviceDataset(cs, "cpu", dtype=torch.float64).weights.dtype == torch.float64
    # the host collate carries the field the same way, and split_crystals gives it back
    h = collate([cs[i] for i in (4, 0, 2)])
    assert h.weight.tolist() == [3.0, 2.0, 0.0] and h.weight.dtype == torch.float32
    assert [float(c["weight"]) for c in split_crystals(h)] == [3.0, 2.0, 0.0]
    # a dataset without weights has none, and its batches no field
    plain = DeviceDataset(_crystals(3), "cpu")
    assert plain.weights is None and "weight" not in plain._graph and plain._f32_tables()["weight"] is None


def test_set_weights_checks_on_the_host_and_writes_in_place():
    from dostransformer_amd.loader import DeviceDataset
    ds = DeviceDataset(_crystals(5, [1.0] * 5), "cpu", dtype=torch.float64)
    t64, t32 = ds._f64_tables()["weight"], ds._f32_tables()["weight"]
    assert t64 is ds.weights and t32 is not ds.weights and t32.dtype == torch.float32
    ptrs = (t64.data_ptr(), t32.data_ptr())
    ds.set_weights([0.0, 0.25, 4.0, 1.0, 2.0])
    assert (ds._f64_tables()["weight"].data_ptr(), ds._f32_tables()["weight"].data_ptr()) == ptrs      # in place: same storage
    assert t64.tolist() == t32.tolist() == [0.0, 0.25, 4.0, 1.0, 2.0]
    ds.set_weights(torch.full((5,), 0.5))
    assert t64.tolist() == t32.tolist() == [0.5] * 5
    for bad, word in (([1.0, math.nan, 1.0, 1.0, 1.0], "not finite"), ([1.0, 1.0, math.inf, 1.0, 1.0], "not finite"),
                      ([1.0, 1.0, 1.0, -0.5, 1.0], "negative"), ([1.0] * 4, "4 weights for 5")):
        with pytest.raises(ValueError, match=word):
            ds.set_weights(bad)
        assert t64.tolist() == [0.5] * 5                                      # a refused call writes nothing
    with pytest.raises(ValueError, match="not finite"):
        DeviceDataset(_crystals(3, [1.0, math.nan, 1.0]), "cpu")
    with pytest.raises(ValueError, match="negative"):
        DeviceDataset(_crystals(3, [1.0, 1.0, -1.0]), "cpu")
    # a dataset built without weights gets its table here - also in the tables that exist already
    plain = DeviceDataset(_crystals(3), "cpu")
    tables = plain._f32_tables()
    plain.set_weights([1.0, 2.0, 3.0])
    assert plain.weights.tolist() == [1.0, 2.0, 3.0] and tables["weight"].tolist() == [1.0, 2.0, 3.0]


# ---- the trainers' constructors ---------------------------------------------------------------------------------------------
def test_trainers_refuse_weights_without_a_per_crystal_loss():
    for cls, model in _trainers():
        m = model()
        for kw in (dict(sample_weights=True), dict(bin_weights=torch.ones(51)), dict(sample_weights=True, bin_weights=[1.0] * 51)):
            with pytest.raises(ValueError, match='loss="crystal_rmse"'):
                cls(m, **kw)
        tr = cls(m, loss="mae", sample_weights=True, bin_weights=torch.ones(51))
        assert tr.sample_weights is True and tr.bin_weights.dtype == torch.float64 and tr.bin_weights.shape == (51,)
        assert not any("weight" in k and k != "weight_decay" for k in tr.state_dict()["hyper"])    # constructor arguments, like loss
        tr = cls(m, loss="mae")
        assert tr.sample_weights is False and tr.bin_weights is None
        tr = cls(m)
        assert tr.sample_weights is False and tr.bin_weights is None


def test_trainers_refuse_bad_bin_weights():
    for cls, model in _trainers():
        m = model()
        for bad, word in ((torch.zeros(51), "sum to 0"), (torch.ones(50), r"\[S\] = \[51\]"), (torch.ones(52), r"\[S\] = \[51\]"),
                          (torch.ones(1, 51), r"\[S\] = \[51\]"), ([1.0] * 50 + [math.nan], "finite"),
                          ([1.0] * 50 + [math.inf], "finite"), ([1.0] * 50 + [-1e-3], ">= 0")):
            with pytest.raises(ValueError, match=word):
                cls(m, loss="mse", bin_weights=bad)
        v = [0.0] * 50 + [1e-3]                                               # zeros are fine as long as one bin is left
        assert cls(m, loss="mse", bin_weights=v).bin_weights.tolist() == v


def test_trainer_refuses_weights_under_data_parallelism():
    from dostransformer_amd._lib import DosxError
    from dostransformer_amd.train import Trainer
    from tests.gpu_util import _FakeDist
    for kw in (dict(sample_weights=True), dict(bin_weights=torch.ones(51))):
        with pytest.raises(DosxError, match="single-GPU mode: not with dist"):
            Trainer(_phonon(), dist=_FakeDist(None), **kw)                    # (refused like loss=, and before it is asked for)
        with pytest.raises(DosxError, match="single-GPU mode: not with dist"):
            Trainer(_phonon(), dist=_FakeDist(None), loss="mse", **kw)
