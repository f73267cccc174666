"""The reference's evaluation at batch_size = 1 in batched passes, on a real MI355X: dosx_eval_metrics / dosx_eval_metrics_f64
(csrc/eval.hip) against evaluate.per_crystal_metrics_host, predict.Predictor(64).forward_dataset and evaluate.test_per_crystal
against the batch-1 loop of the same model and against the pinned oracle run the reference's way (one crystal per batch)."""
import functools
import gc

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-12                                     # x max(1, |v|): float64 sums of at most 600 terms, orders differ
SIZES = (1, 51, 64, 65, 201, 257, 600)          # below / at / just over one wave's 64 lanes, the workload's 51 and 201, many rounds


def _ops():
    from dostransformer_amd import ops
    return ops


def _twin(pred, y, clamp0=False):
    from dostransformer_amd.evaluate import per_crystal_metrics_host
    return per_crystal_metrics_host(pred, y, clamp0)


def _assert_metrics(got, want, tag=""):
    """within 1e-12 max(1, |v|); NaNs where the reference has NaNs, infinities equal"""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    nan, inf = torch.isnan(want), torch.isinf(want)
    assert torch.equal(torch.isnan(got), nan), (tag, got, want)
    assert torch.equal(got[inf], want[inf]), (tag, got[inf], want[inf])
    fin = ~(nan | inf)
    err = (got - want).abs()[fin] / torch.clamp(want.abs()[fin], min=1.0)
    assert err.numel() == 0 or float(err.max()) <= TOL, (tag, float(err.max()))


def _inputs(B, S, dtype, seed):
    """Targets with negative entries, predictions around them; from B = 5 on, row 2 has a constant target (0.5: its sums are exact
    in float64 whatever their order, so the row's mean is the constant and sum (y - mean)^2 is exactly 0)."""
    gen = torch.Generator().manual_seed(seed)
    y = torch.randn(B, S, generator=gen, dtype=torch.float64)
    p = y + 0.4 * torch.randn(B, S, generator=gen, dtype=torch.float64)
    if B >= 5:
        y[2] = 0.5
    assert bool((y < 0).any()) or S == 1
    return p.to(dtype).to(DEV), y.to(dtype).to(DEV)


@pytest.fixture(scope="module", autouse=True)
def _release_shared_state():
    """The models, datasets, recorded buckets and results that the tests of this module share are dropped when the module is done:
    the rest of the suite gets their device memory back."""
    yield
    for cached in (_result, _batch1, _oracle, _case):
        cached.cache_clear()
    gc.collect()


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_eval_metrics_kernel_against_the_twin(dtype):
    ops = _ops()
    for B in (1, 5, 67):
        for S in SIZES:
            for clamp0 in (False, True):
                for outs in (True, False):
                    tag = f"B{B} S{S} clamp{int(clamp0)} outs{int(outs)}"
                    p, y = _inputs(B, S, dtype, 1000 * B + S)
                    table = torch.full((B + 5, 4), -7.0, dtype=torch.float64, device=DEV)       # written in the middle rows only
                    po = torch.full((B + 2, S), -7.0, dtype=dtype, device=DEV) if outs else None
                    yo = torch.full((B + 2, S), -7.0, dtype=dtype, device=DEV) if outs else None
                    ops.eval_metrics(p, y, table[2:2 + B], clamp0=clamp0, pred_out=po[1:1 + B] if outs else None,
                                     y_out=yo[1:1 + B] if outs else None)
                    torch.cuda.synchronize()
                    want = _twin(p.double(), y.double(), clamp0)       # the kernel's own inputs cast to float64
                    _assert_metrics(table[2:2 + B], want, tag)
                    assert bool((table[:2] == -7.0).all()) and bool((table[2 + B:] == -7.0).all()), tag
                    if B >= 5:                                         # the constant target: IEEE division, like evaluate.r2
                        assert float(table[2 + 2, 3]) == -np.inf, (tag, float(table[4, 3]))
                    if outs:
                        pc, yc = (torch.clamp(p, min=0.0), torch.clamp(y, min=0.0)) if clamp0 else (p, y)
                        assert torch.equal(po[1:1 + B], pc) and torch.equal(yo[1:1 + B], yc), tag
                        for t in (po, yo):
                            assert bool((t[0] == -7.0).all()) and bool((t[-1] == -7.0).all()), tag


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_eval_metrics_row_is_bitwise_the_same_alone_and_as_row_66_of_67(dtype):
    ops = _ops()
    for S in SIZES:
        for clamp0 in (False, True):
            p, y = _inputs(67, S, dtype, 77 + S)
            full = torch.empty(67, 4, dtype=torch.float64, device=DEV)
            alone = torch.empty(1, 4, dtype=torch.float64, device=DEV)
            ops.eval_metrics(p, y, full, clamp0=clamp0)
            ops.eval_metrics(p[66:67], y[66:67], alone, clamp0=clamp0)
            torch.cuda.synchronize()
            assert torch.equal(full[66:67].view(torch.int64), alone.view(torch.int64)), (S, clamp0, full[66], alone[0])


def test_eval_metrics_error_zero_on_a_constant_target_is_nan_and_a_perfect_row_is_1():
    ops = _ops()
    for dtype in (torch.float32, torch.float64):
        y = torch.full((2, 51), 0.5, dtype=dtype, device=DEV)
        y[1] = torch.linspace(-1.0, 1.0, 51, dtype=dtype, device=DEV)
        out = torch.empty(2, 4, dtype=torch.float64, device=DEV)
        ops.eval_metrics(y.clone(), y, out)
        torch.cuda.synchronize()
        assert np.isnan(float(out[0, 3])) and float(out[1, 3]) == 1.0 and bool((out[:, :3] == 0.0).all())
        _assert_metrics(out, _twin(y.double(), y.double()))


def test_eval_metrics_wrapper_checks_its_operands():
    ops = _ops()
    p, y = _inputs(4, 51, torch.float32, 3)
    m = torch.empty(4, 4, dtype=torch.float64, device=DEV)
    with pytest.raises(TypeError):
        ops.eval_metrics(p, y.double(), m)
    with pytest.raises(TypeError):
        ops.eval_metrics(p, y, m.float())
    with pytest.raises(TypeError):
        ops.eval_metrics(p.half(), y.half(), m)
    with pytest.raises(ValueError):
        ops.eval_metrics(p, y[:3], m)
    with pytest.raises(ValueError):
        ops.eval_metrics(p, y, m[:3])
    with pytest.raises(ValueError):
        ops.eval_metrics(p[:, ::2], y[:, ::2], m)                       # rows S apart with unit stride only
    with pytest.raises(ValueError):
        ops.eval_metrics(p, y, torch.empty(4, 8, dtype=torch.float64, device=DEV)[:, :4])
    with pytest.raises(ValueError):
        ops.eval_metrics(p, y, m, pred_out=torch.empty(4, 50, device=DEV))


# ---- the evaluator, fp32 ------------------------------------------------------------------------------------------------------
CASES = {"phonon": dict(count=37, seed=401, batch_size=16, chunks=[16, 16, 5], S=51),
         "edos": dict(count=21, seed=402, batch_size=8, chunks=[8, 8, 5], S=201)}
L, T, H = 3, 2, 64


def _double(c):
    return {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in c.items()}


@functools.lru_cache(maxsize=None)
def _case(kind):
    """Model (on the GPU, eval mode), its weights in float64 for the oracle, the crystals (fp32; the eDOS targets moved down by
    0.3 so that the clamp matters) and their DeviceDataset."""
    from dostransformer_amd import synth
    from dostransformer_amd.embedder_eDOS.DOSTransformer import DOSTransformer
    from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
    from dostransformer_amd.loader import DeviceDataset
    c = CASES[kind]
    torch.manual_seed(c["seed"])
    if kind == "phonon":
        model = DOSTransformer_phonon(L, T, 118, 4, H, DEV, 0.0)
        crystals = synth.phonon_crystals(c["count"], c["seed"], dtype=torch.float32)
    else:
        model = DOSTransformer(L, T, 200, 41, 2, H, DEV, 0.0)
        crystals = synth.edos_crystals(c["count"], c["seed"], dtype=torch.float32)
        for cr in crystals:
            cr["y_ft"] = cr["y_ft"] - 0.3
        assert any(bool((cr["y_ft"] < 0).any()) for cr in crystals)
    p64 = {k: (v.detach().clone().double() if v.is_floating_point() else v.clone()) for k, v in model.state_dict().items()}
    model = model.to(DEV).eval()
    assert len({int(cr["x"].shape[0]) for cr in crystals}) > 1                 # unequal crystals: the padding matters
    return dict(model=model, p64=p64, crystals=crystals, ds=DeviceDataset(crystals, DEV))


@functools.lru_cache(maxsize=None)
def _result(kind):
    """One evaluation of the whole split, shared (and left unchanged) by the tests below."""
    from dostransformer_amd import evaluate
    from dostransformer_amd.predict import Predictor
    c = _case(kind)
    pred = Predictor(c["model"], per_crystal_keys=True)
    res = evaluate.test_per_crystal(pred, c["ds"], batch_size=CASES[kind]["batch_size"])
    torch.cuda.synchronize()
    return res, pred


@functools.lru_cache(maxsize=None)
def _batch1(kind):
    """The batch-1 loop of the same model (tests/test_gpu_predict.py::_batch1_loop): per-crystal dos_system rows and node rows."""
    from dostransformer_amd.batch import collate
    c = _case(kind)
    ss, xs = [], []
    with torch.no_grad():
        for cr in c["crystals"]:
            _, x, ds = c["model"](collate([cr]).to(DEV, dtype=torch.float32))
            ss.append(ds.float().clone()); xs.append(x.float().clone())
    return torch.cat(ss), xs


@functools.lru_cache(maxsize=None)
def _oracle(kind):
    """The pinned oracle run the reference's way - O.eval_phonon / O.eval_edos over a loader of single-crystal batches, float64
    copies of the weights - with its forward wrapped so that the (unclamped) per-crystal predictions are kept too."""
    from oracle import dos_oracle as O
    from dostransformer_amd.batch import collate
    c = _case(kind)
    loader = [collate([_double(cr)]) for cr in c["crystals"]]
    name = "dostransformer_phonon_forward" if kind == "phonon" else "dostransformer_forward"
    inner, kept = getattr(O, name), []

    def keeping(*a, **k):
        out = inner(*a, **k)
        kept.append(out[2].detach().clone())
        return out

    setattr(O, name, keeping)
    try:
        four = O.eval_phonon(c["p64"], loader, L, T) if kind == "phonon" else O.eval_edos(c["p64"], loader, L, T)[0]
    finally:
        setattr(O, name, inner)
    preds = torch.cat(kept)
    y = torch.stack([cr["phdos" if kind == "phonon" else "y_ft"].reshape(-1).double() for cr in c["crystals"]])
    assert preds.dtype == torch.float64 and preds.shape == y.shape
    return four, preds, y


@pytest.mark.parametrize("kind", list(CASES))
def test_per_crystal_table_is_the_twin_of_its_rows_and_the_means_are_its_means(kind):
    res, _ = _result(kind)
    c, C = CASES[kind], CASES[kind]["count"]
    assert res.per_crystal.dtype == torch.float64 and tuple(res.per_crystal.shape) == (C, 4) and res.per_crystal.is_cuda
    assert res.preds.dtype == res.y.dtype == torch.float32 and tuple(res.preds.shape) == tuple(res.y.shape) == (C, c["S"])
    _assert_metrics(res.per_crystal, _twin(res.preds, res.y, clamp0=False), kind)      # (res.preds / res.y are clamped already)
    mean = res.per_crystal.mean(0).tolist()
    assert [res.rmse, res.mse, res.mae, res.r2] == mean and all(isinstance(v, float) and np.isfinite(v) for v in mean)
    if kind == "edos":
        assert float(res.preds.min()) >= 0.0 and float(res.y.min()) == 0.0
    # as_reference(): the reference's tuples
    ref = res.as_reference()
    assert isinstance(ref, tuple) and ref[:4] == (res.rmse, res.mse, res.mae, res.r2)
    if kind == "phonon":
        assert len(ref) == 4 and res.embeddings is None and res.mp_id is None
    else:
        assert len(ref) == 5 and isinstance(ref[4], list) and len(ref[4]) == 1 and len(ref[4][0]) == 4
        ids, preds, y, emb = ref[4][0]
        assert ids == [cr["mp_id"] for cr in _case(kind)["crystals"]]
        for a, shape in ((preds, (C, c["S"])), (y, (C, c["S"])), (emb, (C, H))):
            assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.shape == shape
        assert np.array_equal(preds, res.preds.cpu().numpy()) and np.array_equal(emb, res.embeddings.cpu().numpy())


@pytest.mark.parametrize("kind,subset", [("phonon", False), ("phonon", True), ("edos", False), ("edos", True)])
def test_rows_equal_the_batch_1_loop_and_follow_the_indices(kind, subset):
    from dostransformer_amd import evaluate
    c, k = _case(kind), CASES[kind]
    C = k["count"]
    if subset:                                                           # a shuffled subset, through the same predictor
        idx = np.random.default_rng(5).permutation(C)[:C - 6]
        res = evaluate.test_per_crystal(_result(kind)[1], c["ds"], indices=idx, batch_size=k["batch_size"])
        torch.cuda.synchronize()
    else:
        idx, res = np.arange(C), _result(kind)[0]
    ref_s, ref_x = _batch1(kind)
    want = ref_s[torch.as_tensor(idx, device=DEV)]
    sc = max(float(ref_s.abs().max()), 1.0)
    if kind == "edos":
        want = torch.clamp(want, min=0.0)
    assert tuple(res.preds.shape) == (len(idx), k["S"])
    assert float((res.preds - want).abs().max()) <= 4e-6 * sc, float((res.preds - want).abs().max())
    key = "phdos" if kind == "phonon" else "y_ft"
    y = torch.stack([c["crystals"][i][key].reshape(-1) for i in idx]).to(DEV)
    assert torch.equal(res.y, torch.clamp(y, min=0.0) if kind == "edos" else y)
    if kind == "edos":
        assert res.mp_id == [c["crystals"][i]["mp_id"] for i in idx]
        # sum-pooled node embeddings: n_c rows, each within 4e-6 of the scale of x of the batch-1 loop's (that file's bound on x),
        # summed in fp32 in another order (n_c 2^-24 of the scale again); a ghost row of the bucket in a sum would be O(1)
        xs = max(max(float(x.abs().max()) for x in ref_x), 1.0)
        for r, i in enumerate(idx):
            n = ref_x[i].shape[0]
            d = float((res.embeddings[r].double() - ref_x[i].double().sum(0)).abs().max())
            assert d <= n * (4e-6 + 2.0 ** -23) * xs, (r, i, d)
    else:
        assert res.embeddings is None and res.mp_id is None


@pytest.mark.parametrize("kind", list(CASES))
def test_against_the_oracle_at_batch_size_1(kind):
    res, _ = _result(kind)
    four, o_pred, o_y = _oracle(kind)
    S, clamp0 = CASES[kind]["S"], kind == "edos"
    # the GPU's predictions before the clamp (res.preds of eDOS is clamped): the same passes once more
    c = _case(kind)
    if clamp0:
        pred, rows = _result(kind)[1], []
        nmax = int(c["ds"].n_nodes.max())
        for r0 in range(0, CASES[kind]["count"], CASES[kind]["batch_size"]):
            (_, _, dsys), _ = pred.forward_dataset(c["ds"], range(r0, min(r0 + CASES[kind]["batch_size"], CASES[kind]["count"])), nmax)
            rows.append(dsys.clone())
        raw = torch.cat(rows).double().cpu()
        assert torch.equal(torch.clamp(raw, min=0.0).float(), res.preds.cpu())
    else:
        raw = res.preds.double().cpu()
    assert torch.equal(res.y.double().cpu(), torch.clamp(o_y, min=0.0) if clamp0 else o_y)     # the same targets on both sides
    delta = torch.sqrt(((raw - o_pred) ** 2).mean(1))                    # RMS difference per crystal
    print(f"{kind}: largest per-crystal RMS difference to the oracle {float(delta.max()):.3e}")
    assert float(delta.max()) < 1e-4, float(delta.max())
    # |d rmse| <= delta, |d mae| <= delta, |d mse| <= delta (rmse + rmse'), |d r2| <= S delta (rmse + rmse') / sum (y - mean)^2
    # (triangle inequality; the clamp is 1-Lipschitz), each + 1e-12
    got = res.per_crystal.cpu()
    want = _twin(o_pred, o_y, clamp0)
    yc = torch.clamp(o_y, min=0.0) if clamp0 else o_y
    sst = ((yc - yc.mean(1, keepdim=True)) ** 2).sum(1)
    rr = got[:, 0] + want[:, 0]
    bound = torch.stack([delta, delta * rr, delta, S * delta * rr / sst], 1) + 1e-12
    diff = (got - want).abs()
    print(f"{kind}: largest metric difference / bound {float((diff / bound).max()):.3f}")
    assert bool((diff <= bound).all()), (diff / bound).max(0)
    # the four returned means against the oracle's own four (mean over its single-crystal batches)
    mb = bound.mean(0)
    for k, (a, b) in enumerate(zip((res.rmse, res.mse, res.mae, res.r2), four)):
        assert abs(a - b) <= float(mb[k]), (kind, k, a, b, float(mb[k]))


@pytest.mark.parametrize("kind", list(CASES))
def test_second_pass_replays_every_chunk_and_is_bitwise_the_first(kind):
    from dostransformer_amd import evaluate
    from dostransformer_amd.predict import Predictor
    c, k = _case(kind), CASES[kind]
    pred = Predictor(c["model"], per_crystal_keys=True)
    a = evaluate.test_per_crystal(pred, c["ds"], batch_size=k["batch_size"])
    a = a._replace(per_crystal=a.per_crystal.clone(), preds=a.preds.clone(), y=a.y.clone())
    misses, hits = pred.slot_misses, pred.slot_hits
    assert 1 <= misses <= len(k["chunks"]) and misses + hits == len(k["chunks"])
    assert all(key[-1] == "dataset" for key in pred._slots)                # kept apart from the buckets of __call__
    b = evaluate.test_per_crystal(pred, c["ds"], batch_size=k["batch_size"])
    torch.cuda.synchronize()
    assert pred.slot_misses == misses and pred.slot_hits == hits + len(k["chunks"])
    assert (a.rmse, a.mse, a.mae, a.r2) == (b.rmse, b.mse, b.mae, b.r2)
    assert torch.equal(a.per_crystal, b.per_crystal) and torch.equal(a.preds, b.preds) and torch.equal(a.y, b.y)
    if kind == "edos":
        assert torch.equal(a.embeddings, b.embeddings)
    # ... and the shared result of this module came from another predictor on the same buckets: the same numbers
    assert torch.equal(a.per_crystal, _result(kind)[0].per_crystal)


def test_forward_dataset_is_the_call_on_the_collated_batch():
    """forward_dataset against Predictor.__call__ on ds.collate of the same crystals, recorded and replayed, with its own buckets."""
    from dostransformer_amd.predict import Predictor
    c = _case("phonon")
    pred = Predictor(c["model"], per_crystal_keys=True)
    for sel in ([3, 9, 1, 20], [5, 6, 7, 8], [3, 9, 1, 20]):
        nmax = int(c["ds"].n_nodes.max())
        (dg, x, dsys), tgt = pred.forward_dataset(c["ds"], sel, nmax)
        dg, x, dsys, tgt = dg.clone(), x.clone(), dsys.clone(), tgt.clone()
        g = c["ds"].collate(sel, n_max=nmax)
        rg, rx, rs = pred(g)
        assert torch.equal(dg, rg) and torch.equal(x, rx) and torch.equal(dsys, rs) and torch.equal(tgt, g.phdos.float())
    n_ds = sum(key[-1] == "dataset" for key in pred._slots)
    assert n_ds >= 1 and len(pred._slots) == 2 * n_ds and pred.slot_hits >= 2


def test_a_predictor_without_per_crystal_keys_is_refused():
    from dostransformer_amd import evaluate
    from dostransformer_amd.predict import Predictor
    c = _case("phonon")
    with pytest.raises(ValueError, match="per-crystal keys"):
        evaluate.test_per_crystal(Predictor(c["model"]), c["ds"], batch_size=16)


# ---- the evaluator, float64 ---------------------------------------------------------------------------------------------------
L64, T64, H64, C64, BS64 = 3, 1, 32, 13, 5


def _soft64_mha(q, k, v, drop_mask=None):
    """The oracle's attention with a float64 softmax (tests/test_gpu_f64_per_crystal.py: what its 1e-12 is stated for)."""
    dim = q.shape[2]
    w = torch.bmm(q.transpose(0, 1), k.transpose(0, 1).transpose(1, 2)) * (dim ** -0.5)
    w = F.softmax(w, dim=-1)
    if drop_mask is not None:
        w = w * drop_mask.to(w.dtype)
    return torch.bmm(w, v.transpose(0, 1)).transpose(0, 1)


def test_float64_evaluator(monkeypatch):
    """Predictor64 with the module's per-crystal keys on, 13 crystals in chunks of 5, 5 and 3, float64 softmax on both sides: the
    table is the twin of its rows, every crystal's prediction within 1e-12 RMS of the oracle on that crystal alone with the metric
    bounds that follow from it, a second pass replays and is bitwise the first."""
    from oracle import dos_oracle as O
    from dostransformer_amd import evaluate, synth
    from dostransformer_amd import functional64 as F64
    from dostransformer_amd.batch import collate
    from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
    from dostransformer_amd.loader import DeviceDataset
    from dostransformer_amd.predict import Predictor64
    monkeypatch.setattr(O, "multihead_attention", _soft64_mha)
    monkeypatch.setattr(F64, "SOFTMAX64", True)
    torch.manual_seed(403)
    model = DOSTransformer_phonon(L64, T64, 118, 4, H64, DEV, 0.0).double()
    p64 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    crystals = synth.phonon_crystals(C64, 403)
    ds = DeviceDataset(crystals, DEV, dtype=torch.float64)
    model = model.set_program_dtype(torch.float64).to(DEV).eval()
    pred = Predictor64(model)
    with pytest.raises(ValueError, match="per-crystal keys"):
        evaluate.test_per_crystal(pred, ds, batch_size=BS64)
    model.set_per_crystal_keys(True)
    res = evaluate.test_per_crystal(pred, ds, batch_size=BS64)
    res = res._replace(per_crystal=res.per_crystal.clone(), preds=res.preds.clone(), y=res.y.clone())
    assert res.preds.dtype == res.y.dtype == torch.float64 and tuple(res.preds.shape) == (C64, 51)
    _assert_metrics(res.per_crystal, _twin(res.preds, res.y), "f64")
    assert [res.rmse, res.mse, res.mae, res.r2] == res.per_crystal.mean(0).tolist()
    assert len(res.as_reference()) == 4 and res.embeddings is None
    # the oracle, the reference's way
    loader = [collate([cr]) for cr in crystals]
    four = O.eval_phonon(p64, loader, L64, T64)
    with torch.no_grad():
        o_pred = torch.cat([O.dostransformer_phonon_forward(p64, g, L64, T64)[2] for g in loader])
    o_y = torch.stack([cr["phdos"].reshape(-1) for cr in crystals])
    assert torch.equal(res.y.cpu(), o_y)
    delta = torch.sqrt(((res.preds.cpu() - o_pred) ** 2).mean(1))
    print(f"float64: largest per-crystal RMS difference to the oracle {float(delta.max()):.3e}")
    assert float(delta.max()) <= 1e-12, float(delta.max())
    got, want = res.per_crystal.cpu(), _twin(o_pred, o_y)
    sst = ((o_y - o_y.mean(1, keepdim=True)) ** 2).sum(1)
    rr = got[:, 0] + want[:, 0]
    bound = torch.stack([delta, delta * rr, delta, 51 * delta * rr / sst], 1) + 1e-12
    assert bool(((got - want).abs() <= bound).all()), ((got - want).abs() / bound).max(0)
    for k, (a, b) in enumerate(zip((res.rmse, res.mse, res.mae, res.r2), four)):
        assert abs(a - b) <= float(bound.mean(0)[k]), (k, a, b)
    # second pass: replayed, bitwise
    misses, hits = pred.slot_misses, pred.slot_hits
    assert misses + hits == 3
    again = evaluate.test_per_crystal(pred, ds, batch_size=BS64)
    torch.cuda.synchronize()
    assert pred.slot_misses == misses and pred.slot_hits == hits + 3
    assert torch.equal(again.per_crystal, res.per_crystal) and torch.equal(again.preds, res.preds)
    assert (again.rmse, again.mse, again.mae, again.r2) == (res.rmse, res.mse, res.mae, res.r2)
