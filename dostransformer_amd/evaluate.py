"""Evaluation loops of the reference drivers (`utils.py:61-143`: ``test``, ``test_phonon``, ``r2``) on the
libdosx-backed modules.  Same signatures and return values as upstream, so
``main_eDOS.py:135-139`` / ``main_phDOS.py:124-128`` can import them from here unchanged; the metrics stay on
the device until the end of a batch (upstream round-trips every batch through sklearn on the host).

``test_per_crystal(predictor, ds)`` is the same evaluation at the reference's own setting, ``batch_size = 1``
(`main_eDOS.py:55-56`, `main_phDOS.py:52-55`), run in batched passes: the returned numbers are means over the crystals of
per-crystal metrics, which is what "the mean over batches" is when every batch holds one crystal.  ``test`` / ``test_phonon``
fed bigger batches return something else (one R2 over each flattened batch, a short last batch weighted like a full one).
"""
from __future__ import annotations

from typing import Callable, Iterable, List, NamedTuple, Optional

import numpy as np
import torch


def r2(x1: torch.Tensor, x2: torch.Tensor) -> float:
    """`utils.py:20-23`: ``r2_score(x1.flatten(), x2.flatten(), multioutput='variance_weighted')`` — on the
    flattened arrays this is 1 - SS_res / SS_tot with ``x1`` the target."""
    t, p = x1.double().flatten(), x2.double().flatten()
    return float(1.0 - ((t - p) ** 2).sum() / ((t - t.mean()) ** 2).sum())


def _pool_sum(x: torch.Tensor, g, num_graphs: int) -> torch.Tensor:
    """scatter_sum(x, batch) of `utils.py:96-99` (the per-crystal embedding the reference stores): dosx_graph_pool on the batch's
    graph_ptr - the kernel the decoder's own sum-pooling uses (`DOSTransformer.py:151-161`)."""
    from . import ops
    from .batch import graph_meta
    m = graph_meta(g, x.device)
    xf = x.detach().to(torch.float32).contiguous()
    out = torch.empty(num_graphs, xf.shape[1], dtype=torch.float32, device=x.device)
    ops.graph_pool(xf, m.graph_ptr, out.data_ptr(), xf.shape[1], num_graphs, xf.shape[1])
    return out.to(x.dtype)


def test_phonon(model, data_loader: Iterable, criterion: Optional[Callable] = None, r2: Callable = r2, device=None):
    """`utils.py:117-143`.  Returns (rmse, mse, mae, r2), each the mean over batches of the per-batch value.  A model with ONE
    output (Graphnetwork_phonon, or a predictor of it: its forward returns ``dos`` alone) is measured on that output."""
    criterion = criterion if criterion is not None else torch.nn.L1Loss()
    model.eval()
    n = 0
    rmse = mse = mae = r2s = 0.0
    with torch.no_grad():
        for batch in data_loader:
            if device is not None:
                batch.to(device)
            out = model(batch)
            preds_global, preds_system = (out, out) if torch.is_tensor(out) else (out[0], out[2])
            y = batch.phdos.reshape(preds_global.shape[0], -1).to(preds_system.dtype)
            mse_sys = ((y - preds_system) ** 2).mean(dim=1)
            rmse = rmse + torch.sqrt(mse_sys).mean()
            mse = mse + mse_sys.mean()
            mae = mae + criterion(preds_system, y)
            r2s += r2(y, preds_system)
            n += 1
    return float(rmse) / n, float(mse) / n, float(mae) / n, r2s / n


def test(model, data_loader: Iterable, criterion: Optional[Callable] = None, r2: Callable = r2, device=None):
    """`utils.py:61-112` (eDOS).  Target and prediction are clamped at 0 (`:76-78`).  Returns
    (rmse, mse, mae, r2, [[mp_id, preds, y, embeddings]]) with numpy arrays in the last item like upstream."""
    criterion = criterion if criterion is not None else torch.nn.L1Loss()
    model.eval()
    n = 0
    rmse = mse = mae = r2s = 0.0
    ids, preds, ys, embs = [], [], [], []
    with torch.no_grad():
        for batch in data_loader:
            if device is not None:
                batch.to(device)
            _, embeddings, preds_system = model(batch)
            nb = len(batch.mp_id)
            y = torch.clamp(batch.y_ft, min=0.0).reshape(nb, -1).to(preds_system.dtype)
            preds_system = torch.clamp(preds_system, min=0.0)
            mse_sys = ((y - preds_system) ** 2).mean(dim=1)
            rmse = rmse + torch.sqrt(mse_sys).mean()
            mse = mse + mse_sys.mean()
            mae = mae + criterion(preds_system, y)
            r2s += r2(y, preds_system)
            ids += list(batch.mp_id)
            preds.append(preds_system)
            ys.append(y)
            embs.append(_pool_sum(embeddings, batch, nb))
            n += 1
    preds_y = [[ids, torch.cat(preds).cpu().numpy(), torch.cat(ys).cpu().numpy(), torch.cat(embs).cpu().numpy()]]
    return float(rmse) / n, float(mse) / n, float(mae) / n, r2s / n, preds_y


# ---- the reference's evaluation at batch_size = 1, in batched passes ------------------------------------------------------------
def per_crystal_metrics_host(pred: torch.Tensor, y: torch.Tensor, clamp0: bool = False) -> torch.Tensor:
    """[C,4] float64 = (rmse, mse, mae, r2) of every row of ``pred`` against the same row of ``y`` ([C,S], any device): what
    `utils.py:76-89` / `:127-139` compute for a batch of ONE crystal, in torch float64.  ``clamp0``: both are clamped at 0 first
    (`utils.py:74-76`, eDOS).  r2 = 1 - sum (y-p)^2 / sum (y-mean(y))^2, the mean taken first; a constant target gives what IEEE
    division gives (-inf, or NaN when the error is 0 too), like ``r2`` on that row.  This is the definition that
    ``dosx_eval_metrics`` implements on the GPU (``ops.eval_metrics``); only the order of the sums differs."""
    p, t = pred.detach().to(torch.float64), y.detach().to(torch.float64)
    t = t.reshape(p.shape)
    if p.dim() != 2 or p.shape[1] < 1:
        raise ValueError(f"per_crystal_metrics_host: [C,S] rows with S >= 1, got {tuple(p.shape)}")
    if clamp0:
        p, t = torch.clamp(p, min=0.0), torch.clamp(t, min=0.0)
    S = p.shape[1]
    d = t - p
    sse = (d * d).sum(1)
    mse = sse / S
    sst = ((t - t.sum(1, keepdim=True) / S) ** 2).sum(1)
    return torch.stack([torch.sqrt(mse), mse, d.abs().sum(1) / S, 1.0 - sse / sst], 1)


class PerCrystalResult(NamedTuple):
    """What ``test_per_crystal`` returns.  rmse, mse, mae, r2: the reference's return values at batch_size = 1 (means over the
    crystals).  per_crystal: [C,4] float64 on the device, rows in the order of ``indices``.  preds, y: [C,S] in the program's
    dtype (eDOS: clamped at 0).  embeddings [C,H] (sum-pooled node embeddings, `utils.py:91`) and mp_id: eDOS only, else None."""
    rmse: float
    mse: float
    mae: float
    r2: float
    per_crystal: torch.Tensor
    preds: torch.Tensor
    y: torch.Tensor
    embeddings: Optional[torch.Tensor]
    mp_id: Optional[List]

    def as_reference(self):
        """The tuple the reference's loop returns: (rmse, mse, mae, r2) for phonon (`utils.py:143`), (rmse, mse, mae, r2,
        [[mp_id, preds, y, embeddings]]) with numpy arrays for eDOS (`utils.py:112`)."""
        head = (self.rmse, self.mse, self.mae, self.r2)
        if self.embeddings is None:
            return head
        return head + ([[self.mp_id, self.preds.cpu().numpy(), self.y.cpu().numpy(), self.embeddings.cpu().numpy()]],)


def test_per_crystal(predictor, ds, indices=None, batch_size: int = 64, weights=None) -> PerCrystalResult:
    """`utils.test` / `utils.test_phonon` over the crystals ``indices`` (default: all, in order) of a ``loader.DeviceDataset`` at
    the reference's batch size 1, computed in passes of ``batch_size`` crystals: ``predictor`` - a ``predict.Predictor`` with
    ``per_crystal_keys=True``, a ``Predictor64`` whose module has ``set_per_crystal_keys(True)``, or a predictor whose
    ``batch_independent`` is True (the GNN-only baselines: no attention; the metrics come from their one DOS output) - gives every crystal its
    batch-1 outputs from a batched pass, ``dosx_eval_metrics`` turns each row into its four metrics on the device, and the four
    means are read back once at the end.  Every chunk runs with the n_max of the whole selection (few recorded shapes), which is
    valid only because per-crystal keys make the outputs independent of it: without the flag this raises ``ValueError``.

    ``weights``: a [C] tensor or sequence, one weight per selected crystal in the order of ``indices`` - or True for the
    dataset's own (``ds.weights[indices]``): ``rmse``, ``mse``, ``mae`` and ``r2`` are then the weighted means ``sum_c w_c m_c /
    sum_c w_c`` of the per-crystal table, formed in float64 on the device and read back in the same single transfer;
    ``per_crystal`` is unchanged.  None (the default): the plain means."""
    from . import ops
    flag = getattr(predictor, "per_crystal_keys", None)
    if flag is None:
        flag = getattr(predictor.model, "per_crystal_keys", False)
    if not flag and not getattr(predictor, "batch_independent", False):
        raise ValueError("test_per_crystal needs per-crystal keys (Predictor(model, per_crystal_keys=True), or "
                         "model.set_per_crystal_keys(True) under Predictor64): without them a batched pass does not give the "
                         "batch-size-1 outputs the reference's metrics are computed from")
    if batch_size < 1:
        raise ValueError(f"test_per_crystal: batch_size must be positive, got {batch_size}")
    idx = np.arange(len(ds), dtype=np.int64) if indices is None else np.asarray(list(indices), np.int64)
    C = int(idx.shape[0])
    if C == 0:
        raise ValueError("test_per_crystal: no crystals selected")
    w = None
    if weights is not None:
        if weights is True:
            if ds.weights is None:
                raise ValueError("test_per_crystal(weights=True): the dataset holds no weights (ds.set_weights(w))")
            w = ds.weights.index_select(0, torch.from_numpy(idx).to(ds.device)).to(torch.float64)
        else:
            w = weights if torch.is_tensor(weights) else torch.as_tensor(weights, dtype=torch.float64)
            w = w.detach().to(ds.device, torch.float64).reshape(-1)
        if w.numel() != C:
            raise ValueError(f"test_per_crystal: {w.numel()} weights for {C} crystals")
    predictor.eval()
    edos = predictor.kind != "phonon"
    n_max = int(ds.n_nodes[idx].max())
    dev, table, embeddings = ds.device, None, None
    for row0 in range(0, C, batch_size):
        slot, N = predictor._run_dataset(ds, idx[row0:row0 + batch_size], n_max)
        dos_system, x = predictor._eval_outputs(slot)
        B, S = dos_system.shape
        if table is None:
            table = torch.empty(C, 4, dtype=torch.float64, device=dev)
            preds, ys = torch.empty(C, S, dtype=dos_system.dtype, device=dev), torch.empty(C, S, dtype=dos_system.dtype, device=dev)
            if edos:
                embeddings = torch.empty(C, x.shape[1], dtype=torch.float32, device=dev)
        rows = slice(row0, row0 + B)
        # (outside the bucket's recording: the output pointers move with the chunk)
        ops.eval_metrics(dos_system, predictor._target(slot).view(B, S), table[rows], clamp0=edos, pred_out=preds[rows], y_out=ys[rows])
        if edos:
            # the bucket's graph_ptr ends at its N real nodes: the ghost rows behind them belong to no crystal's sum
            H = x.shape[1]
            ops.graph_pool(x, slot.g.meta.graph_ptr, embeddings[rows].data_ptr(), H, B, H)
    means = table.mean(0) if w is None else (table * w[:, None]).sum(0) / w.sum()
    rmse, mse, mae, r2_ = means.tolist()                               # the one transfer
    ops.check_exchanges(dev)            # (the host has just waited for the device: a stalled exchange voids these metrics)
    mp_id = [ds.mp_id[i] for i in idx] if edos and ds.mp_id is not None else None
    return PerCrystalResult(rmse, mse, mae, r2_, table, preds, ys, embeddings, mp_id)


test_per_crystal.__test__ = False          # (a library function named like the reference's, not a pytest test)


class FunctionalsResult(NamedTuple):
    """What ``functionals_per_crystal`` returns.  pred, y: [C,K] float64 on the device, ``F_k`` of every crystal's prediction
    and target (times its ``scale``); mae: [K] host floats, the mean over the crystals of ``|pred - y|``; names: the K rows.
    ratio_pred, ratio_y [C,R] (device), ratio_mae [R] and ratio_names: the same for the table's declared ratios (empty: R = 0)."""
    pred: torch.Tensor
    y: torch.Tensor
    mae: List[float]
    names: List[str]
    ratio_pred: torch.Tensor
    ratio_y: torch.Tensor
    ratio_mae: List[float]
    ratio_names: List[str]


def functionals_per_crystal(result: PerCrystalResult, fn, scale=None) -> FunctionalsResult:
    """The linear functionals ``fn`` (a ``functionals.Functionals`` or a [K,S] table: cumulative DOS, moments, a window, C_V(T))
    of the predictions and targets ``test_per_crystal`` left on the device - one ``dosx_eval_functionals`` launch in float64, no
    host copy of ``preds`` / ``y``.  ``scale``: None, or [C] factors, one per crystal in the result's order (eDOS: the ``y_max``
    that undoes the target's normalisation; a ratio does not depend on it).  The declared ratios (``centre = m1 / m0``) are
    formed from those values in float64 on the device.  Every mean absolute error comes back in ONE transfer."""
    from . import functionals as _fn
    from . import ops
    fn = _fn.as_functionals(fn)
    if fn.norm_rows:
        raise ValueError("functionals_per_crystal: the table has normalised rows, which only the loss divides - report a ratio through "
                         "the plain table's declared ratios (functionals.moments: centre = m1 / m0)")
    preds, ys = result.preds, result.y
    C, S = int(preds.shape[0]), int(preds.shape[1])
    if fn.S != S:
        raise ValueError(f"functionals_per_crystal: the table has {fn.S} columns, the result {S} energy bins")
    dev = preds.device
    sc = None
    if scale is not None:
        sc = scale if torch.is_tensor(scale) else torch.as_tensor(scale, dtype=torch.float64)
        sc = sc.detach().to(dev, torch.float64).reshape(-1).contiguous()
        if sc.numel() != C:
            raise ValueError(f"functionals_per_crystal: {sc.numel()} scales for {C} crystals")
    out = torch.empty(C, 2, fn.K, dtype=torch.float64, device=dev)
    ops.eval_functionals(preds.contiguous(), ys.contiguous(), fn.table.to(dev, preds.dtype).contiguous(), out, scale=sc)
    fp, fy = out[:, 0], out[:, 1]
    num = torch.tensor([a for _, a, _ in fn.ratios], dtype=torch.int64, device=dev)
    den = torch.tensor([b for _, _, b in fn.ratios], dtype=torch.int64, device=dev)
    rp, ry = fp[:, num] / fp[:, den], fy[:, num] / fy[:, den]
    maes = torch.cat([(fp - fy).abs().mean(0), (rp - ry).abs().mean(0)]).tolist()          # the one transfer
    return FunctionalsResult(fp, fy, maes[:fn.K], list(fn.names), rp, ry, maes[fn.K:], [n for n, _, _ in fn.ratios])
