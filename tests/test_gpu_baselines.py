"""The GNN-only baselines (Graphnetwork_phonon, Graphnetwork, mlp) through the fused drivers on a real MI355X: the pair-head
kernels (csrc/pair_head.hip) against float64 torch on the same fp32 operands, train.Trainer on the reference's g10 fixtures and
against the float64 oracle, replay / graph / step_dataset against the eager step, predict.Predictor and
evaluate.test_per_crystal."""
import numpy as np
import pytest
import torch

from tests.gpu_util import DEV, EPS32, bound_ratio
from tests.test_gpu_models import DOS_RMSE, F64_MAX, F64_MEDIAN, F64_P99, _load_model, relerr
from tests.util import batch_from, load, maxabs, rmse, sub

pytestmark = pytest.mark.gpu
SLOPE = float(np.float32(0.01))            # the slope the kernels get (fp32), as the float64 reference's operand too


def _ops():
    from dostransformer_amd import ops
    return ops


# ---- the kernels ---------------------------------------------------------------------------------------------------
SHAPES = [(51, 1, 16), (51, 3, 64), (201, 17, 136), (201, 64, 128), (51, 65, 256), (201, 5, 512)]


def _operands(S, B, H):
    """fp32 operands with one pre-activation exactly 0 (its gate takes the slope, torch's rule) and one all-zero ddos row."""
    g = torch.Generator().manual_seed(1000 * S + 10 * B + H)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).to(torch.float32)
    e1, c, w2, b2, ddos = r(S, H), r(B, H), r(H) / H ** 0.5, r(1), r(B, S)
    s0, b0, h0 = S // 2, B - 1, H - 3
    c[b0, h0] = -e1[s0, h0]
    ddos[B // 2] = 0.0
    if B == 1:                               # (the only row cannot be the zero one: zero a column instead, and keep (s0, b0) live)
        ddos = r(B, S)
        ddos[0, (s0 + 1) % S] = 0.0
    assert float(e1[s0, h0] + c[b0, h0]) == 0.0 and float(ddos[b0, s0]) != 0.0
    return [t.to(DEV) for t in (e1, c, w2, b2, ddos)]


def _reference(e1, c, w2, b2, ddos):
    """float64 torch on the same operands: results and, per element, the sum of the absolute values of its terms."""
    e1, c, w2, b2, ddos = (t.double() for t in (e1, c, w2, b2, ddos))
    pre = e1[:, None, :] + c[None, :, :]                                     # [S, B, H]
    act = torch.where(pre > 0, pre, SLOPE * pre)
    gate = torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, SLOPE))
    d = ddos.T[:, :, None]                                                   # [S, B, 1]
    t_dos, t_g, t_w = act * w2, d * w2 * gate, d * act
    ref = dict(dos=(t_dos.sum(2) + b2).T, de1=t_g.sum(1), dc=t_g.sum(0), dw2=t_w.sum((0, 1)), db2=ddos.sum().reshape(1))
    mag = dict(dos=(t_dos.abs().sum(2) + b2.abs()).T, de1=t_g.abs().sum(1), dc=t_g.abs().sum(0), dw2=t_w.abs().sum((0, 1)),
               db2=ddos.abs().sum().reshape(1))
    return ref, mag


def _run_kernels(e1, c, w2, b2, ddos):
    o = _ops()
    S, H = e1.shape
    B = c.shape[0]
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    dos, de1, dc = nan(B, S), nan(S, H), nan(B, H)
    rows = o.pair_head_partial_rows(S, B)
    part = nan(rows, H + 1)
    o.pair_head_fwd(e1, c, w2, b2, dos, SLOPE)
    o.pair_head_bwd(ddos, e1, c, w2, de1, dc, part, SLOPE)
    dw2, db2 = nan(H), nan(1)
    sink = o.GradSink(torch.device(DEV))
    sink.add(part, 0, dw2, rows, H + 1, H)
    sink.add(part, H, db2, rows, H + 1, 1)
    sink.flush()
    torch.cuda.synchronize()
    return dict(dos=dos, de1=de1, dc=dc, dw2=dw2, db2=db2)


@pytest.mark.parametrize("S,B,H", SHAPES)
def test_pair_head_kernels_against_float64_torch(S, B, H):
    """|got - ref| <= (n + 4) 2^-24 sum|terms| per element, n the number of summed terms (H for dos, B for dE1, S for dC, S B for
    dw2 / db2): a sum of n fp32 products in any order errs by at most (n - 1 + a few roundings per term) 2^-24 of that.  The fp32
    sum E1 + C has the sign of the exact sum (rounding is monotonic and never reaches 0 from a non-zero value), so every gate
    agrees with the float64 reference's and no element is exempt - the one with pre == 0 exactly included."""
    ops_ = _operands(S, B, H)
    got = _run_kernels(*ops_)
    ref, mag = _reference(*ops_)
    n = dict(dos=H, de1=B, dc=S, dw2=S * B, db2=S * B)
    worst = {k: bound_ratio(got[k], ref[k].to(DEV), mag[k].to(DEV), n[k] + 4, what=f"pair_head {k} S{S} B{B} H{H}") for k in ref}
    assert all(w <= 1.0 for w in worst.values()), worst
    again = _run_kernels(*ops_)
    assert all(torch.equal(got[k], again[k]) for k in got)                   # fixed summation order: bitwise run to run


# ---- the three modules ---------------------------------------------------------------------------------------------
def _make(name, H=16, L=3):
    if name == "ph":
        from dostransformer_amd.embedder_phDOS.graphnetwork_phonon import Graphnetwork_phonon
        return Graphnetwork_phonon(L, 118, 4, H, 51, DEV)
    if name == "gn":
        from dostransformer_amd.embedder_eDOS.graphnetwork import Graphnetwork
        return Graphnetwork(L, 200, 41, 2, H, 201, DEV)
    from dostransformer_amd.embedder_eDOS.mlp import mlp
    return mlp(L, 200, 41, 2, H, 201, DEV)


def _batch(name, B, seed, dtype=torch.float32):
    from dostransformer_amd import synth
    return (synth.phonon_batch if name == "ph" else synth.edos_batch)(B, seed=seed, dtype=dtype)


@pytest.mark.parametrize("name", ["ph", "gn", "mlp"])
def test_trainer_matches_the_reference_trajectory(name):
    """train.Trainer on the g10 fixture of the reference's own run: the bounds of test_fused_trainer_matches_golden_trajectory
    (loss 1e-4, p1 2e-6, p3 5e-6) and G8's gradient rule (relerr < 2e-3 per tensor); dead parameters stay bitwise at p0."""
    from dostransformer_amd.train import Trainer
    z = load(f"g10_baselines_{name}.npz")
    model = _load_model(_make(name), z)
    g = batch_from(z).to(DEV, dtype=torch.float32)
    tr = Trainer(model, lr=1e-4)
    loss = tr.forward_backward(g)
    print(f"g10 {name}: loss {float(loss):.8f} (reference {float(z['loss']):.8f})")
    assert abs(float(loss) - float(z["loss"])) < 1e-4
    out = tr.last_outputs
    dos = out[0] if name == "gn" else out
    assert rmse(dos.cpu(), z["dos"]) < DOS_RMSE
    if name == "gn":
        assert rmse(out[1].cpu(), z["x_nodes"]) < DOS_RMSE
    dead = set(str(s) for s in z["dead_params"])
    fp = model.flat_params(g)
    assert set(fp.G) == {k for k, _ in model.named_parameters()} - dead
    for k, gr in fp.G.items():
        e = relerr(gr, z["g/" + k])
        assert e < 2e-3, (k, e)
    tr.optimizer_step()
    p0, p1, p3 = sub(z, "p0/"), sub(z, "p1/"), sub(z, "p3/")
    for k, v in model.state_dict().items():
        assert maxabs(v.cpu(), p1[k]) < 2e-6, ("p1", k)
    tr.step(g)
    tr.step(g)
    for k, v in model.state_dict().items():
        assert maxabs(v.cpu(), p3[k]) < 5e-6, ("p3", k)
    for k in dead:
        assert torch.equal(model.state_dict()[k].cpu(), p0[k].float()), k
        assert dict(model.named_parameters())[k].grad is None, k


def _oracle64(name, params, g32, L=3):
    """Outputs, one-output loss and gradients of the float64 oracle on float64 copies of the fp32 parameters and batch."""
    from oracle import dos_oracle as O
    g64 = g32.to("cpu", dtype=torch.float64)
    leaves = {k: v.detach().cpu().to(torch.float64).requires_grad_(True) for k, v in params.items() if v.is_floating_point()}
    if name == "ph":
        dos = O.graphnetwork_phonon_forward(leaves, g64, L)
        loss = torch.sqrt(((dos - g64.phdos.reshape(dos.shape)) ** 2).mean())
    else:
        dos, _ = O.graphnetwork_forward(leaves, g64, L if name == "gn" else 0)       # (mlp: Graphnetwork without processors)
        y = torch.clamp(g64.y_ft, min=0.0).reshape(dos.shape)
        loss = torch.sqrt(((y - dos) ** 2).mean(1)).mean()
    names = list(leaves)
    gr = torch.autograd.grad(loss, [leaves[k] for k in names], allow_unused=True)
    return dos.detach(), loss.detach(), dict(zip(names, gr))


@pytest.mark.parametrize("name,H", [("ph", 64), ("ph", 128), ("ph", 256), ("gn", 64), ("gn", 128), ("gn", 256), ("mlp", 256)])
def test_trainer_against_the_float64_oracle(name, H):
    """5 synthetic crystals: DOS within DOS_RMSE, every gradient tensor within the phonon element-error bounds of
    tests/test_gpu_models.py (max / 99th percentile / median of |got - ref| / max|ref|)."""
    from dostransformer_amd.train import Trainer
    torch.manual_seed(0)
    model = _make(name, H)
    params = {k: v.detach().clone() for k, v in model.state_dict().items()}
    g = _batch(name, 5, seed=70)
    dos64, loss64, grads64 = _oracle64(name, params, g)
    model = model.to(DEV)
    tr = Trainer(model, lr=1e-4)
    loss = tr.forward_backward(g.to(DEV))
    out = tr.last_outputs
    dos = out[0] if name == "gn" else out
    assert rmse(dos.cpu(), dos64) < DOS_RMSE
    assert abs(float(loss) - float(loss64)) < 2e-4
    fp = model.flat_params(g)
    worst, worst99, worst50 = (0.0, None), (0.0, None), (0.0, None)
    for k, gr in grads64.items():
        if gr is None or float(gr.abs().max()) == 0.0 and k not in fp.G:
            assert k not in fp.G, k
            continue
        e = (fp.G[k].cpu().double() - gr).abs().reshape(-1) / (gr.abs().max() + 1e-6)
        worst = max(worst, (float(e.max()), k))
        if e.numel() >= 256:
            worst99 = max(worst99, (float(torch.quantile(e[:1 << 24], 0.99)), k))
            worst50 = max(worst50, (float(e.median()), k))
    print(f"oracle-live {name} H{H}: max {worst[0]:.3e} at {worst[1]}; p99 {worst99[0]:.3e} at {worst99[1]}; "
          f"median {worst50[0]:.3e} at {worst50[1]}")
    assert worst[0] < F64_MAX and worst99[0] < F64_P99 and worst50[0] < F64_MEDIAN, (worst, worst99, worst50)


def _three_steps(name, mode, batches):
    from dostransformer_amd.train import Trainer
    torch.manual_seed(3)
    model = _make(name, 64).to(DEV)
    tr = Trainer(model, lr=1e-3, **mode)
    losses = [tr.step(b).clone() for b in batches]
    torch.cuda.synchronize()
    return torch.stack(losses), {k: v.clone() for k, v in model.state_dict().items()}


@pytest.mark.parametrize("name", ["ph", "gn", "mlp"])
def test_replay_and_graph_steps_are_bitwise_the_eager_step(name):
    from dostransformer_amd.batch import bucket_sizes, pad_batch
    raw = [_batch(name, 4, seed=80 + k).to(DEV) for k in range(2)]
    batches = []
    for b in raw:                                           # the eager run gets the buckets the replayed runs pad to
        batches.append(pad_batch(b, *bucket_sizes(b.meta.num_nodes, b.meta.num_edges, 8, 128)))
    batches.append(batches[0])                              # the third step replays the first bucket
    l0, p0 = _three_steps(name, {}, batches)
    for mode in (dict(replay=True), dict(graph=True)):
        l1, p1 = _three_steps(name, mode, batches)
        assert torch.equal(l0, l1), (mode, l0, l1)
        assert all(torch.equal(p0[k], p1[k]) for k in p0), mode


@pytest.mark.parametrize("name", ["ph", "mlp"])
def test_step_dataset_is_bitwise_the_step_on_the_collated_batch(name):
    from dostransformer_amd import synth
    from dostransformer_amd.batch import collate
    from dostransformer_amd.loader import DeviceDataset
    from dostransformer_amd.train import Trainer
    cs = synth.phonon_crystals(9, 90, torch.float32) if name == "ph" else synth.edos_crystals(9, 91, torch.float32)
    ds = DeviceDataset(cs, DEV)
    sel = [[0, 3, 5, 7], [1, 2, 8], [0, 3, 5, 7]]
    res = []
    for via_ds in (False, True):
        torch.manual_seed(4)
        model = _make(name, 64).to(DEV)
        tr = Trainer(model, lr=1e-3, replay=True)
        # (the host collate: its message-GEMM tile table is the one the device collate writes into the bucket)
        losses = [(tr.step_dataset(ds, s) if via_ds else tr.step(collate([cs[j] for j in s]).to(DEV))).clone() for s in sel]
        torch.cuda.synchronize()
        res.append((torch.stack(losses), {k: v.clone() for k, v in model.state_dict().items()}))
    assert torch.equal(res[0][0], res[1][0])
    assert all(torch.equal(res[0][1][k], res[1][1][k]) for k in res[0][1])


def test_trainer_checkpoint_resumes_bitwise():
    """state_dict / load_state_dict of a baseline's trainer: two steps, save, a third step == load into a fresh trainer, one step."""
    from dostransformer_amd.train import Trainer
    g = _batch("mlp", 4, seed=120).to(DEV)
    torch.manual_seed(7)
    model = _make("mlp", 64).to(DEV)
    tr = Trainer(model, lr=1e-3)
    tr.step(g)
    tr.step(g)
    sd_m, sd_t = {k: v.clone() for k, v in model.state_dict().items()}, tr.state_dict()
    assert sd_t["step"] == 2 and not any("edge_encoder" in k or "node_encoder_prompt" in k for k in sd_t["exp_avg"])
    l3 = tr.step(g).clone()
    model2 = _make("mlp", 64)
    model2.load_state_dict(sd_m)
    model2 = model2.to(DEV)
    tr2 = Trainer(model2, lr=1e-3)
    tr2.load_state_dict(sd_t)
    assert torch.equal(tr2.step(g), l3)
    a, b = model.state_dict(), model2.state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)


# ---- Predictor / test_per_crystal ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ph", "gn", "mlp"])
def test_predictor_is_bitwise_the_factored_forward_and_within_rmse_of_the_module(name):
    from dostransformer_amd.batch import bucket_sizes, pad_batch
    from dostransformer_amd.predict import Predictor
    torch.manual_seed(5)
    model = _make(name, 64).to(DEV).eval()
    pred = Predictor(model)
    assert pred.batch_independent
    for seed in (100, 101, 100):                            # the third call replays the first bucket
        g = _batch(name, 4, seed=seed).to(DEV)
        out = pred(g)
        gp = pad_batch(g, *bucket_sizes(g.meta.num_nodes, g.meta.num_edges, 8, 128))
        with torch.no_grad():
            want = model._program_fwd(model.flat_params(gp).P, gp, gp.meta, factored_head=True)[:-1]
            plain = model(g)
        torch.cuda.synchronize()
        if name == "gn":
            assert isinstance(out, tuple) and len(out) == 2
            assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1][:g.meta.num_nodes])
            assert tuple(out[1].shape) == tuple(plain[1].shape)
            assert rmse(out[0].cpu(), plain[0].cpu()) < DOS_RMSE and rmse(out[1].cpu(), plain[1].cpu()) < DOS_RMSE
        else:
            assert torch.is_tensor(out) and torch.equal(out, want[0])
            assert rmse(out.cpu(), plain.cpu()) < DOS_RMSE
    assert (pred.slot_misses, pred.slot_hits) == (2, 1)


@pytest.mark.parametrize("name", ["ph", "gn", "mlp"])
def test_per_crystal_evaluation_equals_the_batch_1_loop(name):
    """test_per_crystal over 10 crystals in passes of 4 against the module at batch size 1 with the metrics in float64 torch
    (evaluate.per_crystal_metrics_host): predictions within 4e-6 x their scale, the four metrics within 1e-4 - the tolerances of
    tests/test_gpu_eval_per_crystal.py."""
    from dostransformer_amd import evaluate, synth
    from dostransformer_amd.batch import collate
    from dostransformer_amd.loader import DeviceDataset
    from dostransformer_amd.predict import Predictor
    edos = name != "ph"
    cs = synth.edos_crystals(10, 111, torch.float32) if edos else synth.phonon_crystals(10, 110, torch.float32)
    if edos:
        for cr in cs:
            cr["y_ft"] = cr["y_ft"] - 0.3                    # so that the clamp matters
    torch.manual_seed(6)
    model = _make(name, 64).to(DEV).eval()
    ds = DeviceDataset(cs, DEV)
    res = evaluate.test_per_crystal(Predictor(model), ds, batch_size=4)
    rows, embs = [], []
    with torch.no_grad():
        for cr in cs:
            g1 = collate([cr]).to(DEV, dtype=torch.float32)
            out = model(g1)
            rows.append((out[0] if name == "gn" else out).float().clone())
            if name == "gn":
                embs.append(out[1].double().sum(0))
    want = torch.cat(rows)
    y = torch.stack([cr["y_ft" if edos else "phdos"].reshape(-1) for cr in cs]).to(DEV)
    sc = max(float(want.abs().max()), 1.0)
    wantc = torch.clamp(want, min=0.0) if edos else want
    assert float((res.preds - wantc).abs().max()) <= 4e-6 * sc
    assert torch.equal(res.y, torch.clamp(y, min=0.0) if edos else y)
    table = evaluate.per_crystal_metrics_host(want, y, clamp0=edos)
    got = torch.tensor([res.rmse, res.mse, res.mae, res.r2], dtype=torch.float64)
    assert float((got - table.mean(0).cpu()).abs().max()) < 1e-4, (got, table.mean(0))
    assert float((res.per_crystal - table).abs().max()) < 1e-4
    if edos:
        assert res.embeddings is not None and tuple(res.embeddings.shape) == (10, 64) and res.mp_id == [cr["mp_id"] for cr in cs]
        if name == "gn":
            xs = max(float(torch.stack(embs).abs().max()), 1.0)
            assert float((res.embeddings.double() - torch.stack(embs)).abs().max()) <= 40 * (4e-6 + 2.0 ** -23) * xs
    else:
        assert res.embeddings is None
    # the DOSTransformer case keeps its refusal
    from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
    with pytest.raises(ValueError, match="per-crystal keys"):
        evaluate.test_per_crystal(Predictor(DOSTransformer_phonon(3, 1, 118, 4, 64, DEV, 0.0).to(DEV)), ds)
