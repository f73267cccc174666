"""The float64 Graphnetwork_phonon through the fused float64 drivers on a real MI355X: the float64 pair-head kernels
(csrc/pair_head_f64.hip) against a long-double host reference, train64.GraphnetworkTrainer64 on the reference's own g10 run and
against the float64 oracle, the factored program against the module's own, replay / padding / step_dataset / promotion against
the eager step, checkpoints, predict.Predictor64 and the evaluators.  Bounds: the project's float64 bars (tests/test_gpu_f64.py,
tests/test_gpu_train64.py): outputs and losses 1e-12, gradients 1e-10 relative per tensor, parameters after 3 steps 1e-9."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.f64_ref import SENT, check_sum, guarded as _guarded
from tests.util import batch_from, load, maxabs, rmse, sub

pytestmark = pytest.mark.gpu
DEV = "cuda"
SLOPE = 0.01
L_ = 3
BUCKET = (8, 128)


def _ops():
    from dostransformer_amd import ops
    return ops


def _relmax(got, ref):
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-300))


# =====================================================================================================================
# 1. the kernels
# =====================================================================================================================
# fewer bins than waves, B past one "b" block, H no multiple of 16 or 64, the widest H, the headline shape
SHAPES = [(1, 1, 8), (3, 2, 16), (5, 1, 24), (51, 3, 64), (51, 65, 136), (51, 64, 128), (201, 17, 256), (7, 5, 512)]


def _operands(S, B, H):
    """float64 operands with one pre-activation exactly 0 under a live ddos (its gate takes the slope, torch's rule) and one
    all-zero ddos row - a zero column when B = 1 (the only row cannot be the zero one)."""
    g = torch.Generator().manual_seed(1000 * S + 10 * B + H)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    e1, c, w2, b2, ddos = r(S, H), r(B, H), r(H) / H ** 0.5, r(1), r(B, S)
    s0, b0, h0 = S // 2, B - 1, H - 3
    c[b0, h0] = -e1[s0, h0]
    if B == 1:
        ddos[0, (s0 + 1) % S] = 0.0 if S > 1 else ddos[0, 0]
    else:
        ddos[B // 2 if B // 2 != b0 else 0] = 0.0
    assert float(e1[s0, h0] + c[b0, h0]) == 0.0 and float(ddos[b0, s0]) != 0.0
    return [t.to(DEV) for t in (e1, c, w2, b2, ddos)]


def _reference(e1, c, w2, b2, ddos):
    """Long double on the host from the same float64 operands: results and, per element, the sum of its terms' magnitudes."""
    L = np.longdouble
    assert np.finfo(L).eps <= 2.0 ** -63, "the host reference needs a long double wider than double"
    e1, c, w2, b2, ddos = (t.cpu().numpy().astype(L) for t in (e1, c, w2, b2, ddos))
    pre = e1[:, None, :] + c[None, :, :]                                     # [S, B, H]
    act = np.where(pre > 0, pre, L(SLOPE) * pre)
    gate = np.where(pre > 0, L(1), L(SLOPE))
    d = ddos.T[:, :, None]                                                   # [S, B, 1]
    t_dos, t_g, t_w = act * w2, d * w2 * gate, d * act
    ref = dict(dos=(t_dos.sum(2) + b2).T, de1=t_g.sum(1), dc=t_g.sum(0), dw2=t_w.sum((0, 1)), db2=ddos.sum().reshape(1))
    mag = dict(dos=(np.abs(t_dos).sum(2) + np.abs(b2)).T, de1=np.abs(t_g).sum(1), dc=np.abs(t_g).sum(0),
               dw2=np.abs(t_w).sum((0, 1)), db2=np.abs(ddos).sum().reshape(1))
    return ref, mag


def _run_kernels(e1, c, w2, b2, ddos):
    o = _ops()
    S, H = e1.shape
    B = c.shape[0]
    rows = o.pair_head_partial_rows(S, B)
    assert rows == S
    bufs = dict(dos=_guarded(B, S), de1=_guarded(S, H), dc=_guarded(B, H), part=_guarded(rows, H + 1), dw2=_guarded(H), db2=_guarded(1))
    v = {k: b[0] for k, b in bufs.items()}
    o.pair_head_fwd64(e1, c, w2, b2, v["dos"], SLOPE)
    o.pair_head_bwd64(ddos, e1, c, w2, v["de1"], v["dc"], v["part"], SLOPE)
    o.colsum64(v["part"][:, :H], v["dw2"])
    o.colsum64(v["part"][:, H:], v["db2"])
    torch.cuda.synchronize()
    for k, (view, whole) in bufs.items():
        assert bool((whole[:2] == SENT).all()) and bool((whole[-2:] == SENT).all()), f"{k}: written outside the buffer"
        assert not bool(torch.isnan(view).any()), f"{k}: elements left unwritten"
    return {k: v[k].clone() for k in ("dos", "de1", "dc", "dw2", "db2")}


@pytest.mark.parametrize("S,B,H", SHAPES)
def test_pair_head64_kernels_against_long_double(S, B, H):
    """|got - ref| <= (n + 4) 2^-53 sum|terms| per element, n the number of summed terms (H for dos, B for dE1, S for dC, S B for
    dw2 / db2 after colsum64): a sum of n float64 products in any order errs by at most (n - 1 + a few roundings per term) 2^-53 of
    that.  The float64 sum E1 + C has the sign of the exact sum (rounding is monotonic and never reaches 0 from a non-zero
    value), so every gate agrees with the reference's and no element is exempt - the one with pre == 0 exactly included."""
    operands = _operands(S, B, H)
    got = _run_kernels(*operands)
    ref, mag = _reference(*operands)
    n = dict(dos=H, de1=B, dc=S, dw2=S * B, db2=S * B)
    worst = {k: check_sum(got[k], ref[k], mag[k], n[k]) for k in ref}           # asserts the bound per element
    print(f"pair_head64 S{S} B{B} H{H}: worst error / bound " + ", ".join(f"{k} {w:.3f}" for k, w in worst.items()))
    again = _run_kernels(*operands)
    assert all(torch.equal(got[k], again[k]) for k in got)                   # fixed summation order: bitwise run to run


def test_pair_head64_wrappers_check_dtype_and_layout():
    o = _ops()
    e1, c, w2, b2, ddos = _operands(5, 3, 16)
    dos = torch.empty(3, 5, dtype=torch.float64, device=DEV)
    with pytest.raises(TypeError):
        o.pair_head_fwd64(e1.float(), c, w2, b2, dos)
    with pytest.raises((TypeError, ValueError)):
        o.pair_head_fwd64(e1, c, w2, b2, torch.empty(5, 3, dtype=torch.float64, device=DEV).t())
    with pytest.raises(ValueError):
        o.pair_head_fwd64(e1, c[:, :8], w2, b2, dos)
    with pytest.raises(ValueError):
        o.pair_head_bwd64(ddos, e1, c, w2, torch.empty_like(e1), torch.empty_like(c), torch.empty(5, 16, dtype=torch.float64, device=DEV))


# =====================================================================================================================
# 2 - 4. GraphnetworkTrainer64: the reference's trajectory, the oracle, the module's own program
# =====================================================================================================================
def _gn(H, L=L_, seed=0):
    from dostransformer_amd.embedder_phDOS.graphnetwork_phonon import Graphnetwork_phonon
    torch.manual_seed(seed)
    return Graphnetwork_phonon(L, 118, 4, H, 51, "cpu").double()


def _trainer(model, **kw):
    from dostransformer_amd.train64 import GraphnetworkTrainer64
    return GraphnetworkTrainer64(model, **kw)


def test_trainer64_follows_the_reference_trajectory():
    """g10_baselines_ph.npz is the reference's own float64 run: loss and dos to 1e-12, every gradient to 1e-10 relative, the
    parameters after 1 and 3 AdamW steps to 1e-9; the gradient key set is the fixture's live set and dead parameters stay
    bitwise at p0 with grad None.  The fixture's smallest |pre-activation| (>= 1e-5) rules out a gate that differs."""
    z = load("g10_baselines_ph.npz")
    assert float(z["min_abs_pre"]) >= 1e-5
    model = _gn(16)
    model.load_state_dict(sub(z, "p0/"))
    model = model.to(DEV)
    g = batch_from(z).to(DEV)
    tr = _trainer(model, lr=1e-4)
    loss = tr.forward_backward(g)
    assert loss.dtype == torch.float64 and loss.dim() == 0 and loss.is_cuda
    print(f"g10 float64: loss {float(loss):.15f} (reference {float(z['loss']):.15f})")
    assert abs(float(loss) - float(z["loss"])) <= 1e-12
    dos = tr.last_outputs
    assert dos.dtype == torch.float64 and tuple(dos.shape) == tuple(z["dos"].shape)
    assert maxabs(dos.cpu(), z["dos"]) <= 1e-12
    dead = set(str(s) for s in z["dead_params"])
    fp = model.flat_params(g)
    assert set(fp.G) == {k for k, _ in model.named_parameters()} - dead
    worst = max((_relmax(gr.cpu(), torch.from_numpy(z["g/" + k])), k) for k, gr in fp.G.items())
    print(f"g10 float64: worst per-tensor gradient error {worst[0]:.2e} at {worst[1]}")
    assert worst[0] <= 1e-10, worst
    tr.optimizer_step()
    p0, p1, p3 = sub(z, "p0/"), sub(z, "p1/"), sub(z, "p3/")
    for k, v in model.state_dict().items():
        assert maxabs(v.cpu(), p1[k]) <= 1e-9, ("p1", k)
    tr.step(g)
    tr.step(g)
    for k, v in model.state_dict().items():
        assert maxabs(v.cpu(), p3[k]) <= 1e-9, ("p3", k)
    for k in dead:
        assert torch.equal(model.state_dict()[k].cpu(), p0[k]), k
        assert dict(model.named_parameters())[k].grad is None, k


# seeds of the parameters and of the five crystals, chosen on the host so that the oracle's smallest |E1[s] + C[b]| stays
# >= 1e-9 over the three steps (asserted below): no gate can differ between the oracle and the kernels
ORACLE_CASES = [(64, False, 0, 70), (128, False, 0, 70), (256, False, 0, 70), (64, True, 0, 70)]


@pytest.mark.parametrize("H,prompt,pseed,bseed", ORACLE_CASES)
def test_trainer64_against_the_float64_oracle(monkeypatch, H, prompt, pseed, bseed):
    """Five synthetic crystals, three steps: oracle.graphnetwork_phonon_forward with autograd and torch.optim.AdamW on the CPU
    against GraphnetworkTrainer64 - dos, loss and every gradient at step 1, every parameter after step 3."""
    from oracle import dos_oracle as O
    from dostransformer_amd import synth
    pre_min = []

    def head(p, energies, graph):                       # the oracle's own head, with a look at its pre-activations
        h = O._linear(p, "out_layer.0", torch.cat([energies, graph], 2))
        pre_min.append(float(h.detach().abs().min()))
        return O._linear(p, "out_layer.2", F.leaky_relu(h)).squeeze(2).T

    monkeypatch.setattr(O, "_gn_head", head)
    base = _gn(H, seed=pseed)
    g = synth.phonon_batch(5, seed=bseed, dtype=torch.float64)
    if prompt:                  # 118 + H/2 wide nodes take node_encoder_prompt (graphnetwork_phonon.py:150-153)
        g.x = torch.cat([g.x, torch.randn(g.x.shape[0], H // 2, generator=torch.Generator().manual_seed(2), dtype=torch.float64)], 1)
    lr = 1e-3
    pr = {k: (torch.nn.Parameter(v.detach().clone()) if v.is_floating_point() else v.clone()) for k, v in base.state_dict().items()}
    opt = torch.optim.AdamW([v for v in pr.values() if isinstance(v, torch.nn.Parameter)], lr=lr, weight_decay=1e-2)
    model = copy.deepcopy(base).to(DEV)
    tr = _trainer(model, lr=lr)
    gd = g.clone().to(DEV)
    for step in range(3):
        opt.zero_grad()
        ref_dos = O.graphnetwork_phonon_forward(pr, g, L_)
        ref = torch.sqrt(F.mse_loss(ref_dos, g.phdos.reshape(ref_dos.shape)))
        ref.backward()
        loss = tr.forward_backward(gd)
        if step == 0:
            e = abs(float(loss) - float(ref.detach())) / abs(float(ref.detach()))
            assert rmse(tr.last_outputs.cpu(), ref_dos.detach()) <= 1e-12 and e <= 1e-12, e
            fp = tr._fp
            unused = "GN_encoder.node_encoder." if prompt else "GN_encoder.node_encoder_prompt."
            worst = 0.0
            for k, v in pr.items():
                if not isinstance(v, torch.nn.Parameter):
                    continue
                if v.grad is None:
                    assert k not in fp.G and (k.startswith(unused) or ".node_mlp_1." in k), k
                    continue
                ek = _relmax(fp.G[k].cpu(), v.grad)
                worst = max(worst, ek)
                assert ek <= 1e-10, (k, ek)
            print(f"H={H} prompt={prompt}: loss error {e:.2e}, worst per-tensor gradient error {worst:.2e}")
        opt.step()
        tr.optimizer_step()
    print(f"H={H} prompt={prompt}: smallest |pre-activation| of the oracle over the steps {min(pre_min):.3e}")
    assert len(pre_min) == 3 and min(pre_min) >= 1e-9
    sd = model.state_dict()
    worst = 0.0
    for k, v in pr.items():
        if v.is_floating_point():
            d = float((sd[k].cpu() - v.detach()).abs().max())
            worst = max(worst, d)
            assert d <= 1e-9, (k, d)
    print(f"H={H} prompt={prompt}: largest parameter difference after 3 steps {worst:.2e}")
    assert float((sd["embeddings.weight"].cpu() - base.state_dict()["embeddings.weight"]).abs().max()) > 1e-4      # it trained


def _grads_close(fp, got, ref, tol, tag):
    worst = 0.0
    for n, o in zip(fp.names, fp.offsets):
        k = fp.P[n].numel()
        e = _relmax(got[o:o + k], ref[o:o + k])
        worst = max(worst, e)
        assert e <= tol, (tag, n, e)
    return worst


@pytest.mark.parametrize("H", [64, 136])
def test_factored_program_against_the_modules_own(H):
    """The same module, the same batch: model(batch), torch loss, loss.backward() (the unfactored program behind autograd)
    against the trainer's factored step on a deep copy - dos to 1e-12, the loss to 1e-12 relative, gradients to 1e-10."""
    from dostransformer_amd import synth
    base = _gn(H, seed=11)
    hand, fused = copy.deepcopy(base).to(DEV), copy.deepcopy(base).to(DEV)
    g = synth.phonon_batch(6, seed=31, dtype=torch.float64).to(DEV)
    dos = hand(g)
    ref = torch.sqrt(F.mse_loss(dos, g.phdos.reshape(dos.shape)))
    ref.backward()
    tr = _trainer(fused)
    loss = tr.forward_backward(g)
    assert rmse(tr.last_outputs, dos.detach()) <= 1e-12
    assert abs(float(loss) - float(ref.detach())) <= 1e-12 * abs(float(ref.detach()))
    hfp = hand.flat_params(g)
    assert tr._fp.names == hfp.names
    worst = _grads_close(tr._fp, tr._fp.grad, hfp.grad, 1e-10, "factored vs unfactored")
    print(f"H={H}: factored against unfactored, worst per-tensor gradient error {worst:.2e}")


# =====================================================================================================================
# 5. replay and padding
# =====================================================================================================================
ATOMS = [3, 7, 19, 12, 5, 2, 18, 4, 9, 6, 11]
SEL_A, SEL_A2, SEL_C, SEL_P = [0, 1, 2, 3], [7, 2, 9, 10], [4, 5, 6], [4, 5, 6, 7]      # N 41, 40, 25, 29


@pytest.fixture(scope="module")
def crystals():
    from dostransformer_amd import synth
    gen = torch.Generator().manual_seed(61)
    return [synth.phonon_crystal(gen, n) for n in ATOMS]


@pytest.fixture(scope="module")
def dataset(crystals):
    from dostransformer_amd.loader import DeviceDataset
    return DeviceDataset(crystals, DEV, dtype=torch.float64)


def _collate(crystals, sel):
    from dostransformer_amd.batch import collate
    return collate([crystals[i] for i in sel])


def _pad_to_bucket(g):
    from dostransformer_amd.batch import bucket_sizes, pad_batch
    m = g.meta
    return pad_batch(g, *bucket_sizes(m.num_nodes, m.num_edges, *BUCKET))


def _train(batches, seed=5, H=64, **kw):
    """Fresh module, one step per batch: -> (losses, flat gradients, flat parameters after each step, trainer)."""
    model = _gn(H, seed=seed).to(DEV)
    tr = _trainer(model, lr=1e-3, **kw)
    losses, grads, flats = [], [], []
    for b in batches:
        losses.append(tr.step(b).clone())
        grads.append(tr._fp.grad.clone())
        flats.append(tr._fp.flat.clone())
    torch.cuda.synchronize()
    return losses, grads, flats, tr


def test_replay_is_bitwise_the_eager_step(crystals):
    """Two shapes alternated over three steps: every loss and the flat parameters after every step torch.equal between
    replay = False and replay = True; two recordings and one replay; the recorded list holds the whole step."""
    gs = [_collate(crystals, s).to(DEV) for s in (SEL_A, SEL_C)]
    order = [gs[0], gs[1], gs[0]]
    el, _, ef, etr = _train(order)
    rl, _, rf, rtr = _train(order, replay=True)
    for i in range(3):
        assert torch.equal(el[i], rl[i]) and torch.equal(ef[i], rf[i]), i
    assert (rtr.slot_misses, rtr.slot_hits) == (2, 1) and (etr.slot_misses, etr.slot_hits) == (0, 0)
    assert all(len(s.prog) > 50 for s in rtr._slots.values())
    assert float((ef[0] - ef[2]).abs().max()) > 1e-4
    assert rtr.last_outputs.shape == (4, 51) and rtr.last_outputs.dtype == torch.float64


def test_a_padded_batch_gives_the_unpadded_numbers(crystals):
    """pad_batch to the bucket, and to a bucket with many ghosts: dos bitwise the unpadded batch's, the loss equal, gradients
    within 1e-10 per tensor (row sums grouped differently); without bucket a padded batch is refused before anything runs."""
    from dostransformer_amd._lib import DosxError
    from dostransformer_amd.batch import pad_batch
    g = _collate(crystals, SEL_A).to(DEV)
    ul, ug, _, utr = _train([g])
    udos = utr.last_outputs.clone()
    for padded in (_pad_to_bucket(g), pad_batch(g, 64, 1024)):
        pl, pg, _, ptr = _train([padded], bucket=BUCKET)
        assert torch.equal(ptr.last_outputs, udos) and torch.equal(pl[0], ul[0])
        worst = _grads_close(utr._fp, pg[0], ug[0], 1e-10, "padded vs unpadded")
        print(f"padded to {padded.meta.num_nodes} nodes: worst per-tensor gradient error {worst:.2e}")
    for tr in (utr, _trainer(_gn(64).to(DEV), replay=True)):
        before = tr.step_count
        with pytest.raises(DosxError, match="padded"):
            tr.step(_pad_to_bucket(g))
        assert tr.step_count == before


def _step_dataset_run(ds, sels, promote=0.0, replay=True, seed=5):
    tr = _trainer(_gn(64, seed=seed).to(DEV), lr=1e-3, replay=replay, bucket=BUCKET, promote=promote)
    losses, grads, flats = [], [], []
    for sel in sels:
        losses.append(tr.step_dataset(ds, sel, n_max=19).clone())
        grads.append(tr._fp.grad.clone())
        flats.append(tr._fp.flat.clone())
    torch.cuda.synchronize()
    return losses, grads, flats, tr


def test_step_dataset_is_bitwise_the_step_on_the_padded_collated_batch(dataset):
    """Three steps on selections of one bucket (48, 896): step_dataset (collate straight into the bucket + replay) against
    step(pad_batch(ds.collate(...), *bucket_sizes(...))) on a twin - losses and parameters torch.equal, one recording."""
    from dostransformer_amd.batch import bucket_sizes
    assert bucket_sizes(41, 820, *BUCKET) == bucket_sizes(40, 800, *BUCKET) == (48, 896)
    sels = [SEL_A, SEL_A2, SEL_A]
    dl, _, df, dtr = _step_dataset_run(dataset, sels)
    padded = [_pad_to_bucket(dataset.collate(sel, n_max=19)) for sel in sels]
    tl, _, tf, ttr = _train(padded, replay=True, bucket=BUCKET)
    for i in range(3):
        assert torch.equal(dl[i], tl[i]) and torch.equal(df[i], tf[i]), i
    assert (dtr.slot_misses, dtr.slot_hits, dtr.slot_promoted, len(dtr._slots)) == (1, 2, 0, 1)
    assert (ttr.slot_misses, ttr.slot_hits) == (1, 2)
    # without replay it is the step on the collated batch
    el, _, ef, _ = _step_dataset_run(dataset, [SEL_C], replay=False)
    cl, _, cf, _ = _train([dataset.collate(SEL_C, n_max=19)], bucket=BUCKET)
    assert torch.equal(el[0], cl[0]) and torch.equal(ef[0], cf[0])


def test_step_dataset_promotes_a_first_time_bucket_into_a_live_larger_one(dataset):
    """promote = 0.5: after a step in bucket (48, 896) the selection SEL_P - own bucket (32, 640), same B and n_max - runs in the
    live bucket: no second recording.  Losses to 1e-12, the second step's gradients to 1e-10 and the parameters to 1e-9 of the
    unpromoted run, which records the smaller bucket."""
    from dostransformer_amd.batch import bucket_sizes
    assert bucket_sizes(29, 580, *BUCKET) == (32, 640) and 48 <= 32 * 1.5 and 896 <= 640 * 1.5
    sels = [SEL_A, SEL_P]
    pl, pg, pf, ptr = _step_dataset_run(dataset, sels, promote=0.5)
    ul, ug, uf, utr = _step_dataset_run(dataset, sels)
    assert (ptr.slot_misses, ptr.slot_hits, ptr.slot_promoted, len(ptr._slots)) == (1, 1, 1, 1)
    assert (utr.slot_misses, utr.slot_hits, utr.slot_promoted, len(utr._slots)) == (2, 0, 0, 2)
    for a, b in zip(pl, ul):
        assert abs(float(a) - float(b)) <= 1e-12 * abs(float(b))
    _grads_close(utr._fp, pg[1], ug[1], 1e-10, "promoted vs own bucket")
    assert float((pf[1] - uf[1]).abs().max()) <= 1e-9


# =====================================================================================================================
# 6. checkpoint
# =====================================================================================================================
def test_checkpoint_resumes_bitwise(crystals, tmp_path):
    """Two steps, checkpoint.save, two more steps - against checkpoint.load into a fresh module and trainer and two steps:
    parameters and both moments torch.equal."""
    from dostransformer_amd import checkpoint
    gs = [_collate(crystals, s).to(DEV) for s in (SEL_A, SEL_C)]
    model = _gn(64, seed=5).to(DEV)
    tr = _trainer(model, lr=1e-3, replay=True)
    tr.step(gs[0])
    tr.step(gs[1])
    path = str(tmp_path / "gn64.pt")
    checkpoint.save(path, model, tr)
    tr.step(gs[0])
    tr.step(gs[1])
    model2 = _gn(64, seed=99).to(DEV)
    tr2 = _trainer(model2, replay=True)
    checkpoint.load(path, model2, tr2)
    assert tr2.step_count == 2 and tr2.lr == 1e-3 and tr2._m.dtype == torch.float64
    tr2.step(gs[0])
    tr2.step(gs[1])
    torch.cuda.synchronize()
    a, b = model.state_dict(), model2.state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert tr2.step_count == tr.step_count == 4 and tr._fp.names == tr2._fp.names
    assert torch.equal(tr._m, tr2._m) and torch.equal(tr._v, tr2._v)


# =====================================================================================================================
# 7. Predictor64 and the evaluators
# =====================================================================================================================
def test_predictor64_is_bitwise_the_factored_forward(crystals):
    from dostransformer_amd import functional64 as F64
    from dostransformer_amd.predict import Predictor64
    model = _gn(64, seed=5).to(DEV).eval()
    pred = Predictor64(model)
    assert pred.batch_independent
    for sel in (SEL_A, SEL_C, SEL_A2):                       # the third call replays the first bucket
        g = _collate(crystals, sel).to(DEV)
        out = pred(g)
        gp = _pad_to_bucket(g)
        with torch.no_grad():
            want, _ = F64.graphnetwork_phonon_fwd(model.flat_params(gp).P, model._cfg, gp, gp.meta, factored_head=True)
            plain = model(g)
        torch.cuda.synchronize()
        assert torch.is_tensor(out) and out.dtype == torch.float64 and torch.equal(out, want)
        assert rmse(out, plain) <= 1e-12
    assert (pred.slot_misses, pred.slot_hits) == (2, 1)


def test_the_evaluators_take_predictor64(crystals, dataset):
    """test_per_crystal(Predictor64(model), ds) in passes of 4 against the module at batch size 1, and test_phonon over batches
    of 4 through the predictor against the module: every crystal's prediction within 1e-12 RMS (delta), the metrics within the
    bounds that follow from it (tests/test_gpu_eval_per_crystal.py: delta, delta (r + r'), delta, 51 delta (r + r') / SS_tot,
    + 1e-12).  A batch's R2 is a ratio of sums over its crystals, so the largest per-crystal bound holds for it."""
    from dostransformer_amd import evaluate
    from dostransformer_amd.predict import Predictor64
    model = _gn(64, seed=5).to(DEV).eval()
    pred = Predictor64(model)
    res = evaluate.test_per_crystal(pred, dataset, batch_size=4)
    res = res._replace(per_crystal=res.per_crystal.clone(), preds=res.preds.clone(), y=res.y.clone())
    assert res.preds.dtype == torch.float64 and tuple(res.preds.shape) == (len(ATOMS), 51) and res.embeddings is None
    with torch.no_grad():
        want = torch.cat([model(_collate(crystals, [i]).to(DEV)) for i in range(len(ATOMS))])
    y = torch.stack([cr["phdos"].reshape(-1) for cr in crystals]).to(DEV)
    assert torch.equal(res.y, y)
    delta = torch.sqrt(((res.preds - want) ** 2).mean(1))
    print(f"largest per-crystal RMS difference to the module at batch size 1: {float(delta.max()):.3e}")
    assert float(delta.max()) <= 1e-12
    table = evaluate.per_crystal_metrics_host(want, y)
    sst = ((y - y.mean(1, keepdim=True)) ** 2).sum(1)
    rr = res.per_crystal[:, 0] + table[:, 0]
    bound = torch.stack([delta, delta * rr, delta, 51 * delta * rr / sst], 1) + 1e-12
    assert bool(((res.per_crystal - table).abs() <= bound).all()), ((res.per_crystal - table).abs() / bound).max(0)
    four = evaluate.test_phonon(model, dataset.batches(1))
    for k, (a, b) in enumerate(zip((res.rmse, res.mse, res.mae, res.r2), four)):
        assert abs(a - b) <= float(bound.mean(0)[k]), (k, a, b)
    got = evaluate.test_phonon(pred, dataset.batches(4))
    ref = evaluate.test_phonon(model, dataset.batches(4))
    for k, (a, b) in enumerate(zip(got, ref)):
        assert abs(a - b) <= float(bound.max(0).values[k]), (k, a, b)
