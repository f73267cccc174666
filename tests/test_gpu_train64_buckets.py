"""Shape buckets of the float64 trainer on a real MI355X: the float64 program on ghost-padded batches (forward bitwise, gradients
to rounding), train64.Trainer64(bucket=...) against the unpadded eager trainer and against the float64 oracle, replay against
eager on the same padded geometry (bitwise), the float64 padded collate kernel (dosx_collate_padded_f64) against
pad_batch(ds.collate(...)), Trainer64.step_dataset and predict.Predictor64.  Bounds: the project's float64 bars
(tests/test_gpu_train64.py): losses 1e-12 relative, gradients 1e-10 relative per tensor, parameters after AdamW steps 1e-9."""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 12345.0
L_, T_, H_, S_ = 2, 2, 32, 51
ATOMS_A = [3, 7, 19, 12]           # N 41, E 820
ATOMS_A2 = [4, 19, 6, 11]          # N 40, E 800: the same bucket as A
ATOMS_C = [5, 2, 18]               # another bucket
BUCKET = (8, 128)


def _relmax(got, ref):
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-300))


def _crystals(n_atoms, seed):
    from dostransformer_amd import synth
    gen = torch.Generator().manual_seed(seed)
    return [synth.phonon_crystal(gen, n) for n in n_atoms]


def _collate(cs):
    from dostransformer_amd.batch import collate
    return collate(cs)


def _module(attn_drop=0.0, seed=41):
    from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
    torch.manual_seed(seed)
    return DOSTransformer_phonon(L_, T_, 118, 4, H_, "cpu", attn_drop).double()


def _switch(module, pck=True):
    return module.set_program_dtype(torch.float64).set_per_crystal_keys(pck).to(DEV)


def _per_tensor(fp, got, ref, tol, tag):
    worst = 0.0
    for n, o in zip(fp.names, fp.offsets):
        k = fp.P[n].numel()
        e = _relmax(got[o:o + k], ref[o:o + k])
        worst = max(worst, e)
        assert e <= tol, (tag, n, e)
    return worst


def _pad_to_bucket(g):
    from dostransformer_amd.batch import bucket_sizes, pad_batch
    m = g.meta
    return pad_batch(g, *bucket_sizes(m.num_nodes, m.num_edges, *BUCKET))


@pytest.fixture(scope="module")
def crystals():
    """The 11 crystals of A (0-3), A' (4-7) and C (8-10)."""
    return _crystals(ATOMS_A, 51) + _crystals(ATOMS_A2, 53) + _crystals(ATOMS_C, 52)


@pytest.fixture(scope="module")
def batches(crystals):
    """(A, A', C) on the host; A and A' share the bucket (48, 896, B 4, n_max 19), C has its own."""
    from dostransformer_amd.batch import bucket_sizes
    a, a2, c = _collate(crystals[:4]), _collate(crystals[4:8]), _collate(crystals[8:])
    shapes = [(g.meta.num_nodes, g.meta.num_edges, g.meta.num_graphs, g.meta.n_max) for g in (a, a2, c)]
    assert shapes == [(41, 820, 4, 19), (40, 800, 4, 19), (25, 500, 3, 18)]
    assert bucket_sizes(41, 820, *BUCKET) == bucket_sizes(40, 800, *BUCKET) == (48, 896)
    assert bucket_sizes(25, 500, *BUCKET) == (32, 512)
    return a, a2, c


# =====================================================================================================================
# 1. the float64 program on a ghost-padded batch
# =====================================================================================================================
def _fwd_bwd(model, g, ddos):
    """-> (dos [2B, S], x_L, flat gradient) of the float64 program on batch g with output gradient ddos."""
    from dostransformer_amd import functional64 as F64
    from dostransformer_amd.batch import graph_meta
    fp = model.flat_params(g)
    m = graph_meta(g, fp.flat.device)
    with torch.no_grad():
        dos, xL, ctx = F64.dostransformer_phonon_fwd(fp.P, model._cfg, g, m, drop=None, per_crystal_keys=model.per_crystal_keys)
        fp.grad.zero_()
        F64.dostransformer_phonon_bwd(fp.P, fp.G, model._cfg, m, ctx, ddos, None)
    torch.cuda.synchronize()
    return dos.clone(), xL.clone(), fp.grad.clone()


@pytest.fixture(scope="module")
def unpadded_reference(batches):
    """pck -> (model, batch A on the device, ddos, dos, x_L, flat gradient) of the UNPADDED batch; computed once."""
    out = {}
    for pck in (True, False):
        model = _switch(_module(), pck).eval()
        g = batches[0].clone().to(DEV)
        ddos = torch.randn(2 * 4, S_, generator=torch.Generator().manual_seed(3), dtype=torch.float64).to(DEV)
        out[pck] = (model, g, ddos) + _fwd_bwd(model, g, ddos)
    return out


@pytest.mark.parametrize("pad", [(48, 896), (64, 1024)], ids=["bucket", "many_ghosts"])
@pytest.mark.parametrize("pck", [True, False], ids=["per_crystal", "padded_keys"])
def test_ghost_padding_is_exact_forward_and_rounding_backward(unpadded_reference, pck, pad):
    """pad_batch(A, 48, 896) (7 ghost nodes, 76 ghost edges) and (64, 1024) (23 ghost nodes, 204 ghost edges - no multiple of a
    tile; the weight gradients over the edges then take two row splits instead of one): dos and x_L[:41] torch.equal to the
    unpadded batch; the flat gradient finite everywhere and within 1e-10 relative per tensor of the unpadded one."""
    from dostransformer_amd.batch import pad_batch
    model, g, ddos, dos, xL, grad = unpadded_reference[pck]
    gp = pad_batch(g, *pad)
    assert gp.real_nodes == 41 and gp.meta.num_nodes == pad[0] and gp.meta.num_edges == pad[1]
    dos_p, xL_p, grad_p = _fwd_bwd(model, gp, ddos)
    assert xL_p.shape == (pad[0], H_) and bool(torch.isfinite(xL_p).all())
    assert torch.equal(dos_p, dos), _relmax(dos_p, dos)
    assert torch.equal(xL_p[:41], xL), _relmax(xL_p[:41], xL)
    assert bool(torch.isfinite(grad_p).all())
    worst = _per_tensor(model.flat_params(), grad_p, grad, 1e-10, "grad")
    print(f"pck={pck} pad={pad}: worst per-tensor gradient difference to the unpadded batch {worst:.2e}")
    assert float(grad.abs().max()) > 1e-6


# =====================================================================================================================
# 2 - 4. Trainer64(bucket=...)
# =====================================================================================================================
def _train(model, batches_dev, seed=97, **kw):
    """One step per batch of a fresh Trainer64(model, lr=1e-3, **kw): -> (losses, step-1 gradient, flat clones, trainer)."""
    from dostransformer_amd.train64 import Trainer64
    torch.manual_seed(seed)                     # the dropout seed is drawn from torch's RNG at the first step
    tr = Trainer64(model, lr=1e-3, **kw)
    losses, flats, grad1 = [], [], None
    for i, g in enumerate(batches_dev):
        losses.append(tr.step(g).clone())
        if i == 0:
            grad1 = tr._fp.grad.clone()
        flats.append(tr._fp.flat.clone())
    return losses, grad1, flats, tr


def _close(la, ga, fa, lb, gb, fb, fp, tag):
    """The float64 bars between two runs: losses 1e-12 relative, step-1 gradients 1e-10 per tensor, final parameters 1e-9."""
    for i, (x, y) in enumerate(zip(la, lb)):
        e = abs(float(x) - float(y)) / abs(float(y))
        assert e <= 1e-12, (tag, "loss", i, e)
    worst = _per_tensor(fp, ga, gb, 1e-10, tag + " grad")
    d = float((fa[-1] - fb[-1]).abs().max())
    print(f"{tag}: worst per-tensor step-1 gradient difference {worst:.2e}, largest parameter difference {d:.2e}")
    assert d <= 1e-9, (tag, "parameters", d)


def test_bucketed_replay_trainer_against_the_unpadded_eager_trainer(batches):
    """Two deep copies of one dropout-0.1 module, same torch seed, three steps on A, A', A: Trainer64(replay=True, bucket=(8, 128))
    against Trainer64().  One recording, two replays, one slot; last_outputs[1] is cut to the real nodes."""
    base = _module(0.1)
    a, a2, _ = batches
    gs = [b.clone().to(DEV) for b in (a, a2, a)]
    el, eg, ef, etr = _train(_switch(copy.deepcopy(base)).train(), gs)
    bl, bg, bf, btr = _train(_switch(copy.deepcopy(base)).train(), gs, replay=True, bucket=BUCKET)
    _close(bl, bg, bf, el, eg, ef, etr._fp, "bucketed replay vs unpadded eager")
    assert (btr.slot_misses, btr.slot_hits, len(btr._slots)) == (1, 2, 1)
    assert next(iter(btr._slots))[:4] == (48, 896, 4, 19)
    assert btr.last_outputs[1].shape == (41, H_) and etr.last_outputs[1].shape == (41, H_)
    assert float((ef[0] - ef[2]).abs().max()) > 1e-4                                     # it trained


def test_bucketed_replay_is_bitwise_eager_on_the_same_padded_geometry(batches):
    """Four steps alternating A and C, dropout 0.1: Trainer64(replay=True, bucket=...) fed the unpadded batches (padded on the
    fly) against Trainer64(replay=False, bucket=...) fed pad_batch(...) of them - every loss and the flat parameters after
    every step torch.equal.  Two recordings, two replays."""
    base = _module(0.1)
    a, _, c = batches
    plain = [b.clone().to(DEV) for b in (a, c, a, c)]
    padded = [_pad_to_bucket(b) for b in plain]
    rl, _, rf, rtr = _train(_switch(copy.deepcopy(base)).train(), plain, replay=True, bucket=BUCKET)
    el, _, ef, etr = _train(_switch(copy.deepcopy(base)).train(), padded, replay=False, bucket=BUCKET)
    for i in range(4):
        assert torch.equal(rl[i], el[i]) and torch.equal(rf[i], ef[i]), i
    assert (rtr.slot_misses, rtr.slot_hits, len(rtr._slots)) == (2, 2, 2) and (etr.slot_misses, etr.slot_hits) == (0, 0)
    assert etr.last_outputs[1].shape == (25, H_) and rtr.last_outputs[1].shape == (25, H_)
    assert all(len(s.prog) > 50 for s in rtr._slots.values())
    # an already padded batch is taken as it is by the replay trainer too
    loss = rtr.step(padded[0])
    assert (rtr.slot_misses, rtr.slot_hits) == (2, 3) and bool(torch.isfinite(loss))


def _soft64_mha(q, k, v, drop_mask=None):
    dim = q.shape[2]
    w = torch.bmm(q.transpose(0, 1), k.transpose(0, 1).transpose(1, 2)) * (dim ** -0.5)
    w = F.softmax(w, dim=-1)
    if drop_mask is not None:
        w = w * drop_mask.to(w.dtype)
    return torch.bmm(w, v.transpose(0, 1)).transpose(0, 1)


def test_bucketed_replay_trainer_against_the_oracle_crystal_by_crystal(monkeypatch, crystals):
    """fp64 softmax on both sides, per-crystal keys: three steps of Trainer64(replay=True, bucket=(8, 128)) on A against the
    float64 oracle run on every crystal alone, the batch loss over the concatenated DOS vectors and torch.optim.AdamW on the
    CPU.  Step-1 loss within 1e-12, parameters after three steps within 1e-9."""
    from oracle import dos_oracle as O
    from dostransformer_amd import functional64 as F64
    from dostransformer_amd.train64 import Trainer64
    monkeypatch.setattr(O, "multihead_attention", _soft64_mha)
    monkeypatch.setattr(F64, "SOFTMAX64", True)
    base = _module()
    lr, beta = 1e-3, 1.0
    cs = crystals[:4]
    singles = [_collate([c]) for c in cs]
    phdos = _collate(cs).phdos
    pr = {k: (torch.nn.Parameter(v.detach().clone()) if v.is_floating_point() else v.clone()) for k, v in base.state_dict().items()}
    opt = torch.optim.AdamW([v for v in pr.values() if isinstance(v, torch.nn.Parameter)], lr=lr, weight_decay=1e-2)
    model = _switch(copy.deepcopy(base))
    tr = Trainer64(model, lr=lr, beta=beta, replay=True, bucket=BUCKET)
    gd = _collate(cs).to(DEV)
    for step in range(3):
        opt.zero_grad()
        outs = [O.dostransformer_phonon_forward(pr, g1, L_, T_) for g1 in singles]
        ref = O.loss_phonon(torch.cat([o[0] for o in outs]), torch.cat([o[2] for o in outs]), phdos, beta)
        ref.backward()
        opt.step()
        loss = tr.step(gd)
        ref = float(ref.detach())
        print(f"step {step}: loss {float(loss):.15g}, oracle {ref:.15g}")
        if step == 0:
            assert abs(float(loss) - ref) <= 1e-12 * abs(ref), (float(loss), ref)
    assert (tr.slot_misses, tr.slot_hits) == (1, 2)
    sd = model.state_dict()
    worst = 0.0
    for k, v in pr.items():
        if v.is_floating_point():
            d = float((sd[k].cpu() - v.detach()).abs().max())
            worst = max(worst, d)
            assert d <= 1e-9, (k, d)
    print(f"largest parameter difference after 3 steps: {worst:.2e}")


# =====================================================================================================================
# 5. the float64 padded collate kernel
# =====================================================================================================================
@pytest.fixture(scope="module")
def dataset(crystals):
    from dostransformer_amd.loader import DeviceDataset
    return DeviceDataset(crystals, DEV, dtype=torch.float64)


def _guarded(shape, front):
    """A float64 buffer of ``shape`` inside a sentinel-filled one, ``front`` doubles in: -> (view, whole buffer)."""
    count = 1
    for s in shape:
        count *= s
    whole = torch.full((count + front + 5,), SENT, dtype=torch.float64, device=DEV)
    return whole[front:front + count].view(*shape), whole


@pytest.mark.parametrize("front", [4, 3], ids=["aligned16", "aligned8"])
def test_collate_padded_f64_matches_pad_batch(dataset, front):
    """collate_into on a float64 bucket (48, 896, B 4, n_max 19) whose feature buffers sit between sentinels - 16-byte aligned
    (rows of x move as 16-byte vectors) and 8-byte aligned only (element by element): every field the program reads
    torch.equal to pad_batch(ds.collate(sel), 48, 896), for [0, 1, 2, 3] and then [4, 5, 6, 7] INTO THE SAME BUFFERS (one real
    node fewer: nothing of the first batch is left, the ghost rows are zeros); the sentinels are untouched; the dataset made
    no fp32 copy."""
    import numpy as np
    from dostransformer_amd.batch import pad_batch
    from dostransformer_amd.slots import Slot
    ds = dataset
    slot = Slot.empty("phonon", torch.device(DEV), torch.float64, 4, 48, 896, 19, 118, 3, S_)
    guards = {}
    for k in ("x", "edge_vec", "phdos"):
        view, whole = _guarded(tuple(slot.g[k].shape), front)
        assert view.data_ptr() % 16 == (0 if front % 2 == 0 else 8) and view.is_contiguous()
        slot.g[k] = view
        guards[k] = (whole, view.numel())
    for sel in ([0, 1, 2, 3], [4, 5, 6, 7]):
        ds.collate_into(slot.g, np.asarray(sel, np.int64), slot.collate_scratch())
        torch.cuda.synchronize()
        ref = pad_batch(ds.collate(sel), 48, 896)
        n_real = ref.real_nodes
        for k in ("x", "edge_vec", "phdos"):
            assert slot.g[k].dtype == torch.float64 and torch.equal(slot.g[k], ref[k]), (sel, k)
            whole, count = guards[k]
            assert bool((whole[:front] == SENT).all()) and bool((whole[front + count:] == SENT).all()), (sel, k, "sentinel")
        assert torch.equal(slot.g.system, ref.system.to(torch.int32)), sel
        for k in ("src", "dst", "rowptr_dst", "perm_src", "rowptr_src", "graph_ptr", "node_graph", "dense_row", "inv_deg"):
            assert torch.equal(getattr(slot.g.meta, k), getattr(ref.meta, k)), (sel, k)
        assert bool((slot.g.x[n_real:] == 0).all()) and bool((slot.g.edge_vec[20 * n_real:] == 0).all())
        assert float(slot.g.x[:n_real].abs().sum(1).min()) > 0          # (every real atom row carries its mass)
    assert getattr(ds, "_tables32", None) is None
    t = ds._f64_tables()
    assert t["x"] is ds._x and t["edge"] is ds._edge["edge_vec"] and t["target"] is ds._graph["phdos"]


# =====================================================================================================================
# 6. Trainer64.step_dataset
# =====================================================================================================================
def _step_dataset_run(base, ds, sels, promote=0.0, seed=97):
    from dostransformer_amd.train64 import Trainer64
    torch.manual_seed(seed)
    tr = Trainer64(_switch(copy.deepcopy(base)).train(), lr=1e-3, replay=True, bucket=BUCKET, promote=promote)
    losses, flats, grads = [], [], []
    for sel in sels:
        losses.append(tr.step_dataset(ds, sel, n_max=19).clone())
        grads.append(tr._fp.grad.clone())
        flats.append(tr._fp.flat.clone())
    return losses, grads, flats, tr


def test_step_dataset_is_bitwise_the_step_on_the_padded_collated_batch(dataset):
    """Four steps on fixed selections with n_max = 19, dropout 0.1: step_dataset (collate straight into the bucket + replay)
    torch.equal in every loss and in the flat parameters after every step to step(pad_batch(ds.collate(sel, n_max=19), ...)) on
    a twin trainer.  One recording, three replays; without replay step_dataset is the step on the collated batch."""
    from dostransformer_amd.train64 import Trainer64
    base = _module(0.1)
    sels = [[0, 1, 2, 3], [4, 5, 6, 7], [3, 2, 1, 0], [4, 5, 6, 7]]
    dl, _, df, dtr = _step_dataset_run(base, dataset, sels)
    padded = [_pad_to_bucket(dataset.collate(sel, n_max=19)) for sel in sels]
    tl, _, tf, ttr = _train(_switch(copy.deepcopy(base)).train(), padded, replay=True, bucket=BUCKET)
    for i in range(4):
        assert torch.equal(dl[i], tl[i]) and torch.equal(df[i], tf[i]), i
    assert (dtr.slot_misses, dtr.slot_hits, dtr.slot_promoted, len(dtr._slots)) == (1, 3, 0, 1)
    assert dtr.last_outputs[1].shape == (40, H_) and dtr.step_count == 4
    # a larger n_max serves the selection [8, 9, 10] (largest crystal 18 atoms); eager: the step on the collated batch
    e1 = Trainer64(_switch(copy.deepcopy(base)).train(), lr=1e-3, bucket=BUCKET)
    e2 = Trainer64(_switch(copy.deepcopy(base)).train(), lr=1e-3)
    torch.manual_seed(97)                       # (each trainer's first step draws its module's dropout seed)
    l1 = e1.step_dataset(dataset, [8, 9, 10], n_max=19)
    torch.manual_seed(97)
    l2 = e2.step(dataset.collate([8, 9, 10], n_max=19))
    assert torch.equal(l1, l2) and torch.equal(e1._fp.flat, e2._fp.flat)


def test_step_dataset_promotes_a_first_time_bucket_into_a_live_larger_one(dataset):
    """promote = 0.5: after a step on [0, 1, 2, 3] (bucket 48, 896) the selection [8, 9, 10, 4] - own bucket (32, 640), B 4,
    n_max 19 - runs in the live bucket: no second recording, one slot.  Losses, the second step's gradients and the parameters
    are within the float64 bars of the unpromoted run, which records the smaller bucket."""
    from dostransformer_amd.batch import bucket_sizes
    base = _module(0.1)
    sels = [[0, 1, 2, 3], [8, 9, 10, 4]]
    N2 = 5 + 2 + 18 + 4
    assert bucket_sizes(N2, 20 * N2, *BUCKET) == (32, 640) and 48 <= 32 * 1.5 and 896 <= 640 * 1.5
    pl, pg, pf, ptr = _step_dataset_run(base, dataset, sels, promote=0.5)
    ul, ug, uf, utr = _step_dataset_run(base, dataset, sels)
    assert (ptr.slot_misses, ptr.slot_hits, ptr.slot_promoted, len(ptr._slots)) == (1, 1, 1, 1)
    assert (utr.slot_misses, utr.slot_hits, utr.slot_promoted, len(utr._slots)) == (2, 0, 0, 2)
    assert ptr.last_outputs[1].shape == (N2, H_) and utr.last_outputs[1].shape == (N2, H_)
    assert torch.equal(pl[0], ul[0]) and torch.equal(pf[0], uf[0])                     # (the first step is the same step)
    _close(pl, pg[1], pf, ul, ug[1], uf, utr._fp, "promoted vs own bucket")
    # the second visit of that bucket records it (train.Trainer._lookup's rule)
    ptr.step_dataset(dataset, sels[1], n_max=19)
    assert (ptr.slot_misses, ptr.slot_promoted, len(ptr._slots)) == (2, 1, 2)


# =====================================================================================================================
# 7. predict.Predictor64
# =====================================================================================================================
def test_predictor64_replays_the_forward_bitwise_and_serves_the_evaluation_loop(batches):
    """Eval mode, A then A' then A: outputs torch.equal to model(batch) under no_grad, in float64, x cut to the real nodes; one
    recording and two replays.  evaluate.test_phonon through the predictor returns exactly what it returns through the module.
    A training-mode module with dropout is refused."""
    from dostransformer_amd import evaluate
    from dostransformer_amd.predict import Predictor64
    model = _switch(_module(0.1)).eval()
    pred = Predictor64(model, bucket=BUCKET)
    a, a2, c = (b.clone().to(DEV) for b in batches)
    for g, n in ((a, 41), (a2, 40), (a, 41)):
        with torch.no_grad():
            ref = [t.clone() for t in model(g)]
        out = pred(g)
        assert all(t.dtype == torch.float64 for t in out) and out[1].shape == (n, H_)
        for x, y in zip(out, ref):
            assert torch.equal(x, y)
    assert (pred.slot_misses, pred.slot_hits, len(pred._slots)) == (1, 2, 1)
    want = evaluate.test_phonon(model, [a, a2, c])
    got = evaluate.test_phonon(Predictor64(model), [a, a2, c])
    assert got == want and all(x == x for x in got)
    model.train()
    with pytest.raises(RuntimeError, match="eval"):
        pred(a)
