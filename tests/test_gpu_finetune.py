"""Fine-tuning on a real MI355X: frozen parameters (``requires_grad``) are honoured by every driver - bitwise untouched, with zero
moments - and the parameters that train get exactly the step an all-trainable twin composes for them: the pruned backward
programs (functional.wgrad_needed / trunk_cut / first_encoder_cut) remove launches and weight-gradient jobs, never arithmetic.

The twin: an all-trainable model of the same class loaded with the current parameters runs the step in the SAME mode with
lr = weight_decay = 0 (its parameters stay put, its flat gradient is the step's gradient); the test then applies ops.adamw /
ops.adamw64 tensor by tensor to the trainable ones only."""
import copy

import numpy as np
import pytest
import torch

from tests.gpu_util import _FakeDist

pytestmark = pytest.mark.gpu
DEV = "cuda"
TRUNK = ("GN_encoder", "stacked_processor", "GN_decoder")
LR, WD, BETAS, EPS = 1e-3, 1e-2, (0.9, 0.999), 1e-8


def _make(kind, H=64, T=2):
    if kind == "phonon":
        from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
        return DOSTransformer_phonon(2, T, 118, 4, H, DEV, 0.0).to(DEV)
    from dostransformer_amd.embedder_eDOS.DOSTransformer import DOSTransformer
    return DOSTransformer(2, T, 200, 41, 2, H, DEV, 0.0).to(DEV)


def _batch(kind, seed):
    from dostransformer_amd import synth
    if kind == "phonon":
        return synth.phonon_batch(4, seed=seed, dtype=torch.float32)
    return synth.edos_batch(4, seed=seed, dtype=torch.float32)


def _padded(kind, seeds):
    from dostransformer_amd.batch import bucket_sizes, pad_batch
    out = []
    for s in seeds:
        b = _batch(kind, s).to(DEV)
        out.append(pad_batch(b, *bucket_sizes(b.meta.num_nodes, b.meta.num_edges)))
    return out


def _recipe(model, which):
    if which == "A":
        return model.freeze(*TRUNK)
    if which == "B":
        # (the prompt table under its own name: the Electron-DOS reference spells it `promt_token`)
        return model.train_only(model._cfg.prompt_key.rsplit(".", 1)[0], "fc_prompt")
    if which == "C":
        for n, p in model.named_parameters():
            if n == "transformer.layers.0.fc1.weight" or n == "embeddings.weight" or n.startswith("stacked_processor.1"):
                p.requires_grad_(False)
        model.update_trainable()
        return model
    if which == "D":
        return model.train_only("GN_encoder.node_encoder")
    raise ValueError(which)


def _assert_fused(model, g):
    """the cross attentions' backward runs inside dosx_ffn_bwd at this shape: the fused path is the one under test"""
    from dostransformer_amd import functional as Fn
    cfg, m = model._cfg, g.meta
    assert cfg.H <= 256
    assert Fn.attention_bwd_in_ffn(cfg.S, m.num_graphs, m.n_max, cfg.H, False)              # transformer
    assert Fn.attention_bwd_in_ffn(cfg.S, 2 * m.num_graphs, m.n_max, cfg.H, False)          # transformer_source


def _twin_of(model, make):
    twin = make()
    twin.load_state_dict(copy.deepcopy(model.state_dict()))
    return twin


def _views(fp, buf):
    return {n: buf[o:o + fp.P[n].numel()] for n, o in zip(fp.names, fp.offsets)}


def _adamw_by_tensor(P, G, M, V, names, step, f64=False):
    """ops.adamw / ops.adamw64 on clones, one tensor at a time -> {name: (p, m, v)}"""
    from dostransformer_amd import ops
    out = {}
    for n in names:
        # each tensor in a buffer of its own, zero-padded to the 64 elements every parameter is aligned to in the flat buffer:
        # the kernels' vector body then handles every element, as it does there (their scalar tail, which a 1-element tensor
        # alone would take, is compiled separately and need not round alike)
        k = P[n].numel()
        kp = (k + 63) // 64 * 64
        p, g, m, v = (torch.zeros(kp, dtype=P[n].dtype, device=DEV) for _ in range(4))
        for dst, src in ((p, P), (g, G), (m, M), (v, V)):
            dst[:k].copy_(src[n].detach().reshape(-1))
        if f64:
            ops.adamw64(p, g, m, v, kp, LR, BETAS[0], BETAS[1], EPS, WD, step)
        else:
            ops.adamw(p, g, m, v, kp, LR, BETAS[0], BETAS[1], EPS, WD, step, 1.0)
        out[n] = (p[:k], m[:k], v[:k])
    return out


def _check_step(tr, twin_tr, do_step, step, init, f64=False):
    """One step of ``tr`` (partly frozen) against what the all-trainable twin + per-tensor AdamW compose; checks (a) and (b)."""
    model, twin = tr.model, twin_tr.model
    twin.load_state_dict(copy.deepcopy(model.state_dict()))
    do_step(twin_tr)                                                  # lr = wd = 0: leaves the step's gradient in its flat buffer
    tfp = twin.flat_params() if twin_tr._fp is None else twin_tr._fp
    assert not tfp.frozen and tfp.n_train == tfp.total
    fp0 = tr._fp
    if fp0 is None:
        P0, M0, V0 = {n: p.detach().clone() for n, p in model.named_parameters()}, None, None
    else:
        P0 = {n: t.clone() for n, t in fp0.P.items()}
        M0, V0 = ({n: t.clone() for n, t in _views(fp0, b).items()} for b in (tr._m, tr._v))
    loss = do_step(tr)
    fp = tr._fp
    assert fp.frozen and 0 < fp.n_train < fp.total
    if M0 is None:
        M0 = {n: torch.zeros_like(fp.P[n]).reshape(-1) for n in fp.names}
        V0 = {n: torch.zeros_like(fp.P[n]).reshape(-1) for n in fp.names}
    train = fp.trainable_names()
    want = _adamw_by_tensor(P0, tfp.G, M0, V0, train, step, f64)
    torch.cuda.synchronize()
    Mv, Vv = _views(fp, tr._m), _views(fp, tr._v)
    for n in train:                                                  # (b) bitwise the independently composed step
        p, m, v = want[n]
        assert torch.equal(fp.P[n].reshape(-1), p), ("param", n, step)
        assert torch.equal(Mv[n], m) and torch.equal(Vv[n], v), ("moments", n, step)
        assert not torch.equal(p, P0[n].reshape(-1)), ("did not move", n)
    for n in fp.frozen:                                              # (a) frozen: bitwise the initial values, zero moments
        assert torch.equal(fp.P[n], init[n]), ("frozen parameter moved", n, step)
        assert not bool(Mv[n].any()) and not bool(Vv[n].any()), ("frozen moments", n, step)
    assert bool(torch.isfinite(loss))
    return loss


def _linears(fp, keys):
    """weight names among ``keys`` (the Linears a program reached) whose weight or bias trains"""
    return {k for k in set(keys) if k not in fp.frozen or (k[:-6] + "bias" in fp.P and k[:-6] + "bias" not in fp.frozen)}


def _check_stats(which, tr, twin_tr, T):
    """(c): what the pruned program consists of, against the all-trainable twin's program in the same mode"""
    st, full = tr.program_stats(), twin_tr.program_stats()
    fp = tr._fp
    assert full["wgrad_jobs"] == len(full["wgrad_keys"]) > 0 and st["wgrad_jobs"] == len(st["wgrad_keys"])
    assert st["launches"] == sum(e.startswith("dosx_") for e in st["entries"]) > 0
    # one job list entry per deferred job: exactly the twin's jobs whose Linear has a trainable weight or bias, in its order
    reached = _linears(fp, full["wgrad_keys"])
    if which in ("C", "D"):                                          # (nothing cut: every Linear is still reached)
        assert st["wgrad_keys"] == [k for k in full["wgrad_keys"] if k in reached]
    else:                                                            # (behind the cut nothing is reached)
        assert sorted(st["wgrad_keys"]) == sorted(k for k in full["wgrad_keys"] if k in reached)
    assert len(set(st["wgrad_keys"])) == len(reached) and st["wgrad_jobs"] < full["wgrad_jobs"]
    cnt = lambda s, name: s["entries"].count(name)
    if which in ("A", "B"):
        assert cnt(st, "dosx_dense_normalize_pool_bwd") == 0 and cnt(st, "dosx_dense_normalize_bwd") == 0
        assert st["launches"] < full["launches"]
        for name in ("dosx_mlp_ln_bwd", "dosx_edge_mlp_bwd", "dosx_node_grad", "dosx_gather_bwd"):     # no trunk backward
            assert cnt(st, name) == 0, name
    if which == "A":
        assert cnt(st, "dosx_ffn_bwd") == cnt(full, "dosx_ffn_bwd") == 3 * T
    if which == "B":                                                 # ... and no backward of the `transformer` encoder
        assert cnt(full, "dosx_ffn_bwd") == 3 * T and cnt(st, "dosx_ffn_bwd") == 2 * T
        assert cnt(st, "dosx_embed_rows_bwd") == 1
    if which == "D":
        # all-trainable's launches except weight-gradient launches: the flush launches that lost all their jobs, the prompt
        # table's row scatter with the product that makes its rows, and the energy table's row reduction
        from collections import Counter
        diff = Counter(e for e in full["entries"] if e.startswith("dosx_"))
        diff.subtract(Counter(e for e in st["entries"] if e.startswith("dosx_")))
        diff = {k: v for k, v in diff.items() if v}
        assert diff.pop("dosx_embed_rows_bwd", 0) == 1 and diff.pop("dosx_gemm", 0) == 1 and diff.pop("dosx_reduce_rows", 0) == 1
        assert diff.pop("dosx_grad_flush", 0) >= 0 and not diff, diff


CASES = [(k, r, m) for k in ("phonon", "edos") for r in "ABCD" for m in ("eager", "replay")] + \
        [(k, "A", m) for k in ("phonon", "edos") for m in ("graph", "dataset")]


@pytest.mark.parametrize("kind,which,mode", CASES)
def test_frozen_parameters_are_honoured_and_the_rest_steps_as_composed(kind, which, mode):
    from dostransformer_amd import synth
    from dostransformer_amd.loader import DeviceDataset
    from dostransformer_amd.train import Trainer
    torch.manual_seed(7)
    T = 2
    model = _recipe(_make(kind, T=T), which)
    twin = _twin_of(model, lambda: _make(kind, T=T))
    init = {n: p.detach().clone() for n, p in model.named_parameters()}
    kw = dict(replay=mode in ("replay", "dataset"), graph=mode == "graph")
    tr = Trainer(model, lr=LR, weight_decay=WD, betas=BETAS, eps=EPS, **kw)
    twin_tr = Trainer(twin, lr=0.0, weight_decay=0.0, **kw)
    if mode == "dataset":
        cs = (synth.phonon_crystals if kind == "phonon" else synth.edos_crystals)(8, seed=43, dtype=torch.float32)
        ds = DeviceDataset(cs, DEV)
        nmax = max(int(x["x"].shape[0]) for x in cs)
        sels = [np.array(s) for s in ([0, 1, 2, 3], [4, 5, 6, 7], [0, 1, 2, 3])]
        _assert_fused(model, ds.collate(sels[0], n_max=nmax))
        steps = [lambda t, s=s: t.step_dataset(ds, s, n_max=nmax) for s in sels]
    else:
        b = _padded(kind, (21, 22))
        _assert_fused(model, b[0])
        steps = [lambda t, g=g: t.step(g) for g in (b[0], b[1], b[0])]          # (the third step replays a recorded slot)
    for i, do in enumerate(steps):
        _check_step(tr, twin_tr, do, i + 1, init)
        _check_stats(which, tr, twin_tr, T)
    tr.check()
    if mode in ("replay", "dataset", "graph"):
        assert tr.slot_hits >= 1                                      # (the third step replayed a recorded / captured slot)


def _oracle_steps(kind, model, frozen, g32, L, T, steps, lr):
    """float64 oracle forward + loss + oracle.adamw_step with the frozen names' gradients set to None"""
    from oracle import dos_oracle as O
    g64 = g32.to("cpu", dtype=torch.float64)
    params = {k: (v.detach().cpu().clone().double() if v.is_floating_point() else v.cpu().clone()) for k, v in model.state_dict().items()}
    state, out = {}, []
    for _ in range(steps):
        leaves = {k: v.detach().requires_grad_(True) for k, v in params.items() if v.is_floating_point()}
        if kind == "phonon":
            dg, _, ds = O.dostransformer_phonon_forward(leaves, g64, L, T)
            loss = O.loss_phonon(dg, ds, g64.phdos, 1.0)
        else:
            dg, _, ds = O.dostransformer_forward(leaves, g64, L, T)
            loss = O.loss_edos(dg, ds, g64.y_ft, 1.0)
        names = list(leaves)
        gr = dict(zip(names, torch.autograd.grad(loss, [leaves[k] for k in names], allow_unused=True)))
        for n in frozen:
            gr[n] = None
        O.adamw_step(params, gr, state, lr)
        out.append((float(loss.detach()), {k: v.clone() for k, v in params.items()}))
    return out


@pytest.mark.parametrize("kind,which", [("phonon", "A"), ("phonon", "B"), ("edos", "A")])
def test_fine_tuning_follows_the_float64_oracle(kind, which):
    """Three steps against the float64 oracle whose frozen gradients are None (torch's AdamW skips them, decay included), at the
    bars of the golden-trajectory test (tests/test_gpu_models.py): loss 1e-4, parameters 2e-6 after one step and 5e-6 after three."""
    from dostransformer_amd.train import Trainer
    torch.manual_seed(3)
    model = _recipe(_make(kind), which)
    g = _batch(kind, 21)
    _assert_fused(model, g.clone().to(DEV))
    frozen = set(model.flat_params().frozen)
    ref = _oracle_steps(kind, model, frozen, g, 2, 2, 3, 1e-4)
    tr = Trainer(model, lr=1e-4, beta=1.0)
    g = g.to(DEV)
    worst = {}
    for i in range(3):
        loss = tr.step(g)
        if i == 0:
            print(f"fine-tune oracle {kind} {which}: loss {float(loss):.8f} oracle {ref[0][0]:.8f}")
            assert abs(float(loss) - ref[0][0]) < 1e-4
        if i in (0, 2):
            w = max((float((v.detach().cpu().double() - ref[i][1][k]).abs().max()), k) for k, v in model.state_dict().items()
                    if v.is_floating_point())
            worst[i] = w
            print(f"fine-tune oracle {kind} {which}: after step {i + 1} worst parameter error {w[0]:.3e} at {w[1]}")
    assert worst[0][0] < 2e-6, worst
    assert worst[2][0] < 5e-6, worst
    for n in frozen:                                                 # the oracle left them alone too
        assert torch.equal(ref[2][1][n], model.state_dict()[n].detach().cpu().double())


@pytest.mark.parametrize("which", ["A", "B", "C"])
def test_module_path_leaves_frozen_grads_none(which):
    """model(g) -> loss.backward(): a frozen parameter's .grad stays None (torch's behaviour), the trainable ones get bitwise the
    gradients of the all-trainable model (a gradient on the returned node embeddings included: under a frozen trunk it reaches
    frozen parameters only)."""
    torch.manual_seed(5)
    model = _recipe(_make("phonon"), which)
    twin = _twin_of(model, lambda: _make("phonon"))
    g = _batch("phonon", 23).to(DEV)
    _assert_fused(model, g)
    gen = torch.Generator().manual_seed(1)
    w = [torch.randn(4, 51, generator=gen).to(DEV), torch.randn(4, 51, generator=gen).to(DEV)]
    for mdl in (model, twin):
        dg, x, ds = mdl(g)
        ((dg * w[0]).sum() + (ds * w[1]).sum() + x.sum() * 1e-3).backward()
    frozen = model.flat_params().frozen
    tw = dict(twin.named_parameters())
    n_train = 0
    for n, p in model.named_parameters():
        if n in frozen:
            assert p.grad is None, n
        elif n in model.flat_params().P:
            assert p.grad is not None and torch.equal(p.grad, tw[n].grad), n
            n_train += 1
    assert n_train == len(model.trainable_names()) > 0
    # and torch.optim.AdamW, which skips grad None, moves no frozen parameter
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    torch.optim.AdamW([p for p in model.parameters()], lr=1e-3).step()
    for n, p in model.named_parameters():
        assert torch.equal(p, before[n]) == (n in frozen or p.grad is None), n


def test_guard_sees_the_trainable_gradient_only():
    """Recipe A behind max_grad_norm: the norm is the float64 norm of the twin's TRAINABLE gradients (what clip_grad_norm_ over the
    trainable parameters sees), within the norm bar of tests/test_gpu_trainer_guard.py (fp32: 1e-4 relative); locate() keeps
    naming the right parameter in the [trainable | frozen] layout."""
    from dostransformer_amd import guard
    from dostransformer_amd.train import Trainer
    norm_bar = 1e-4
    torch.manual_seed(9)
    model = _recipe(_make("phonon"), "A")
    twin = _twin_of(model, lambda: _make("phonon"))
    init = {n: p.detach().clone() for n, p in model.named_parameters()}
    g = _batch("phonon", 24).to(DEV)
    _assert_fused(model, g)
    twin_tr = Trainer(twin, lr=0.0, weight_decay=0.0)
    twin_tr.step(g)
    tfp = twin.flat_params()
    tr = Trainer(model, lr=LR, max_grad_norm=1e-3)
    tr.step(g)
    fp = tr._fp
    total = float(torch.sqrt(sum(tfp.G[n].double().pow(2).sum() for n in fp.trainable_names())))
    everything = float(tfp.grad.double().pow(2).sum().sqrt())
    got = float(tr.grad_norm)
    print(f"guard norm {got:.9e}  trainable {total:.9e}  all {everything:.9e}")
    assert abs(got - total) <= norm_bar * total and abs(everything - total) > 10 * norm_bar * total
    r = tr.guard_report()
    assert r.applied == 1 and r.skipped == 0 and abs(r.clip - 1e-3 / (total + 1e-6)) <= 2 * norm_bar
    for n in fp.frozen:
        assert torch.equal(fp.P[n], init[n]), n
    for n, o in zip(fp.names, fp.offsets):
        assert guard.locate(fp, o) == (n, 0) and guard.locate(fp, o + fp.P[n].numel() - 1) == (n, fp.P[n].numel() - 1)


def test_checkpoint_resume_is_bitwise_and_files_cross_frozen_sets(tmp_path):
    from dostransformer_amd import checkpoint
    from dostransformer_amd.train import Trainer
    b = _padded("phonon", (21, 22))
    seq = [b[0], b[1], b[0]]
    torch.manual_seed(11)
    a = _recipe(_make("phonon"), "B")
    start = copy.deepcopy(a.state_dict())
    ta = Trainer(a, lr=LR, replay=True)
    for g in seq:
        ta.step(g)
    c = _recipe(_make("phonon"), "B")
    c.load_state_dict(copy.deepcopy(start))
    tc = Trainer(c, lr=LR, replay=True)
    for g in seq[:2]:
        tc.step(g)
    path = str(tmp_path / "ft.pt")
    checkpoint.save(path, c, tc)
    assert torch.load(path, weights_only=True)["optimizer"]["trainable"] == c.flat_params().trainable_names()
    torch.manual_seed(99)                                            # everything must come from the file
    d = _recipe(_make("phonon"), "B")
    td = Trainer(d, lr=5e-2, replay=True)
    checkpoint.load(path, d, td)
    assert td.step_count == 2 and td.lr == LR
    td.step(seq[2])
    for (k, va), (_, vd) in zip(a.state_dict().items(), d.state_dict().items()):
        assert torch.equal(va, vd), k
    fa, fd = ta._fp, td._fp
    assert fa.names == fd.names and torch.equal(ta._m, td._m) and torch.equal(ta._v, td._v)
    # a file from an all-trainable run loads into a partly frozen trainer (by name), which then trains its own set only
    full = _make("phonon")
    tf = Trainer(full, lr=LR)
    tf.step(seq[0])
    p_full = str(tmp_path / "full.pt")
    checkpoint.save(p_full, full, tf)
    e = _recipe(_make("phonon"), "A")
    te = Trainer(e, lr=LR)
    checkpoint.load(p_full, e, te)
    assert te.step_count == 1
    before = {n: p.detach().clone() for n, p in e.named_parameters()}
    te.step(seq[1])
    fz = te._fp.frozen
    assert fz and all(torch.equal(dict(e.named_parameters())[n], before[n]) for n in fz)
    assert all(not torch.equal(dict(e.named_parameters())[n], before[n]) for n in te._fp.trainable_names())
    checkpoint.load(path, full, tf)                                  # ... and the reverse
    assert tf.step_count == 2


def test_trainer64_honours_frozen_parameters():
    from dostransformer_amd.train64 import Trainer64
    from tests.test_gpu_train64 import ATOMS_A, ATOMS_B, _collate, _crystals, _module, _switch
    model = _switch(_module(seed=41).freeze(*TRUNK))
    twin = _switch(_module(seed=41))
    init = {n: p.detach().clone() for n, p in model.named_parameters()}
    batches = [_collate(_crystals(a, s)).to(DEV) for a, s in ((ATOMS_A, 51), (ATOMS_B, 52))]
    for replay in (False, True):
        tr = Trainer64(model, lr=LR, weight_decay=WD, betas=BETAS, eps=EPS, replay=replay)
        twin_tr = Trainer64(twin, lr=0.0, weight_decay=0.0, replay=replay)
        for i, g in enumerate((batches[0], batches[1], batches[0])):
            loss = _check_step(tr, twin_tr, lambda t, g=g: t.step(g), i + 1, init, f64=True)
            assert loss.dtype == torch.float64
        init = {n: p.detach().clone() for n, p in model.named_parameters()}     # (the second trainer starts from zero moments)
        for n in tr._fp.frozen:
            assert n.startswith(TRUNK)


def test_graphnetwork_trainer64_honours_frozen_parameters():
    from dostransformer_amd import synth
    from dostransformer_amd.train64 import GraphnetworkTrainer64
    from tests.test_gpu_baselines64 import _gn
    model, twin = _gn(32, seed=3).freeze(*TRUNK).to(DEV), _gn(32, seed=3).to(DEV)
    init = {n: p.detach().clone() for n, p in model.named_parameters()}
    g = synth.phonon_batch(5, seed=31, dtype=torch.float64).to(DEV)
    tr = GraphnetworkTrainer64(model, lr=LR, weight_decay=WD, betas=BETAS, eps=EPS)
    twin_tr = GraphnetworkTrainer64(twin, lr=0.0, weight_decay=0.0)
    for i in range(2):
        _check_step(tr, twin_tr, lambda t: t.step(g), i + 1, init, f64=True)
    names = tr._fp.trainable_names()
    assert "out_layer.0.weight" in names and "embeddings.weight" in names and not any(n.startswith(TRUNK) for n in names)


@pytest.mark.parametrize("mode", ["eager", "replay"])
def test_fp32_graphnetwork_honours_frozen_parameters_and_ends_behind_the_head(mode):
    from dostransformer_amd import synth
    from dostransformer_amd.batch import bucket_sizes, pad_batch
    from dostransformer_amd.embedder_eDOS.graphnetwork import Graphnetwork
    from dostransformer_amd.train import Trainer
    torch.manual_seed(2)
    mk = lambda: Graphnetwork(2, 200, 41, 2, 64, 201, DEV).to(DEV)
    model = mk().freeze(*TRUNK)
    twin = _twin_of(model, mk)
    init = {n: p.detach().clone() for n, p in model.named_parameters()}
    g = synth.edos_batch(4, seed=25, dtype=torch.float32).to(DEV)
    g = pad_batch(g, *bucket_sizes(g.meta.num_nodes, g.meta.num_edges))
    kw = dict(replay=mode == "replay")
    tr = Trainer(model, lr=LR, weight_decay=WD, betas=BETAS, eps=EPS, **kw)
    twin_tr = Trainer(twin, lr=0.0, weight_decay=0.0, **kw)
    for i in range(2):
        _check_step(tr, twin_tr, lambda t: t.step(g), i + 1, init)
    st, full = tr.program_stats(), twin_tr.program_stats()
    assert st["launches"] < full["launches"] and set(st["wgrad_keys"]) == {"out_layer.0.weight"}
    assert not any(k.startswith(TRUNK) for k in st["wgrad_keys"]) and any(k.startswith(TRUNK) for k in full["wgrad_keys"])


def test_wide_program_honours_frozen_parameters():
    """hidden > 256: the unfused program has the same cut"""
    from dostransformer_amd.train import Trainer
    torch.manual_seed(4)
    mk = lambda: _make("phonon", H=384, T=1)
    model = _recipe(mk(), "A")
    twin = _twin_of(model, mk)
    init = {n: p.detach().clone() for n, p in model.named_parameters()}
    g = _batch("phonon", 26).to(DEV)
    tr = Trainer(model, lr=LR, weight_decay=WD, betas=BETAS, eps=EPS)
    twin_tr = Trainer(twin, lr=0.0, weight_decay=0.0)
    for i in range(2):
        _check_step(tr, twin_tr, lambda t: t.step(g), i + 1, init)
    st, full = tr.program_stats(), twin_tr.program_stats()
    assert st["launches"] < full["launches"] and st["entries"].count("dosx_dense_slots_bwd") == 0
    assert full["entries"].count("dosx_dense_slots_bwd") == 1


def test_refusals():
    from dostransformer_amd._lib import DosxError
    from dostransformer_amd.train import Trainer
    with pytest.raises(DosxError, match="not with dist"):
        Trainer(_recipe(_make("phonon"), "A"), dist=_FakeDist(None))
    Trainer(_make("phonon"), dist=_FakeDist(None))                    # nothing frozen: accepted as before
    model = _make("phonon")
    tr = Trainer(model, lr=LR)
    g = _batch("phonon", 21).to(DEV)
    tr.step(g)
    tr.check()
    model.fc.weight.requires_grad_(False)                             # flags changed, update_trainable() not called
    before = model.fc.weight.detach().clone()
    tr.step(g)                                                        # (the step still trains the earlier set ...)
    assert not torch.equal(model.fc.weight, before)
    with pytest.raises(DosxError, match=r"update_trainable\(\)"):     # ... and check() says which call is missing
        tr.check()
    assert model.update_trainable()
    tr.check()
    before = model.fc.weight.detach().clone()
    tr.step(g)
    assert torch.equal(model.fc.weight, before) and tr._fp.frozen == {"fc.weight"}
    with pytest.raises(ValueError, match="GN_encodr"):
        model.freeze("GN_encodr")
