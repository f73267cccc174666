"""Optimizer parameter groups on a real MI355X (include/dosx.h: DosxAdamWGroups, dosx_adamw_grouped*; param_groups.py;
``Trainer(param_groups=...)``).

The main net needs no tolerance: a grouped launch is BITWISE what the ungrouped kernels (ops.adamw / ops.adamw64 and their guarded
forms) do to clones, one call per maximal run of chunks of one group with that group's (lr, weight_decay) - at the sizes where
the chunk indexing can go wrong.  The trainers are held to the same composition tensor by tensor, from the gradient an
ungrouped twin (lr = weight_decay = 0, same mode) leaves in its flat buffer.  Only the comparison with torch.optim.AdamW has a
bar: the project's own for that comparison (tests/test_gpu_ffn.py: err < 1e-6 for fp32; tests/test_gpu_train64.py: 1e-9 for
float64)."""
import copy

import pytest
import torch

from tests import test_gpu_trainer_guard as TG
from tests.gpu_util import DEV, err, ops

pytestmark = pytest.mark.gpu

B1, B2, EPS = 0.9, 0.999, 1e-8
DTYPES = [torch.float32, torch.float64]
IDS = ["f32", "f64"]
NAN = float("nan")
# one sweep of the capped grid: dosx_adamw 4096 workgroups x 256 threads x 4 floats, dosx_adamw_f64 (ADAMW64_MAX_WGS) 2048 x 256 x 2
SWEEP = {torch.float32: 4096 * 1024, torch.float64: 2048 * 512}


def _groups16():
    """16 groups: group 0 without weight decay, group 2 at lr = 0, every pair distinct"""
    return [(0.0 if k == 2 else 1e-3 * (k + 1) / 16, 1e-2 * k / 4) for k in range(16)]


def _shape(case, dtype):
    """-> (chunk ids, groups)"""
    g16 = _groups16()
    if case == "one":                      # n = 64: one chunk, not group 0
        return [1], g16[:2]
    if case == "aba":                      # n = 192: A, B, A
        return [0, 1, 0], g16[:2]
    if case == "every":                    # n = 64 * 17: a change at every chunk of the first workgroup's sweep, group 15 in use
        return [c % 16 for c in range(16)] + [3], g16
    if case == "lr0":                      # a run of the lr = 0 group between two others
        return [0, 2, 2, 1], g16[:3]
    assert case == "sweep"                 # one sweep of the capped grid + 3 chunks: the last chunks are not the first one's group
    n_chunks = SWEEP[dtype] // 64 + 3
    return [(c // 4099) % 3 for c in range(n_chunks - 3)] + [3, 3, 3], g16[:4]


def _runs(ids):
    out, a = [], 0
    for c in range(1, len(ids) + 1):
        if c == len(ids) or ids[c] != ids[a]:
            out.append((a, c, ids[a]))
            a = c
    return out


def _state(dtype, n, step, seed):
    """p, g, m, v of n + 64 elements (a sentinel chunk behind n); step > 1: moments as if steps had been taken"""
    gen = torch.Generator().manual_seed(seed)
    r = lambda: torch.randn(n + 64, generator=gen, dtype=torch.float64)
    p, g = r(), r() * 0.1
    m = r() * 0.05 if step > 1 else torch.zeros(n + 64, dtype=torch.float64)
    v = (r() * 0.05) ** 2 if step > 1 else torch.zeros(n + 64, dtype=torch.float64)
    return [t.to(dtype).to(DEV) for t in (p, g, m, v)]


def _compose(dtype, state, ids, groups, step, grad_scale=1.0, recs=None):
    """The UNGROUPED kernels on clones, one call per maximal run of equal group id -> (p, m, v)"""
    o = ops()
    out = [t.clone() for t in state]
    for a, b, k in _runs(ids):
        lr, wd = groups[k]
        p, g, m, v = (t[64 * a:64 * b].clone() for t in state)
        n = 64 * (b - a)
        if recs is not None:
            (o.adamw_guarded if dtype == torch.float32 else o.adamw64_guarded)(p, g, m, v, n, lr, B1, B2, EPS, wd, recs[k][0])
        elif dtype == torch.float32:
            o.adamw(p, g, m, v, n, lr, B1, B2, EPS, wd, step, grad_scale)
        else:
            o.adamw64(p, g, m, v, n, lr, B1, B2, EPS, wd, step)
        for dst, src in zip((out[0], out[2], out[3]), (p, m, v)):
            dst[64 * a:64 * b].copy_(src)
    return out[0], out[2], out[3]


def _ids_dev(ids):
    return torch.tensor(ids, dtype=torch.uint8).to(DEV)


def _same_bits(got, want, tag):
    for name, a, b in zip("pmv", got, want):
        assert torch.equal(a, b), (tag, name, int((a != b).sum()))


# =====================================================================================================================
# 1. bitwise composition
# =====================================================================================================================
@pytest.mark.parametrize("step", [1, 7])
@pytest.mark.parametrize("case", ["one", "aba", "every", "lr0", "sweep"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_grouped_launch_is_the_ungrouped_launch_run_by_run(dtype, case, step):
    o = ops()
    ids, groups = _shape(case, dtype)
    n = 64 * len(ids)
    if case == "sweep":
        assert n == SWEEP[dtype] + 192 and ids[0] != ids[-1]
    if case == "every":
        assert max(ids) == 15 and all(ids[c] != ids[c + 1] for c in range(16))
    assert any(wd == 0.0 for _, wd in groups)
    scales = (1.0, 0.37) if dtype == torch.float32 else (1.0,)
    for gs in scales:
        st = _state(dtype, n, step, 11 + step)
        want = _compose(dtype, st, ids, groups, step, gs)
        p, g, m, v = (t.clone() for t in st)
        if dtype == torch.float32:
            o.adamw_grouped(p, g, m, v, n, _ids_dev(ids), groups, B1, B2, EPS, step, gs)
        else:
            o.adamw64_grouped(p, g, m, v, n, _ids_dev(ids), groups, B1, B2, EPS, step)
        _same_bits((p, m, v), want, (case, step, gs))
        assert torch.equal(g, st[1])                                              # g is only read, the sentinel chunk untouched
        for x, x0 in zip((p, m, v), (st[0], st[2], st[3])):
            assert torch.equal(x[n:], x0[n:])
        if case == "lr0":                                                         # lr = 0: parameters bitwise, moments advanced
            assert torch.equal(p[64:192], st[0][64:192])
            assert not torch.equal(m[64:192], st[2][64:192]) and not torch.equal(v[64:192], st[3][64:192])
            assert not torch.equal(p[:64], st[0][:64])


# =====================================================================================================================
# 2. one group with the trainer's values is the ungrouped launch
# =====================================================================================================================
@pytest.mark.parametrize("guarded", [False, True], ids=["plain", "guarded"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_one_group_is_the_ungrouped_launch(dtype, guarded):
    o = ops()
    n, step, lr, wd = 64 * 33, 4, 1e-3, 1e-2
    st = _state(dtype, n, step, 5)
    a, b = [t.clone() for t in st], [t.clone() for t in st]
    ids = torch.zeros(n // 64, dtype=torch.uint8, device=DEV)
    f32 = dtype == torch.float32
    if guarded:
        rec, ws = o.guard_buffers(DEV)
        o.grad_guard(st[1], n, rec, ws, 0.5, lr, B1, B2, step)
        (o.adamw_guarded if f32 else o.adamw64_guarded)(*a, n, lr, B1, B2, EPS, wd, rec)
        (o.adamw_grouped_guarded if f32 else o.adamw64_grouped_guarded)(*b, n, ids, [(lr, wd)], B1, B2, EPS, step, rec)
        assert o.guard_read(rec).clip < 1.0
    elif f32:
        o.adamw(*a, n, lr, B1, B2, EPS, wd, step, 1.0)
        o.adamw_grouped(*b, n, ids, [(lr, wd)], B1, B2, EPS, step, 1.0)
    else:
        o.adamw64(*a, n, lr, B1, B2, EPS, wd, step)
        o.adamw64_grouped(*b, n, ids, [(lr, wd)], B1, B2, EPS, step)
    for x, y, x0 in zip(a, b, st):
        assert torch.equal(x, y)
    assert not torch.equal(a[0], st[0])


# =====================================================================================================================
# 3. guarded
# =====================================================================================================================
@pytest.mark.parametrize("state", ["quiet", "clipping", "after_skip"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_grouped_guarded_launch_is_the_guarded_launch_run_by_run(dtype, state):
    """The reference record of group k is the one dosx_grad_guard_* writes when called with lr_k (one record per group, fed the
    same gradients in the same order, so their sticky counts agree).  after_skip: attempt 1 carries a NaN - skipped, p, m, v
    bitwise untouched in every group - so that attempt 2 runs at AdamW time t = 1 != step = 2: the per-group step sizes are
    recomputed on the device."""
    o = ops()
    ids = [c % 4 for c in range(16)] + [2]
    groups = _groups16()[:4]
    n = 64 * len(ids)
    f32 = dtype == torch.float32
    st = _state(dtype, n, 3, 31)
    recs = [o.guard_buffers(DEV) for _ in groups]
    mine = o.guard_buffers(DEV)
    fn = o.adamw_grouped_guarded if f32 else o.adamw64_grouped_guarded
    max_norm = 0.25 * float(st[1][:n].double().norm()) if state == "clipping" else None
    step = 1
    if state == "after_skip":
        bad = st[1].clone()
        bad[n - 3] = NAN
        for (rec, ws), (lr, _) in zip(recs + [mine], groups + [(1e-3, 0.0)]):
            o.grad_guard(bad, n, rec, ws, max_norm, lr, B1, B2, step)
        p, g, m, v = st[0].clone(), bad, st[2].clone(), st[3].clone()
        fn(p, g, m, v, n, _ids_dev(ids), groups, B1, B2, EPS, step, mine[0])
        r = o.guard_read(mine[0])
        assert (r.skip, r.skipped, r.n_bad, r.first_bad) == (1, 1, 1, n - 3)
        _same_bits((p, m, v), (st[0], st[2], st[3]), "skipped step")
        step = 2
    for (rec, ws), (lr, _) in zip(recs + [mine], groups + [(1e-3, 0.0)]):
        o.grad_guard(st[1], n, rec, ws, max_norm, lr, B1, B2, step)
    r = o.guard_read(mine[0])
    assert r.skip == 0 and r.t == (1 if state == "after_skip" else step) and (r.clip < 1.0) == (state == "clipping")
    want = _compose(dtype, st, ids, groups, step, recs=recs)
    p, g, m, v = (t.clone() for t in st)
    fn(p, g, m, v, n, _ids_dev(ids), groups, B1, B2, EPS, step, mine[0])
    _same_bits((p, m, v), want, state)
    assert torch.equal(g, st[1]) and not torch.equal(p[:n], st[0][:n])
    for x, x0 in zip((p, m, v), (st[0], st[2], st[3])):
        assert torch.equal(x[n:], x0[n:])


# =====================================================================================================================
# 4. against torch.optim.AdamW with param groups
# =====================================================================================================================
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_three_steps_against_torch_adamw_with_param_groups(dtype):
    """Three tensors in three groups, lr in {1e-3, 1e-4, 0}, three steps; the reference is torch.optim.AdamW on the CPU in float64,
    foreach=False.  fp32: err < 1e-6 (tests/test_gpu_ffn.py's bar and measure); float64: 1e-9 on the parameters
    (tests/test_gpu_train64.py's bar: the largest absolute difference)."""
    o = ops()
    sizes, lrs, wds = (1003, 64, 130), (1e-3, 1e-4, 0.0), (1e-2, 0.0, 1e-2)
    offs, tot, ids = [], 0, []
    for k, s in enumerate(sizes):
        offs.append(tot)
        ids += [k] * ((s + 63) // 64)
        tot += (s + 63) // 64 * 64
    gen = torch.Generator().manual_seed(3)
    p = torch.zeros(tot, dtype=dtype, device=DEV)
    refs = []
    for s, off in zip(sizes, offs):
        x = torch.randn(s, generator=gen, dtype=torch.float64).to(dtype)
        p[off:off + s] = x.to(DEV)
        refs.append(torch.nn.Parameter(x.double().clone()))
    opt = torch.optim.AdamW([{"params": [r], "lr": lr, "weight_decay": wd} for r, lr, wd in zip(refs, lrs, wds)], betas=(B1, B2),
                            eps=EPS, foreach=False)
    p0, m, v = p.clone(), torch.zeros_like(p), torch.zeros_like(p)
    chunk = _ids_dev(ids)
    for step in range(1, 4):
        g = torch.zeros(tot, dtype=dtype, device=DEV)
        for r, s, off in zip(refs, sizes, offs):
            x = (torch.randn(s, generator=gen, dtype=torch.float64) * 0.1).to(dtype)
            g[off:off + s] = x.to(DEV)
            r.grad = x.double().clone()
        opt.step()
        (o.adamw_grouped if dtype == torch.float32 else o.adamw64_grouped)(p, g, m, v, tot, chunk, list(zip(lrs, wds)), B1, B2, EPS, step)
    for k, (r, s, off) in enumerate(zip(refs, sizes, offs)):
        got = p[off:off + s].cpu()
        if dtype == torch.float32:
            e = err(got, r.detach())
            print(f"adamw_grouped[f32] group {k} against torch: err {e:.3g} (1e-6)")
            assert e < 1e-6
        else:
            e = float((got - r.detach()).abs().max())
            print(f"adamw_grouped[f64] group {k} against torch: {e:.3g} (1e-9)")
            assert e <= 1e-9
    assert torch.equal(p[offs[2]:offs[2] + sizes[2]], p0[offs[2]:offs[2] + sizes[2]])             # lr = 0: nothing moved, decay included
    assert not torch.equal(p[:sizes[0]], p0[:sizes[0]])


# =====================================================================================================================
# 5. trainers
# =====================================================================================================================
class _Fam:
    """One trainer family: same-bits model factory, trainer factory, one batch."""

    def __init__(self, name):
        from dostransformer_amd import synth
        from dostransformer_amd.train import Trainer
        from dostransformer_amd.train64 import GraphnetworkTrainer64, Trainer64
        self.name, self.f64 = name, name in ("t64", "gn64")
        if name == "phonon":                                   # the L3 T1 H32 model of tests/test_gpu_step.py
            from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
            self._mk = lambda: DOSTransformer_phonon(3, 1, 118, 4, 32, DEV, 0.0).to(DEV)
            self.g = synth.phonon_batch(4, seed=81, dtype=torch.float32).to(DEV)
            self._tr = Trainer
        elif name == "edos":
            from dostransformer_amd.embedder_eDOS.DOSTransformer import DOSTransformer
            self._mk = lambda: DOSTransformer(3, 1, 200, 41, 2, 32, DEV, 0.0).to(DEV)
            self.g = synth.edos_batch(4, seed=82, dtype=torch.float32).to(DEV)
            self._tr = Trainer
        else:
            cfg = TG._cfg(name)
            self._mk, self.g = cfg._mk, cfg.g
            self._tr = Trainer64 if name == "t64" else GraphnetworkTrainer64

    def model(self):
        torch.manual_seed(3)
        return self._mk()

    def trainer(self, model, mode, **kw):
        return self._tr(model, betas=(B1, B2), eps=EPS, **({"replay": True} if mode == "replay" else {}), **kw)


_FAMS = {}


def _fam(name):
    if name not in _FAMS:
        _FAMS[name] = _Fam(name)
    return _FAMS[name]


def _views(fp, buf):
    return {n: buf[o:o + fp.P[n].numel()] for n, o in zip(fp.names, fp.offsets)}


def _adamw_by_tensor(P, G, M, V, names, group_of, values, step, f64, recs=None):
    """ops.adamw / ops.adamw64 (recs: their guarded forms, one record per group) on clones, one tensor at a time with its group's
    (lr, wd) -> {name: (p, m, v)}.  Each tensor in a buffer of its own, zero-padded to the 64 elements every parameter is aligned
    to in the flat buffer: the kernels' vector body then handles every element, as it does there."""
    o = ops()
    out = {}
    for n in names:
        lr, wd = values[group_of[n]]
        k = P[n].numel()
        kp = (k + 63) // 64 * 64
        p, g, m, v = (torch.zeros(kp, dtype=P[n].dtype, device=DEV) for _ in range(4))
        for dst, src in ((p, P), (g, G), (m, M), (v, V)):
            dst[:k].copy_(src[n].detach().reshape(-1))
        if recs is not None:
            (o.adamw64_guarded if f64 else o.adamw_guarded)(p, g, m, v, kp, lr, B1, B2, EPS, wd, recs[group_of[n]][0])
        elif f64:
            o.adamw64(p, g, m, v, kp, lr, B1, B2, EPS, wd, step)
        else:
            o.adamw(p, g, m, v, kp, lr, B1, B2, EPS, wd, step, 1.0)
        out[n] = (p[:k], m[:k], v[:k])
    return out


def _composed_steps(name, mode, groups, steps=3, lr=1e-3, wd=1e-2, prepare=None, max_grad_norm=None, between=None):
    """``steps`` steps of a grouped trainer, each against the composition: an ungrouped twin (lr = wd = 0, same mode, loaded with
    the current parameters) leaves the step's gradient in its flat buffer; every trainable tensor must then be, bit for bit, what
    the ungrouped per-tensor call with its group's CURRENT values makes of it.  -> (trainer, model, initial parameters)"""
    o = ops()
    fam = _fam(name)
    model, twin = fam.model(), fam.model()
    if prepare is not None:
        prepare(model)
    init = {n: p.detach().clone() for n, p in model.named_parameters()}
    frozen0 = {n for n, p in model.named_parameters() if not p.requires_grad}
    kw = {} if max_grad_norm is None else {"max_grad_norm": max_grad_norm}
    tr = fam.trainer(model, mode, lr=lr, weight_decay=wd, param_groups=groups(model) if callable(groups) else groups, **kw)
    twin_tr = fam.trainer(twin, mode, lr=0.0, weight_decay=0.0)
    assert tr.lr == lr and tr.wd == wd and tr.param_groups[0]["lr"] == lr and tr.param_groups[0]["weight_decay"] == wd
    group_of = {n: k for k, grp in enumerate(tr.param_groups) for n in grp["names"]}
    recs = None if max_grad_norm is None else [o.guard_buffers(DEV) for _ in tr.param_groups]
    for i in range(steps):
        step = i + 1
        twin.load_state_dict(copy.deepcopy(model.state_dict()))
        twin_tr.step(fam.g)
        tfp = twin_tr._fp
        assert not tfp.frozen
        fp0 = tr._fp
        if fp0 is None:
            P0 = {n: p.detach().clone() for n, p in model.named_parameters()}
            M0 = V0 = None
        else:
            P0 = {n: t.clone() for n, t in fp0.P.items()}
            M0, V0 = ({n: t.clone() for n, t in _views(fp0, b).items()} for b in (tr._m, tr._v))
        values = [(grp["lr"], grp["weight_decay"]) for grp in tr.param_groups]
        loss = tr.step(fam.g)
        fp = tr._fp
        assert tr._chunk_group.numel() == fp.n_train // 64 and tr._chunk_group.device == fp.flat.device
        if M0 is None:
            M0 = {n: torch.zeros_like(fp.P[n]).reshape(-1) for n in fp.names}
            V0 = {n: torch.zeros_like(fp.P[n]).reshape(-1) for n in fp.names}
        train = fp.trainable_names()
        if recs is not None:                               # the record dosx_grad_guard_* writes when called with lr_k, same gradient
            assert not fp.frozen and tfp.n_train == fp.n_train and tfp.names == fp.names
            for (rec, ws), (lr_k, _) in zip(recs, values):
                o.grad_guard(tfp.grad, tfp.n_train, rec, ws, max_grad_norm, lr_k, B1, B2, step)
        want = _adamw_by_tensor(P0, tfp.G, M0, V0, train, group_of, values, step, fam.f64, recs)
        torch.cuda.synchronize()
        Mv, Vv = _views(fp, tr._m), _views(fp, tr._v)
        moved = 0
        for n in train:
            p, m, v = want[n]
            assert torch.equal(fp.P[n].reshape(-1), p), ("param", n, step, group_of[n])
            assert torch.equal(Mv[n], m) and torch.equal(Vv[n], v), ("moments", n, step)
            moved += not torch.equal(p, P0[n].reshape(-1))
        assert moved > len(train) // 2
        for n in fp.frozen:                                # bitwise what they were before the step (frozen from the start: the
            assert torch.equal(fp.P[n].reshape(-1), P0[n].reshape(-1)), ("frozen parameter moved", n, step)      # initial values)
            assert torch.equal(Mv[n], M0[n]) and torch.equal(Vv[n], V0[n]), ("frozen moments", n, step)
            if n in frozen0:
                assert torch.equal(fp.P[n], init[n]) and not bool(Mv[n].any()) and not bool(Vv[n].any()), ("frozen", n, step)
        assert bool(torch.isfinite(loss))
        if between is not None:
            between(tr, step)
    tr.check()
    return tr, model, init


def _three_groups(model):
    """the trunk at a tenth of the rate, the transformer stacks without weight decay, the rest implicit"""
    return [{"params": ["GN_encoder.", "stacked_processor."], "lr": 1e-4},
            {"params": [n for n, _ in model._live_named() if n.startswith("transformer")] or ["GN_decoder."], "weight_decay": 0.0}]


@pytest.mark.parametrize("mode", ["eager", "replay"])
@pytest.mark.parametrize("name", ["phonon", "edos", "t64", "gn64"])
def test_trainer_with_groups_steps_every_tensor_with_its_groups_values(name, mode):
    tr, _, _ = _composed_steps(name, mode, _three_groups)
    assert len(tr.param_groups) == 3 and all(grp["names"] for grp in tr.param_groups)
    if mode == "replay":
        assert tr.slot_hits >= 1


@pytest.mark.parametrize("name", ["phonon", "t64"])
def test_groups_with_frozen_parameters(name):
    """freeze() in front of the first step and again after the second: frozen tensors bitwise untouched, the chunk map rebuilt
    for the new layout; a group whose parameters are all frozen touches nothing."""
    def later(tr, step):
        if step == 2:
            before = tr._chunk_group
            tr.model.freeze("GN_encoder.")
            assert tr.model._flat is not tr._fp
            tr._before = before
    tr, model, _ = _composed_steps(name, "eager", _three_groups, prepare=lambda m: m.freeze("transformer"), between=later)
    fp = tr._fp
    assert tr._chunk_group is not tr._before and tr._chunk_group.numel() == fp.n_train // 64 < tr._before.numel()
    assert any(n.startswith("GN_encoder.") for n in fp.frozen) and any(n.startswith("transformer") for n in fp.frozen)
    assert all(n in fp.frozen for n in tr.param_groups[2]["names"])


@pytest.mark.parametrize("name", ["phonon", "t64"])
def test_groups_with_max_grad_norm(name):
    fam = _fam(name)
    probe_tr = fam.trainer(fam.model(), "eager", lr=0.0, weight_decay=0.0, max_grad_norm=1e30)
    probe_tr.step(fam.g)
    norm = float(probe_tr.grad_norm)
    tr, _, _ = _composed_steps(name, "eager", _three_groups, max_grad_norm=0.5 * norm)
    assert tr.guard_report().applied == 3 and tr.guarded


def test_learning_rate_schedule_on_a_replayed_trainer_records_nothing():
    """param_groups[k]["lr"] assigned between the steps of a replayed trainer: the next step uses it (the composition reads the
    current values) and nothing new is recorded."""
    seen = []

    def between(tr, step):
        seen.append((tr.slot_misses, tr.slot_hits))
        tr.param_groups[1]["lr"] = 1e-4 * 0.5 ** step
        tr.param_groups[0]["lr"] = 1e-3 * 0.9 ** step
    tr, _, _ = _composed_steps("phonon", "replay", _three_groups, steps=4, between=between)
    assert [m for m, _ in seen] == [1, 1, 1, 1] and [h for _, h in seen] == [0, 1, 2, 3]
    assert tr.param_groups[1]["lr"] == 1e-4 * 0.5 ** 4 and tr.lr == 1e-3


def test_no_decay_groups_keep_the_norms_out_of_the_weight_decay():
    from dostransformer_amd import param_groups as pg
    tr, model, init = _composed_steps("phonon", "eager", lambda m: [{"params": pg.no_decay(m), "weight_decay": 0.0}], steps=1)
    name = "transformer.layer_norm.weight"
    assert name in tr.param_groups[1]["names"] and tr.param_groups[1]["weight_decay"] == 0.0
    # after one step from zero moments: p - lr * g / (|g| + eps), without the 1 - lr * wd the decayed twin would apply
    plain = _fam("phonon").trainer(_fam("phonon").model(), "eager", lr=1e-3, weight_decay=1e-2)
    plain.step(_fam("phonon").g)
    assert not torch.equal(plain._fp.P[name], tr._fp.P[name])
    assert torch.equal(plain._fp.P["fc.weight"], tr._fp.P["fc.weight"])           # a decayed weight: the same step in both


# =====================================================================================================================
# 6. checkpoint resume
# =====================================================================================================================
@pytest.mark.parametrize("name", ["phonon", "t64"])
def test_grouped_trainer_resumes_bitwise(name):
    fam = _fam(name)
    model = fam.model()
    tr = fam.trainer(model, "eager", lr=1e-3, weight_decay=1e-2, param_groups=_three_groups(model))
    tr.step(fam.g)
    tr.param_groups[1]["lr"] = 3e-5                         # a schedule's value: it must come back from the file, by group index
    tr.step(fam.g)
    sd_model, sd = copy.deepcopy(model.state_dict()), tr.state_dict()
    assert [sorted(grp) for grp in sd["param_groups"]] == [["lr", "names", "weight_decay"]] * 3
    fresh = fam.model()
    fresh.load_state_dict(sd_model)
    tr2 = fam.trainer(fresh, "eager", lr=1e-3, weight_decay=1e-2, param_groups=_three_groups(fresh))
    tr2.load_state_dict(sd)
    assert tr2.param_groups[1]["lr"] == 3e-5 and tr2.step_count == 2
    la, lb = tr.step(fam.g), tr2.step(fam.g)
    torch.cuda.synchronize()
    assert torch.equal(la, lb)
    assert tr._fp.names == tr2._fp.names and torch.equal(tr._fp.flat, tr2._fp.flat)
    assert torch.equal(tr._m, tr2._m) and torch.equal(tr._v, tr2._v)
