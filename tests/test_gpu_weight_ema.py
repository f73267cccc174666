"""The exponential moving average of the weights on a real MI355X (include/dosx.h: DosxAdamWEma, dosx_adamw_ema / _f64,
dosx_swap_buffers; ema.py; ``Trainer(ema_decay=...)``).

Two nets need no tolerance.  p', m', v' of a launch that also averages are BITWISE those of the entry without the average, on
clones, at the sizes where the indexing can go wrong.  And the average itself is BITWISE what a kernel from before this feature
leaves in ``m`` when it is handed ``g = p'``, ``m = ema``, ``beta1 = d_t``, ``grad_scale = 1``, ``lr = 0`` (``_oracle``): the
average's update is the first-moment update read with other operands.  Only the trainers' comparison with float64 arithmetic on
the host has a bar, and it is derived: each step rounds the difference once and the fma once, so after k steps an element is
within ``k x 2 x eps(T) x max(|p|, |ema|)`` (the largest magnitudes the element had so far) of the float64 recurrence run on the
same parameter snapshots with the same (T-rounded) decay.

The file's name sorts it behind the other GPU files on purpose.  tests/test_gpu_graph.py and tests/test_gpu_train_per_crystal.py
hand dosx_mlp_ln_* / dosx_ffn_* weight matrices that were allocated one after the other, and those entries refuse two matrices
more than 2 GiB apart: what a file in front of them allocates and frees decides where such a pair lands.  Run as
tests/test_gpu_ema.py (in front of them) this file's sweep-sized buffers and trainers made 8 - 19 of their cases fail with that
refusal; run last it can shift nobody's addresses."""
import contextlib
import copy

import pytest
import torch

from tests import test_gpu_param_groups as PG
from tests import test_gpu_trainer_guard as TG
from tests.gpu_util import DEV, ops

pytestmark = pytest.mark.gpu

B1, B2, EPS, LR, WD = PG.B1, PG.B2, PG.EPS, 1e-3, 1e-2
DTYPES, IDS, SWEEP = PG.DTYPES, PG.IDS, PG.SWEEP
NAN = float("nan")
DECAY = 0.999
TS = (1, 9, 8989, 8990, 8991)              # at decay 0.999 the warm-up's min switches between 8989 and 8990
FORMS = ["plain", "guarded", "grouped", "grouped_guarded"]
SIZES = {torch.float32: (1, 3, 4, 5, 67, 64 * 17, 4096 * 1024 + 7), torch.float64: (1, 2, 3, 67, 64 * 17, 2048 * 512 + 3)}
GROUPED_CASES = ("one", "aba", "sweep")    # n = 64, 192, one sweep + 192 (tests/test_gpu_param_groups.py: _shape)


def _sched(decay, warmup, t):
    from dostransformer_amd import ema
    return ema.schedule(decay, warmup, t)


_STATES = {}
_DS = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_the_shared_inputs():
    yield
    _STATES.clear()
    _DS.clear()


def _state(dtype, n, step, seed=None):
    """(p, g, m, v, ema) of n + 64 elements (a sentinel chunk behind n), never written; the small ones are made once per
    (dtype, n, step) and shared"""
    key = (dtype, n, step)
    if key in _STATES:
        return _STATES[key]
    st = PG._state(dtype, n, step, 100 + step if seed is None else seed)
    gen = torch.Generator().manual_seed(7 + step)
    e = (st[0].double().cpu() + 0.3 * torch.randn(n + 64, generator=gen, dtype=torch.float64)).to(dtype).to(DEV)
    if n <= 1 << 17:
        _STATES[key] = st + [e]
    return st + [e]


def _oracle(dtype, p_new, ema_old, n, d):
    """What the EXISTING unguarded entry leaves in ``m`` for g = p', m = ema, beta1 = d, grad_scale = 1, lr = 0 -> ema'"""
    o = ops()
    e, p, v = ema_old.clone(), p_new.clone(), torch.zeros_like(p_new)
    if dtype == torch.float32:
        o.adamw(p, p_new, e, v, n, 0.0, d, B2, EPS, 0.0, 1, 1.0)
    else:
        o.adamw64(p, p_new, e, v, n, 0.0, d, B2, EPS, 0.0, 1)
    assert torch.equal(p, p_new)                                # lr = 0: the oracle's own p does not move
    return e


def _launch(dtype, form, bufs, n, step, rec=None, ids=None, groups=None, ema=None, gs=1.0):
    """One AdamW launch of ``form`` on ``bufs`` = [p, g, m, v] through the public wrappers, with or without ``ema=``."""
    o = ops()
    f32 = dtype == torch.float32
    kw = {} if ema is None else {"ema": ema}
    if form == "plain":
        (o.adamw(*bufs, n, LR, B1, B2, EPS, WD, step, gs, **kw) if f32 else o.adamw64(*bufs, n, LR, B1, B2, EPS, WD, step, **kw))
    elif form == "guarded":
        if ema is not None:
            kw["step"] = step
        (o.adamw_guarded if f32 else o.adamw64_guarded)(*bufs, n, LR, B1, B2, EPS, WD, rec, **kw)
    elif form == "grouped":
        (o.adamw_grouped(*bufs, n, ids, groups, B1, B2, EPS, step, gs, **kw) if f32 else
         o.adamw64_grouped(*bufs, n, ids, groups, B1, B2, EPS, step, **kw))
    else:
        (o.adamw_grouped_guarded if f32 else o.adamw64_grouped_guarded)(*bufs, n, ids, groups, B1, B2, EPS, step, rec, **kw)


def _cases(dtype, form):
    """-> [(n, chunk ids on the device or None, groups or None)]"""
    if "grouped" not in form:
        return [(n, None, None) for n in SIZES[dtype]]
    out = []
    for case in GROUPED_CASES:
        ids, groups = PG._shape(case, dtype)
        out.append((64 * len(ids), PG._ids_dev(ids), groups))
    assert [c[0] for c in out] == [64, 192, SWEEP[dtype] + 192]
    return out


# =====================================================================================================================
# 2. the average bit for bit over the schedule
# =====================================================================================================================
@pytest.mark.parametrize("t0", [0, 5])
@pytest.mark.parametrize("warmup", [False, True], ids=["fixed", "warmup"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_average_is_the_first_moment_update_of_the_kernel_from_before(dtype, warmup, t0):
    """t = step - t0 in {1, 9, 8989, 8990, 8991}, ungrouped at n = 67 (vector body + tail) and 64 x 17, grouped at 192."""
    ids, groups = PG._shape("aba", dtype)
    seen = set()
    for t in TS:
        step = t + t0
        d = _sched(DECAY, warmup, t)
        seen.add(d)
        for form, n in (("plain", 67), ("plain", 64 * 17), ("grouped", 192)):
            st = _state(dtype, n, 7)
            b, e = [x.clone() for x in st[:4]], st[4].clone()
            _launch(dtype, form, b, n, step, None, PG._ids_dev(ids), groups, ema=(e, DECAY, warmup, t0))
            want = _oracle(dtype, b[0], st[4], n, d)
            assert torch.equal(e, want), (form, n, t, int((e != want).sum()))
            assert torch.equal(e[n:], st[4][n:])
    assert len(seen) == (4 if warmup else 1)                    # 2/11, 10/19, 8990/8999, then the decay itself (8990 and 8991)
    if dtype == torch.float32:                                  # (the two float32 decays around the switch differ: the test can tell)
        assert ops().ema_decay_at(DECAY, True, 8989) != ops().ema_decay_at(DECAY, True, 8990)


# =====================================================================================================================
# 3. skipped steps
# =====================================================================================================================
@pytest.mark.parametrize("form", ["guarded", "grouped_guarded"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_skipped_step_leaves_the_average_and_does_not_advance_its_warmup(dtype, form):
    o = ops()
    ids, groups = PG._shape("every", dtype)
    n = 64 * len(ids)
    ids = PG._ids_dev(ids)
    st = _state(dtype, n, 7)
    rec, ws = o.guard_buffers(DEV)
    bad = st[1].clone()
    bad[n - 3] = NAN
    o.grad_guard(bad, n, rec, ws, None, LR, B1, B2, 1)
    b, e = [st[0].clone(), bad, st[2].clone(), st[3].clone()], st[4].clone()
    _launch(dtype, form, b, n, 1, rec, ids, groups, ema=(e, DECAY, True, 0))
    r = o.guard_read(rec)
    assert (r.skip, r.skipped, r.n_bad, r.first_bad) == (1, 1, 1, n - 3)
    assert torch.equal(e, st[4])                                # the average: bitwise untouched
    for x, x0 in zip((b[0], b[2], b[3]), (st[0], st[2], st[3])):
        assert torch.equal(x, x0)
    # attempt 2 is AdamW's step 1: the average warms up by the applied time
    o.grad_guard(st[1], n, rec, ws, None, LR, B1, B2, 2)
    r = o.guard_read(rec)
    assert r.skip == 0 and r.t == 1
    b = [x.clone() for x in st[:4]]
    _launch(dtype, form, b, n, 2, rec, ids, groups, ema=(e, DECAY, True, 0))
    want = _oracle(dtype, b[0], st[4], n, _sched(DECAY, True, int(r.t)))
    assert torch.equal(e, want), int((e != want).sum())
    assert not torch.equal(e, _oracle(dtype, b[0], st[4], n, _sched(DECAY, True, 2)))         # not the attempt count's decay
    assert not torch.equal(b[0][:n], st[0][:n]) and torch.equal(e[n:], st[4][n:])


# =====================================================================================================================
# 4. trainers against float64 arithmetic
# =====================================================================================================================
def _averaged_model(flat0, decay):
    """torch.optim.swa_utils.AveragedModel with the EMA multi_avg_fn over one flat parameter, None where torch has none"""
    swa = torch.optim.swa_utils
    if not hasattr(swa, "get_ema_multi_avg_fn"):
        return None, None
    holder = torch.nn.Module()
    holder.w = torch.nn.Parameter(flat0.clone())
    avg = swa.AveragedModel(holder, multi_avg_fn=swa.get_ema_multi_avg_fn(decay))
    avg.update_parameters(holder)                               # the first update copies: the average starts at the parameters
    return holder, avg


def _dataset():
    """eight synthetic phonon crystals, device-resident (step_dataset)"""
    if "ds" not in _DS:
        from dostransformer_amd import synth
        from dostransformer_amd.loader import DeviceDataset
        _DS["ds"] = DeviceDataset(synth.phonon_crystals(8, 91, torch.float32), DEV)
    return _DS["ds"]


@pytest.mark.parametrize("warmup", [False, True], ids=["fixed", "warmup"])
@pytest.mark.parametrize("name,mode", [("phonon", "eager"), ("phonon", "replay"), ("edos", "eager"), ("edos", "replay"),
                                       ("t64", "eager"), ("phonon", "graph"), ("phonon", "dataset")])
def test_trainer_average_against_float64_arithmetic(name, mode, warmup):
    """``dataset``: ``replay=True`` stepped through ``step_dataset`` (two selections, so two slots)."""
    o = ops()
    cfg = TG._cfg(name)
    tr, model = cfg.trainer("replay" if mode == "dataset" else mode, ema_decay=0.9, ema_warmup=warmup)
    fp = model.flat_params(cfg.g)
    dtype = fp.flat.dtype
    assert dtype == (torch.float64 if name == "t64" else torch.float32)
    eps = torch.finfo(dtype).eps
    ema64 = fp.flat.detach().double().cpu()
    mag = ema64.abs()
    holder, avg = _averaged_model(fp.flat.detach(), 0.9) if not warmup else (None, None)
    for k in range(1, 6):
        if mode == "dataset":
            tr.step_dataset(_dataset(), [0, 1, 2, 3] if k % 2 else [4, 5, 6, 7, 1])
        else:
            tr.step(cfg.g)
        torch.cuda.synchronize()
        assert tr._fp is fp and tr._ema_t0 == 0
        p = fp.flat.detach().double().cpu()
        d = o.ema_decay_at(0.9, warmup, k, dtype)               # the decay the kernel applies: d_t rounded once to T
        assert abs(d - _sched(0.9, warmup, k)) <= eps
        ema64 = ema64 + (p - ema64) * (1.0 - d)
        mag = torch.maximum(mag, torch.maximum(p.abs(), ema64.abs()))
        bar = k * 2.0 * eps * mag
        diff = (tr._ema.double().cpu() - ema64).abs()
        worst = float((diff / bar.clamp_min(1e-300)).max())
        print(f"ema[{name}-{mode}-{'warmup' if warmup else 'fixed'}] step {k}: worst |ema - float64| / (k x 2 eps max(|p|, |ema|)) = {worst:.3g}")
        assert bool((diff <= bar).all()), (k, worst)
        if avg is not None:
            with torch.no_grad():
                holder.w.copy_(fp.flat)
            avg.update_parameters(holder)
            da = (tr._ema.double() - avg.module.w.detach().double()).abs().cpu()
            worst = float((da / bar.clamp_min(1e-300)).max())
            print(f"ema[{name}-{mode}] step {k}: worst |ema - AveragedModel| / bar = {worst:.3g}")
            assert bool((da <= bar).all()), (k, worst)
    assert not torch.equal(tr._ema, fp.flat) and bool(torch.isfinite(tr._ema).all())
    if mode == "replay":
        assert tr.slot_hits >= 4
    tr.check()


# =====================================================================================================================
# 5. modes compose
# =====================================================================================================================
def _views(fp, buf):
    return {n: buf[o:o + fp.P[n].numel()] for n, o in zip(fp.names, fp.offsets)}


def _twins(name, prepare=None, **kw):
    """the same trainer with and without the average, same initial bits"""
    fam = PG._fam(name)
    out = []
    for extra in ({}, {"ema_decay": 0.9}):
        model = fam.model()
        k = dict(kw)
        if prepare is not None:
            k.update(prepare(model) or {})
        out.append((fam.trainer(model, "eager", lr=LR, weight_decay=WD, **k, **extra), model))
    return fam, out[0], out[1]


def _same_trained_bits(a, b):
    torch.cuda.synchronize()
    assert a._fp.names == b._fp.names and a._fp.n_train == b._fp.n_train
    assert torch.equal(a._fp.flat, b._fp.flat) and torch.equal(a._m, b._m) and torch.equal(a._v, b._v)


@pytest.mark.parametrize("name", ["phonon", "t64"])
def test_average_with_max_grad_norm(name):
    fam = PG._fam(name)
    probe = fam.trainer(fam.model(), "eager", lr=0.0, weight_decay=0.0, max_grad_norm=1e30)
    probe.step(fam.g)
    fam, (plain, _), (tr, _) = _twins(name, max_grad_norm=0.5 * float(probe.grad_norm))
    clips = []
    for _ in range(3):
        plain.step(fam.g)
        tr.step(fam.g)
        clips.append(float(tr.guard_report().clip))
    _same_trained_bits(plain, tr)
    assert tr.guard_report().applied == 3 and clips[0] < 1.0    # (the first step's norm is the probe's: clipped to half)
    assert not torch.equal(tr._ema, tr._fp.flat)


@pytest.mark.parametrize("name", ["phonon", "t64"])
def test_average_with_a_no_decay_group(name):
    from dostransformer_amd import param_groups as pg
    fam, (plain, _), (tr, _) = _twins(name, prepare=lambda m: {"param_groups": [{"params": pg.no_decay(m), "weight_decay": 0.0}]})
    for _ in range(3):
        plain.step(fam.g)
        tr.step(fam.g)
    _same_trained_bits(plain, tr)
    assert tr.param_groups is not None and not torch.equal(tr._ema, tr._fp.flat)


@pytest.mark.parametrize("name", ["phonon", "t64"])
def test_average_with_frozen_parameters_and_a_freeze_in_mid_run(name):
    """freeze("GN_encoder") in front of the first step: the trained parameters are bitwise those without the average, a frozen
    parameter's average IS the parameter.  freeze("GN_decoder.") after two steps: the average follows the new layout by name -
    the step behind it is, bit for bit, the oracle's on the re-homed average."""
    fam, (plain, pm), (tr, model) = _twins(name, prepare=lambda m: m.freeze("GN_encoder") and None)
    for _ in range(2):
        plain.step(fam.g)
        tr.step(fam.g)
    _same_trained_bits(plain, tr)
    fp = tr._fp
    frozen = sorted(fp.frozen)
    assert frozen and all(n.startswith("GN_encoder") for n in frozen) and fp.n_train < fp.total
    ev = _views(fp, tr._ema)
    for n in frozen:
        assert torch.equal(ev[n], fp.P[n].reshape(-1)), n
    assert any(not torch.equal(ev[n], fp.P[n].reshape(-1)) for n in fp.trainable_names())
    before = {n: t.clone() for n, t in ev.items()}
    for m in (pm, model):
        m.freeze("GN_decoder.")
    assert model._flat is not fp
    plain.step(fam.g)
    tr.step(fam.g)
    _same_trained_bits(plain, tr)
    fp2 = tr._fp
    assert fp2 is model._flat and fp2.n_train < fp.n_train and tr._ema_t0 == 0
    rehomed = torch.zeros_like(fp2.flat)
    for n, t in _views(fp2, rehomed).items():
        t.copy_(before[n])
    f32 = fp2.flat.dtype == torch.float32
    d = _sched(0.9, True, 3)
    want = _oracle(fp2.flat.dtype, fp2.flat[:fp2.n_train].clone(), rehomed[:fp2.n_train].clone(), fp2.n_train, d)
    assert torch.equal(tr._ema[:fp2.n_train], want)
    ev2 = _views(fp2, tr._ema)
    for n in fp2.frozen:                                        # frozen now: the average stays what it was when they froze
        assert torch.equal(ev2[n], before[n]), n
    assert any(n.startswith("GN_decoder.") for n in fp2.frozen) and f32 == (name == "phonon")


# =====================================================================================================================
# 6. evaluating under the average
# =====================================================================================================================
@pytest.mark.parametrize("name", ["phonon", "t64"])
def test_recorded_predictor_sees_the_average_inside_the_block(name):
    from dostransformer_amd._lib import DosxError
    from dostransformer_amd.predict import Predictor, Predictor64
    cfg = TG._cfg(name)
    tr, model = cfg.trainer("replay" if name == "phonon" else "eager", ema_decay=0.9, ema_warmup=False)
    for _ in range(3):
        tr.step(cfg.g)
    mk = (lambda m: Predictor(m, per_crystal_keys=True)) if name == "phonon" else Predictor64
    pred = mk(model)
    own = [t.clone() for t in pred(cfg.g)]                      # recorded here, BEFORE the block, on the trained weights
    torch.cuda.synchronize()
    flat = tr._fp.flat.clone()
    avg = tr._ema.clone()
    assert pred.slot_misses == 1 and not torch.equal(flat, avg)
    sd = tr.ema_state_dict()
    with tr.ema_weights() as same:
        assert same is tr
        inside = [t.clone() for t in pred(cfg.g)]
        torch.cuda.synchronize()
        assert torch.equal(tr._fp.flat, avg) and torch.equal(tr._ema, flat)
        for k, v in model.state_dict().items():                 # everything that reads the model sees the average
            assert torch.equal(v.detach().cpu(), sd[k]), k
        assert {k: v for k, v in tr.ema_state_dict().items()}.keys() == sd.keys()
        for what in (lambda: tr.step(cfg.g), lambda: tr.forward_backward(cfg.g), tr.optimizer_step, tr.state_dict):
            with pytest.raises(DosxError, match=r"inside `with trainer\.ema_weights\(\):`"):
                what()
        with pytest.raises(DosxError, match="does not nest"):
            with tr.ema_weights():
                pass
    torch.cuda.synchronize()
    assert pred.slot_misses == 1 and pred.slot_hits == 1        # nothing was re-recorded
    assert torch.equal(tr._fp.flat, flat) and torch.equal(tr._ema, avg)
    fresh = cfg.model()
    fresh.load_state_dict(sd)
    want = mk(fresh)(cfg.g)
    torch.cuda.synchronize()
    assert len(inside) == len(want) == len(own)
    for a, b in zip(inside, want):
        assert torch.equal(a, b)
    assert any(not torch.equal(a, b) for a, b in zip(inside, own))
    # the body raises: the trained weights still come back
    with pytest.raises(ZeroDivisionError):
        with tr.ema_weights():
            assert torch.equal(tr._fp.flat, avg)
            1 / 0
    torch.cuda.synchronize()
    assert torch.equal(tr._fp.flat, flat) and torch.equal(tr._ema, avg) and tr._ema_block is False
    again = pred(cfg.g)
    torch.cuda.synchronize()
    for a, b in zip(again, own):
        assert torch.equal(a, b)
    tr.step(cfg.g)                                              # and the run goes on
    tr.check()


def test_freeze_inside_the_block_is_reported_and_undone():
    from dostransformer_amd._lib import DosxError
    cfg = TG._cfg("phonon")
    tr, model = cfg.trainer("eager", ema_decay=0.9, ema_warmup=False)
    for _ in range(2):
        tr.step(cfg.g)
    torch.cuda.synchronize()
    before = {n: t.clone() for n, t in tr._fp.P.items()}
    with pytest.raises(DosxError, match="laid out anew"):
        with tr.ema_weights():
            model.freeze("GN_encoder.")
            with pytest.raises(DosxError, match=r"inside `with trainer\.ema_weights\(\):`"):
                tr._state(model.flat_params())
    for n, t in model._flat.P.items():                          # the trained values are back under the new layout
        assert torch.equal(t, before[n]), n
    tr.step(cfg.g)
    assert tr._fp is model._flat and tr._fp.frozen


# =====================================================================================================================
# 7. resume
# =====================================================================================================================
@pytest.mark.parametrize("name,mode", [("phonon", "replay"), ("t64", "eager")])
def test_trainer_with_average_resumes_bitwise(name, mode, tmp_path):
    from dostransformer_amd import checkpoint
    cfg = TG._cfg(name)
    a, _ = cfg.trainer(mode, ema_decay=0.9)
    for _ in range(4):
        a.step(cfg.g)
    b, mb = cfg.trainer(mode, ema_decay=0.9)
    for _ in range(2):
        b.step(cfg.g)
    path = str(tmp_path / "ckpt.pt")
    checkpoint.save(path, mb, b)
    c, mc = cfg.trainer(mode, ema_decay=0.5, ema_warmup=False)                # (the file's hyper-parameters win)
    with torch.no_grad():
        for p in mc.parameters():
            p.add_(1.0)
    checkpoint.load(path, mc, c)
    assert (c.ema_decay, c.ema_warmup, c._ema_t0, c.step_count) == (0.9, True, 0, 2)
    for _ in range(2):
        c.step(cfg.g)
    torch.cuda.synchronize()
    assert a._fp.names == c._fp.names
    assert torch.equal(a._ema, c._ema) and torch.equal(a._fp.flat, c._fp.flat)
    assert torch.equal(a._m, c._m) and torch.equal(a._v, c._v)
    assert not torch.equal(a._ema, a._fp.flat)


# =====================================================================================================================
# 8. swap_buffers
# =====================================================================================================================
def test_swap_buffers_exchanges_exactly():
    from dostransformer_amd import _abi
    o = ops()
    sweep = _abi.DOSX_SWAP_MAX_BLOCKS * _abi.DOSX_SWAP_THREADS * 16
    def one(nbytes):
        n = nbytes // 4
        gen = torch.Generator().manual_seed(nbytes % 1000)
        a0 = torch.randint(-2 ** 31, 2 ** 31 - 1, (n + 4,), generator=gen, dtype=torch.int64).to(torch.int32).to(DEV)
        b0 = torch.randint(-2 ** 31, 2 ** 31 - 1, (n + 4,), generator=gen, dtype=torch.int64).to(torch.int32).to(DEV)
        a, b = a0.clone(), b0.clone()
        o.swap_buffers(a, b, n)
        assert torch.equal(a[:n], b0[:n]) and torch.equal(b[:n], a0[:n]), nbytes
        assert torch.equal(a[n:], a0[n:]) and torch.equal(b[n:], b0[n:]), (nbytes, "sentinel")
        o.swap_buffers(a, b, n)
        assert torch.equal(a, a0) and torch.equal(b, b0), (nbytes, "twice is the identity")

    for nbytes in (16, 48, sweep + 16):                         # one vector, three, the grid-stride second trip
        with _own_pool(nbytes // 4):
            one(nbytes)
    x = torch.arange(8, dtype=torch.float64, device=DEV)
    y = -x.clone()
    o.swap_buffers(x, y)                                        # blind to the element type; default: all of it
    assert torch.equal(y, torch.arange(8, dtype=torch.float64, device=DEV)) and torch.equal(x, -y)
    with pytest.raises(ValueError):
        o.swap_buffers(x, y, 9)
    with pytest.raises(TypeError):
        o.swap_buffers(x, y.float())
# =====================================================================================================================
# 1. p, m, v bit for bit; the average against the kernel from before (every size) - defined last: the sweep-sized cases run
#    behind everything that leaves small allocations alive (the shared trainer configurations)
# =====================================================================================================================
@pytest.mark.parametrize("step", [1, 7])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_launch_with_average_leaves_p_m_v_of_the_launch_without(dtype, form, step):
    for n, ids, groups in _cases(dtype, form):
        with _own_pool(n):
            _one_size(dtype, form, step, n, ids, groups)


@contextlib.contextmanager
def _own_pool(n):
    """The sweep-sized cases allocate in a memory pool of their own, which goes back to the driver with them: they leave no
    cached blocks behind for the allocations of later tests to be carved from.  (Kernels elsewhere in the suite need operands
    that were allocated one after the other to lie within 2 GiB of each other - dosx_mlp_ln_fwd's two weight matrices.)"""
    if n <= 1 << 17:
        yield
        return
    pool = torch.cuda.MemPool()
    try:
        with torch.cuda.use_mem_pool(pool):
            yield
    finally:
        torch.cuda.synchronize()
        del pool


def _one_size(dtype, form, step, n, ids, groups):
    o = ops()
    t0 = 0 if step == 1 else 5                                  # t = 1, 2: inside the warm-up
    st = _state(dtype, n, step)
    rec = None
    if "guarded" in form:                                       # a record that clips: the guarded arithmetic is in play
        rec, ws = o.guard_buffers(DEV)
        norm = float(torch.linalg.vector_norm(st[1][:n], dtype=torch.float64))
        o.grad_guard(st[1], n, rec, ws, 0.5 * norm, LR, B1, B2, step)
    a, b = [t.clone() for t in st[:4]], [t.clone() for t in st[:4]]
    e = st[4].clone()
    _launch(dtype, form, a, n, step, rec, ids, groups, gs=0.37)
    _launch(dtype, form, b, n, step, rec, ids, groups, ema=(e, DECAY, True, t0), gs=0.37)
    if rec is not None:
        r = o.guard_read(rec)
        assert r.skip == 0 and r.t == step and r.clip < 1.0
    for name, x, y, x0 in zip("pgmv", a, b, st):
        assert torch.equal(x, y), (n, name, int((x != y).sum()))
        assert torch.equal(y[n:], x0[n:]), (n, name, "sentinel")
    assert torch.equal(b[1], st[1]) and not torch.equal(b[0][:n], st[0][:n])
    assert torch.equal(e[n:], st[4][n:]), (n, "ema sentinel")
    del a
    want = _oracle(dtype, b[0], st[4], n, _sched(DECAY, True, step - t0))
    assert torch.equal(e, want), (n, "ema", int((e != want).sum()))
    assert not torch.equal(e[:n], st[4][:n])


