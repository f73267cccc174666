"""The guarded optimizer step's kernels on a real MI355X (csrc/step_guard.hip: dosx_grad_guard_f32 / _f64; csrc/adamw.hip:
dosx_adamw_guarded, dosx_adamw_guarded_f64), each called directly, for fp32 and float64 gradients.

Every gradient buffer is n + 8 long with NaN behind n: a kernel that read past n would count a non-finite element.  The
statistics are held to a long-double reference within bounds counted from the kernel's own summation order (section 1), the
non-finite findings are exact, the guarded AdamW with nothing tripped and no clipping is BITWISE the unguarded kernel, with a
coefficient < 1 it keeps the per-step bounds of the unguarded kernels' tests (tests/test_gpu_tail.py section C,
tests/test_gpu_train64.py section 2), and a skipped step changes nothing and does not advance AdamW's time."""
import math

import numpy as np
import pytest
import torch

from tests import test_gpu_tail as T32
from tests import test_gpu_train64 as T64
from tests.gpu_util import DEV, bound_ratio, ops

pytestmark = pytest.mark.gpu

L = np.longdouble
NAN, INF = float("nan"), float("inf")
U64 = 2.0 ** -53
THREADS, MAX_BLOCKS = 256, 256                             # DOSX_GUARD_THREADS, DOSX_GUARD_MAX_BLOCKS (asserted below)
DTYPES = [torch.float32, torch.float64]
IDS = ["f32", "f64"]
LR, WD = 1e-3, 1e-2


def _per(dtype):
    return 4 if dtype == torch.float32 else 2


def _sweep(dtype):
    """elements one sweep of the capped grid covers"""
    return MAX_BLOCKS * THREADS * _per(dtype)


def _blocks(n, dtype):
    return min(max(-(-(n // _per(dtype)) // THREADS), 1), MAX_BLOCKS)


# =====================================================================================================================
# 1. the statistics
# =====================================================================================================================
# sumsq, u = 2^-53 for BOTH dtypes (the accumulator is a double; the square of a float is exact in it, the square of a double
# is fused into the addition: fma(x, x, sum), one rounding per element).  Every term is >= 0, so each rounding is relative to a
# partial sum <= sumsq and the error is <= depth * u * sumsq, depth = the longest chain of additions an element goes through:
#   a thread's own elements     PER per 16-byte vector x ceil(nvec / (blocks * 256)) vectors, + 1 for a tail element
#   the workgroup's tree        8 levels (256 threads)
#   the last arriver            ceil(blocks / 256) slots per thread (1: the grid is capped at 256 workgroups), + 8 levels
# norm = sqrt(sumsq): half the relative error of sumsq + the (correctly rounded) square root's own half ulp: depth / 2 + 1.
# clip = max_norm / (norm + 1e-6): the norm's error, the sum, the division: depth / 2 + 3.
def _depth(n, dtype):
    per, nb = _per(dtype), _blocks(n, dtype)
    return per * -(-(n // per) // (nb * THREADS)) + 1 + 8 + -(-nb // THREADS) + 8


def _gradient(n, dtype, seed):
    """n + 8 elements, NaN behind n: |g| over 1e-8 .. 100, with exact zeros, 1e-30 and a subnormal of the dtype among them."""
    gen = torch.Generator().manual_seed(seed)
    u = torch.rand(n, generator=gen, dtype=torch.float64)
    g = torch.randn(n, generator=gen, dtype=torch.float64) * 10.0 ** (u * 10 - 8)
    perm = torch.randperm(n, generator=gen)
    k = max(1, min(100, n // 8))
    if n >= 8:
        g[perm[:k]] = 0.0
        g[perm[k:2 * k]] = 1e-30
        g[perm[2 * k:3 * k]] = 1e-40 if dtype == torch.float32 else 1e-310
    buf = torch.full((n + 8,), NAN, dtype=dtype, device=DEV)
    buf[:n] = g.to(dtype).to(DEV)
    return buf


def _guard(g, n, max_norm=None, step=1, status=None, bufs=None, lr=LR):
    o = ops()
    rec, ws = bufs if bufs is not None else o.guard_buffers(DEV)
    o.grad_guard(g, n, rec, ws, max_norm, lr, 0.9, 0.999, step, status)
    return o.guard_read(rec), rec, ws


def _sumsq_ref(g, n, finite_only=False):
    x = g[:n].cpu().numpy().astype(L)
    if finite_only:
        x = x[np.isfinite(x)]
    return np.sum(x * x)


def _sizes(dtype):
    s, per = _sweep(dtype), _per(dtype)
    return [1, 3, 4, 5, 255, 1025, s - 1, s + THREADS * per * 3 + per - 1, 2 * s + 5]


@pytest.mark.parametrize("k", range(9))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_grad_norm_against_long_double(dtype, k):
    """sumsq / norm within the counted bound at: one element, the scalar tail alone, one vector, vector + tail, a partial
    workgroup, 256 k + 1, one sweep of the capped grid - 1, one sweep + a partial sweep + tail, two sweeps + 5; nothing flagged
    (zeros, 1e-30 and subnormals are finite); two runs give identical bits."""
    from dostransformer_amd import _abi
    assert (_abi.DOSX_GUARD_THREADS, _abi.DOSX_GUARD_MAX_BLOCKS) == (THREADS, MAX_BLOCKS)
    n = _sizes(dtype)[k]
    o = ops()
    assert o._lib.load().dosx_grad_guard_blocks(n, 4 if dtype == torch.float32 else 8) == _blocks(n, dtype)
    g = _gradient(n, dtype, 100 + k)
    g0 = g.clone()
    r, rec, ws = _guard(g, n)
    first = rec.clone()
    r2, _, _ = _guard(g, n, bufs=(rec, ws))
    ref = _sumsq_ref(g, n)
    assert ref > 0
    d = _depth(n, dtype)
    e_sum = float(abs(L(r.sumsq) - ref) / (L(d * U64) * ref))
    e_norm = float(abs(L(r.norm) - np.sqrt(ref)) / (L((d / 2 + 1) * U64) * np.sqrt(ref)))
    print(f"grad_guard[{dtype}, n={n}]: depth {d}, sumsq error / bound = {e_sum:.3g}, norm error / bound = {e_norm:.3g}")
    assert e_sum <= 1.0 and e_norm <= 1.0
    assert (r.n_bad, r.first_bad, r.skip, r.reason, r.clip) == (0, -1, 0, 0, 1.0)
    assert (r.applied, r.skipped, r.t) == (1, 0, 1) and (r2.applied, r2.skipped) == (2, 0)
    assert torch.equal(first.view(torch.int64)[:8], rec.view(torch.int64)[:8])                    # identical bits, run to run
    assert torch.equal(g[:n], g0[:n]) and bool(torch.isnan(g[n:]).all())
    assert int(ws[0]) == 0                                                                        # the ticket counter is back at zero


def _plant_cases(dtype):
    s, per = _sweep(dtype), _per(dtype)
    n = 2 * s + 5                                       # n % per == 1: the last element is the scalar tail
    nb = MAX_BLOCKS
    last_wg = (nb * THREADS + (nb - 1) * THREADS + 17) * per + 1       # second sweep, last workgroup
    return [(1, [0]), (5, [4]), (5, [0, 4]), (1025, [0]), (1025, [1024]), (1025, [3, 700, 1024]), (n, [n - 1]), (n, [last_wg]),
            (n, [last_wg, n - 1]), (n, [0, last_wg]), (s + THREADS * per * 3 + per - 1, [s + 5, s + THREADS * per * 3 + per - 2])]


@pytest.mark.parametrize("k", range(11))
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_non_finite_elements_are_counted_and_located(dtype, k):
    """NaN, +inf and -inf planted at index 0, at n - 1, in the scalar tail, in the last workgroup of a multi-sweep size: n_bad
    and first_bad exact, skip = 1 with the non-finite reason alone, sumsq still the sum over the finite elements."""
    from dostransformer_amd import _abi
    n, where = _plant_cases(dtype)[k]
    assert all(0 <= i < n for i in where) and (n <= 5 or n % _per(dtype) != 0)
    g = _gradient(n, dtype, 200 + k)
    for j, i in enumerate(where):
        g[i] = (NAN, INF, -INF)[(j + k) % 3]
    r, rec, _ = _guard(g, n, max_norm=1.0, step=7)
    assert (r.n_bad, r.first_bad, r.skip, r.reason) == (len(where), min(where), 1, _abi.DOSX_GUARD_NONFINITE)
    assert (r.applied, r.skipped, r.first_skip_step, r.first_skip_reason, r.first_skip_bad) == (0, 1, 7, 1, min(where))
    ref = _sumsq_ref(g, n, finite_only=True)
    assert abs(L(r.sumsq) - ref) <= L(_depth(n, dtype) * U64) * ref and math.isfinite(r.norm) and math.isfinite(r.clip)


def test_float64_overflow_of_the_sum_is_a_reason_to_skip():
    """One element of 1e200: finite, its square is not - the overflow reason, no element flagged."""
    from dostransformer_amd import _abi
    n = 1025
    g = _gradient(n, torch.float64, 231)
    g[600] = 1e200
    r, _, _ = _guard(g, n, max_norm=1.0)
    assert (r.n_bad, r.first_bad, r.skip, r.reason) == (0, -1, 1, _abi.DOSX_GUARD_OVERFLOW) and r.sumsq == INF
    assert (r.first_skip_step, r.first_skip_reason, r.first_skip_bad) == (1, _abi.DOSX_GUARD_OVERFLOW, -1)
    g[600] = 1e150                                       # 1e300: fits
    r, _, _ = _guard(g, n, max_norm=1.0)
    assert (r.skip, r.reason) == (0, 0) and abs(r.norm / 1e150 - 1) < 1e-12


@pytest.mark.parametrize("n", [5, 1025, 300001])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_clip_coefficient(dtype, n):
    """No max_norm, and max_norm / (norm + 1e-6) >= 1 (2 x norm, norm + 1e-5, 1e30, inf): exactly 1.0.  Below that - 0.999, 0.5,
    1e-3 and 0 times the norm - torch's max_norm / (norm + 1e-6) against long double within depth / 2 + 3 roundings."""
    g = _gradient(n, dtype, 240 + n % 7)
    norm = np.sqrt(_sumsq_ref(g, n))
    r, _, _ = _guard(g, n)
    assert r.clip == 1.0
    for mx in (2.0 * r.norm, r.norm + 1e-5, 1e30, INF):
        assert _guard(g, n, max_norm=mx)[0].clip == 1.0, mx
    for frac in (0.999, 0.5, 1e-3, 0.0):
        mx = frac * float(norm)
        rr, _, _ = _guard(g, n, max_norm=mx)
        ref = L(mx) / (norm + L(1e-6))
        assert ref < 1 and rr.skip == 0
        bound = L((_depth(n, dtype) / 2 + 3) * U64) * ref
        print(f"clip[{dtype}, n={n}, {frac:g} x norm]: error / bound = {float(abs(L(rr.clip) - ref) / bound) if bound else 0.0:.3g}")
        assert abs(L(rr.clip) - ref) <= bound and rr.clip < 1.0


# =====================================================================================================================
# 2. the guarded AdamW
# =====================================================================================================================
def _state(dtype, n, step, seed):
    """(p, g, m, v) of the unguarded kernels' tests, the gradient's sentinel tail replaced by NaN (n + 8 elements at least)."""
    p, g, m, v = (T32._adam_state if dtype == torch.float32 else T64._adam_state)(n, step, seed)
    g[n:] = NAN
    return p, g, m, v


def _sent(dtype):
    return T32.SENT if dtype == torch.float32 else T64.SENT


def _unguarded(dtype, p, g, m, v, n, step, lr=LR, wd=WD):
    o = ops()
    if dtype == torch.float32:
        o.adamw(p, g, m, v, n, lr, 0.9, 0.999, 1e-8, wd, step, 1.0)
    else:
        o.adamw64(p, g, m, v, n, lr, 0.9, 0.999, 1e-8, wd, step)


def _guarded(dtype, p, g, m, v, n, step, bufs, max_norm=None, lr=LR, wd=WD, status=None):
    o = ops()
    rec, ws = bufs
    o.grad_guard(g, n, rec, ws, max_norm, lr, 0.9, 0.999, step, status)
    (o.adamw_guarded if dtype == torch.float32 else o.adamw64_guarded)(p, g, m, v, n, lr, 0.9, 0.999, 1e-8, wd, rec)


ADAM_N = {torch.float32: [1, 2, 3, 4, 5, 1003, 1024, T32.ADAM_CAP - 1, T32.ADAM_CAP + 4 * 256 * 3 + 3, 2 * T32.ADAM_CAP + 5],
          torch.float64: [1, 2, 3, 255, 1025, 2 * T64.ADAM64_SWEEP + 2 * 256 * 3 + 1]}


@pytest.mark.parametrize("step", [1, 1000])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_guarded_adamw_without_a_trip_is_bitwise_the_unguarded_kernel(dtype, step):
    """Guard on, nothing non-finite, no max_norm and a max_norm above the norm: p, m, v are bit for bit those of ops.adamw(...,
    grad_scale=1.0) / ops.adamw64 on the same inputs, at the sizes of the unguarded kernels' tests."""
    o = ops()
    for n in ADAM_N[dtype]:
        s0 = _state(dtype, n, step, 400 + n % 1000)
        for mx in (None, 1e30):
            a, b = [t.clone() for t in s0], [t.clone() for t in s0]
            _unguarded(dtype, *a, n, step)
            _guarded(dtype, *b, n, step, o.guard_buffers(DEV), max_norm=mx)
            for name, x, y in zip("pgmv", a, b):
                assert torch.equal(x[:n], y[:n]), (n, mx, name)
            for t in (b[0], b[2], b[3]):
                assert bool((t[n:] == _sent(dtype)).all()), (n, "written behind n")
            assert bool(torch.isnan(b[1][n:]).all())


def _adam_ref64(p, g, m, v, t, clip, lr, wd):
    """tests/test_gpu_train64.py's long-double reference on g * clip (clip: the record's double, the product in long double)"""
    decay, step_size, bc2_sqrt = 1 - lr * wd, lr / (1 - 0.9 ** t), math.sqrt(1 - 0.999 ** t)
    p, g, m, v = (x.cpu().numpy().astype(L) for x in (p, g, m, v))
    g = g * L(clip)
    m1 = m + (g - m) * L(1 - 0.9)
    v1 = v * L(0.999) + L(1 - 0.999) * g * g
    denom = np.sqrt(v1) / L(bc2_sqrt) + L(1e-8)
    p2 = p * L(decay) - L(step_size) * (m1 / denom)
    return (p2, m1, v1), (np.abs(p) + L(step_size) * (np.abs(m) + np.abs(g)) / denom, np.abs(m) + np.abs(g), v1)


# float64 with a coefficient: g clip is one more rounding on g wherever g enters - m' 4 + 1, v' 6 + 2 (g twice), p' 16 + 1 (m') + 1
# (denom: half of v') = 18.  fp32: the kernel's gr = g gs already is section C's first line (1 rounding, counted in 4 / 6 / 16); the
# reference multiplies by the coefficient the kernel applied - the record's clip rounded to fp32, as dosx_adamw's grad_scale is -
# and the coefficient itself is held to long double by test_clip_coefficient, so its own rounding adds nothing here.
C64_CLIP_M, C64_CLIP_V, C64_CLIP_P = T64.C_ADAM_M + 1, T64.C_ADAM_V + 2, T64.C_ADAM_P + 2


def _check_step(dtype, n, state, state0, t, clip, tag, lr=LR, wd=WD):
    """p, m, v of `state` against one reference step at AdamW time t from `state0` with the coefficient `clip`"""
    p, g, m, v = state
    p0, g0, m0, v0 = state0
    if dtype == torch.float32:
        (p1, m1, v1), (sp, sm, sv) = T32._adam_ref(p0[:n], g0[:n], m0[:n], v0[:n], t, lr, wd, float(np.float32(clip)))
        assert bound_ratio(m[:n], m1, sm, T32.C_ADAM_M, tag + ".m") <= 1.0
        assert bound_ratio(v[:n], v1, sv, T32.C_ADAM_V, tag + ".v") <= 1.0
        assert bound_ratio(p[:n], p1, sp, T32.C_ADAM_P, tag + ".p") <= 1.0
    else:
        refs, scales = _adam_ref64(p0[:n], g0[:n], m0[:n], v0[:n], t, clip, lr, wd)
        for name, got, ref, sc, c in zip("pmv", (p, m, v), refs, scales, (C64_CLIP_P, C64_CLIP_M, C64_CLIP_V)):
            err = np.abs(got[:n].cpu().numpy().astype(L) - ref)
            bound = L(c * U64) * sc
            worst = float(np.max(err / np.maximum(bound, np.finfo(L).tiny)))
            print(f"bound[{tag}.{name}]: worst error / (c={c} x 2^-53 x scale) = {worst:.3g}")
            assert bool(np.all(err <= bound)), (tag, name, worst)
    for x in (p, m, v):
        assert bool((x[n:] == _sent(dtype)).all()), tag + ": written behind n"
    assert torch.equal(g[:n], g0[:n]) and bool(torch.isnan(g[n:]).all()), tag + ": gradient changed"


@pytest.mark.parametrize("step", [1, 1000])
@pytest.mark.parametrize("n", [1, 3, 5, 1003, 1025, 300001])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_guarded_adamw_with_a_coefficient_below_one(dtype, n, step):
    """max_norm = 0.37 x the gradient's norm: every element is updated with g x clip, clip the record's; g itself is not written."""
    o = ops()
    st = _state(dtype, n, step, 500 + n % 1000)
    st0 = [t.clone() for t in st]
    norm = np.sqrt(_sumsq_ref(st[1], n))
    mx = 0.37 * float(norm)
    bufs = o.guard_buffers(DEV)
    _guarded(dtype, *st, n, step, bufs, max_norm=mx)
    r = o.guard_read(bufs[0])
    want = L(mx) / (norm + L(1e-6))                      # (a small norm sits next to the 1e-6: the coefficient is then below 0.37)
    assert abs(L(r.clip) - want) <= L((_depth(n, dtype) / 2 + 3) * U64) * want and r.clip < 0.3701 and r.skip == 0 and r.t == step
    _check_step(dtype, n, st, st0, step, r.clip, f"adamw_guarded[{dtype},n{n},step{step}]")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_trajectory_with_a_skipped_step(dtype):
    """Five steps at n = 1003 with clipping, the third gradient poisoned (a NaN and an inf).  The skipped step leaves p, m, v
    bitwise, the sentinels intact and g unchanged; AdamW's time does not advance (t = step - skipped, recomputed on the device).
    fp32: every applied step within section C's bounds from the kernel's own state.  float64: the end state against
    torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW in float64 that saw the four good gradients only, at the bars of
    test_adamw_f64_three_steps_against_torch_adamw (1e-9 on p, 1e-12 relative on the moments)."""
    o = ops()
    n = 1003
    p, _, m, v = _state(dtype, n, 1, 601)
    bufs = o.guard_buffers(DEV)
    grads = [_state(dtype, n, 1, 610 + s)[1] for s in range(5)]
    grads[2][17], grads[2][900] = NAN, INF
    norms = [float(np.sqrt(_sumsq_ref(g, n))) for i, g in enumerate(grads) if i != 2]
    mx = float(np.median(norms))                                   # some steps clip, some do not
    ref = torch.nn.Parameter(p[:n].double().cpu().clone())
    opt = torch.optim.AdamW([ref], lr=LR, betas=(0.9, 0.999), eps=1e-8, weight_decay=WD)
    clipped = 0
    for s, g in enumerate(grads):
        st0 = [t.clone() for t in (p, g, m, v)]
        _guarded(dtype, p, g, m, v, n, s + 1, bufs, max_norm=mx)
        r = o.guard_read(bufs[0])
        if s == 2:
            assert (r.skip, r.n_bad, r.first_bad, r.skipped, r.applied, r.first_skip_step) == (1, 2, 17, 1, 2, 3)
            for x, x0 in zip((p, m, v), (st0[0], st0[2], st0[3])):
                assert torch.equal(x, x0)                                       # bitwise, sentinels included
            bits = torch.int32 if dtype == torch.float32 else torch.int64
            assert torch.equal(g.view(bits), st0[1].view(bits))                 # g unchanged, the poison included
            continue
        t = s + 1 - (1 if s > 2 else 0)
        assert (r.skip, r.t, r.skipped) == (0, t, 1 if s > 2 else 0)
        clipped += r.clip < 1.0
        _check_step(dtype, n, (p, g, m, v), st0, t, r.clip, f"trajectory[{dtype},step{s + 1},t{t}]")
        ref.grad = g[:n].double().cpu().clone()
        torch.nn.utils.clip_grad_norm_([ref], mx)
        opt.step()
    assert 0 < clipped < 4
    if dtype == torch.float64:
        state = opt.state[ref]
        e_p = float((p[:n].cpu() - ref.detach()).abs().max())
        e_m, e_v = T64._relmax(m[:n].cpu(), state["exp_avg"]), T64._relmax(v[:n].cpu(), state["exp_avg_sq"])
        print(f"trajectory[f64] against torch: p {e_p:.3g} (1e-9), m {e_m:.3g}, v {e_v:.3g} (1e-12)")
        assert e_p <= 1e-9 and e_m <= 1e-12 and e_v <= 1e-12


def test_a_reported_stall_skips_the_step_until_the_check_has_cleared_it():
    """ops.exchange_selftest files a stall report (no exchange stalls): the next guarded steps are skipped with the stall reason,
    ops.check_exchanges raises and clears, the step after that applies."""
    from dostransformer_amd import _abi
    from dostransformer_amd._lib import DosxError
    o = ops()
    dtype, n = torch.float32, 1003
    st = _state(dtype, n, 1, 701)
    bufs = o.guard_buffers(DEV)
    addr = o.exchange_status_address(DEV)
    assert addr != 0 and addr % 4 == 0 and o.exchange_status_address(DEV) == addr
    assert o.exchange_status(DEV)[0] == 0
    try:
        o.exchange_selftest(DEV, _abi.DOSX_EXCHANGE_KERNEL_ENC_CS_FWD, 5)
        st0 = [t.clone() for t in st]
        for attempt in (1, 2):
            _guarded(dtype, *st, n, attempt, bufs, max_norm=1.0, status=addr)
            r = o.guard_read(bufs[0])
            assert (r.skip, r.reason, r.n_bad, r.skipped, r.applied) == (1, _abi.DOSX_GUARD_STALLED, 0, attempt, 0)
            assert (r.first_skip_step, r.first_skip_reason, r.first_skip_bad) == (1, _abi.DOSX_GUARD_STALLED, -1)
            for x, x0 in zip(st, st0):
                assert torch.equal(x[:n], x0[:n])
        _guarded(dtype, *[t.clone() for t in st], n, 3, o.guard_buffers(DEV), status=None)         # not handed the status: applies
        with pytest.raises(DosxError, match="enc_cs_fwd, tile 5"):
            o.check_exchanges(DEV)
        _guarded(dtype, *st, n, 3, bufs, status=addr)
        r = o.guard_read(bufs[0])
        assert (r.skip, r.reason, r.skipped, r.applied, r.t) == (0, 0, 2, 1, 1)
        _check_step(dtype, n, st, st0, 1, 1.0, "after_the_stall")
    finally:
        o.exchange_status(DEV, clear=True)
