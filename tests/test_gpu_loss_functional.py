"""dosx_loss_rows_fn / dosx_loss_rows_fn_f64 (csrc/loss_functional.hip) on a real MI355X: the per-crystal losses with a penalty on
K linear functionals of the DOS against float64 torch autograd of the definition in include/dosx.h, computed on the CPU on the
same rounded inputs and the same rounded table -

    u_k = sum_s fn_w[k,s] r_s,   h = (1 / K) sum_k e(u_k),   l_b = f(pg_b) + beta f(ps_b) + lam (h(pg_b) + beta h(ps_b)),
    loss[0] = sum_b w_b l_b / B_global

- and what holds bit for bit by construction: no table or lam == 0 (the weighted entry's kernels), appended all-zero rows, a zero
sample weight, a NaN confined to its crystal, run to run, and a crystal's numbers wherever it stands in whatever batch.

float64 is held to the project's bars (tests/test_gpu_loss_rows._judge): 1e-12 relative for loss and per_crystal, 1e-10 of the
row's largest entry for the gradient rows.

fp32 is judged element by element with tests/gpu_util.bound_ratio.  Every element's bar is the pointwise term's own bar
(tests/test_gpu_loss_weighted._judge_w's constants times its scales) PLUS the new term's bar PLUS one rounding of the result for
the final addition.  The new term's bar is counted from the kernel's summation order (the header comment of
csrc/loss_functional.hip), every rounding at most 2^-24 of the magnitude it acts on, n = ceil(S / 64):

  u_k, against A_k = sum_s |fn_w[k,s] r_s|:  the subtraction r = p - t (1), the product (1), n - 1 additions in the lane, 6
      levels of the wave reduction:                                                                      c_u = n + 7
  a gradient element, against G_s = coef lam / K sum_k |fn_w[k,s]| 2 A_k (SQ) or coef lam / K sum_k |fn_w[k,s]| (ABS):
      SQ  e'(u_k) = 2 u_k carries c_u (the doubling is exact), the product with fn_w[k,s] 1, the K - 1 additions over k:
                                                                                                          c_u + K
      ABS e'(u_k) = +-1 exactly (the inputs keep |u_k| >= 1e-4 A_k, far above c_u 2^-24 A_k), the products exact, K - 1
          additions (counted as K):                                                                       K
      and the coefficient coef lam / K: 1 / B_global (1), lam / K (1), their product (1), times the sum (1), + 1 with sample
      weights (w_b / B_global), + 1 for the second output (beta coef):                                    + 4 [+ 1] [+ 1]
  per_crystal, against lam / K (sum_k A_k^2 [+ beta ...]) (SQ) or lam / K (sum_k A_k [+ beta ...]) (ABS):
      SQ  u_k^2 carries 2 c_u + 1, K - 1 additions;  ABS |u_k| carries c_u, K - 1 additions;  then lam / K, beta h(ps), the sum
      of the two, the product with lam / K (4):                                       SQ 2 c_u + K + 4,   ABS c_u + K + 3
  loss[0]: every crystal's bar times w_b / B_global, + tests/test_gpu_loss_rows.c_total's own roundings of the final sum.

Contraction into fused multiply-adds removes roundings and never adds one, so the counts are upper bounds either way.

Inputs: uniform [0,1) predictions and targets (targets shifted down by 0.2 where the clamp is tested), every crystal drawn from
a seed of its own and redrawn alone (next sub-seed, at most 64 times) until on BOTH outputs every |u_k| >= 1e-4 A_k - ABS has a
kink there - and the pointwise margins of tests/test_gpu_loss_rows.py hold (no zero residual for MAE, none within 1e-6 delta of
Huber's branch point); asserted on the CPU before anything is judged.  No crystal and no k is left out of the judgement."""
import math

import pytest
import torch

from tests.gpu_util import DEV, bound_ratio
from tests.test_gpu_loss_rows import DELTA, DTYPES, KINDS, NAN, Out, _c, _elem_scale, _judge, _ops, _target, c_total, f32
from tests.test_gpu_loss_weighted import BETA, _bits, _f_w, _weights

pytestmark = pytest.mark.gpu

# S over the lane boundaries at B = 5 with one functional and with S of them; K one over / one under S at the 64 edge; B over the
# four-crystals-per-workgroup edge and the one-workgroup form's 256 at (S, K) = (51, 51).  (5, 512, 512) runs once, below.
SHAPES = sorted({(5, S, K) for S in (1, 63, 64, 65, 201) for K in (1, S)}) + [(5, 64, 65), (5, 65, 64)] + \
    [(B, 51, 51) for B in (1, 3, 4, 257)]
FKINDS = ["sq", "abs"]
TABLES = ["cumulative", "random"]
LAM = 0.5                              # exact in fp32
MARGIN = 1e-4


@pytest.fixture(scope="module", autouse=True)
def _own_memory_pool():
    """As tests/test_gpu_loss_weighted.py: this module allocates from a memory pool of its own, given back when it is done."""
    pool = torch.cuda.MemPool()
    with torch.cuda.use_mem_pool(pool):
        yield
    torch.cuda.synchronize()
    del pool


# ---- tables and inputs (all on the CPU; moved to the device once) ------------------------------------------------------------
def _table(which, K, S, dt, seed=0):
    """cumulative: row k is 0.25 on the bins below the k-th of K equal steps through the grid (K == S: the lower triangle);
    random: dense uniform (-1, 1).  Rounded to dt; returned on the CPU in float64 (what the kernel reads, exactly)."""
    if which == "cumulative":
        t = torch.zeros(K, S, dtype=torch.float64)
        for k in range(K):
            t[k, :max(1, ((k + 1) * S + K - 1) // K)] = 0.25
    else:
        g = torch.Generator().manual_seed(4242 + 7 * K + S + seed)
        t = 2.0 * torch.rand(K, S, generator=g, dtype=torch.float64) - 1.0
    return t.to(dt).double()


def _margins_hold(p, t, tab):
    """one crystal's output p [S] against its target t: every |u_k| >= MARGIN A_k, no zero residual, none near Huber's branch"""
    r = p - t
    u, A = tab @ r, tab.abs() @ r.abs()
    ra = r.abs()
    return bool((u.abs() >= MARGIN * A).all()) and bool((A > 0).all()) and float(ra.min()) > 0.0 and \
        float((ra - DELTA).abs().min()) > 1e-6 * DELTA


def _draw(B, S, dt, clamp, tab, seed):
    """(pg, ps, y) [B,S] rounded to dt, on the CPU in float64; crystal b from the seed (seed, b, try)"""
    rows, worst = [], 0
    for b in range(B):
        for sub in range(64):
            g = torch.Generator().manual_seed((seed * 1009 + b) * 64 + sub)
            y = torch.rand(S, generator=g, dtype=torch.float64) - (0.2 if clamp else 0.0)
            pg, ps = torch.rand(S, generator=g, dtype=torch.float64), torch.rand(S, generator=g, dtype=torch.float64)
            pg, ps, y = (x.to(dt).double() for x in (pg, ps, y))
            t = _target(y, clamp)
            if _margins_hold(pg, t, tab) and _margins_hold(ps, t, tab):
                break
        else:
            raise AssertionError(f"crystal {b}: no draw with every |u_k| >= {MARGIN} A_k in 64 tries")
        worst = max(worst, sub)
        rows.append((pg, ps, y))
    pg, ps, y = (torch.stack([r[i] for r in rows]) for i in range(3))
    return pg, ps, y, worst


def _assert_input_margins(pg, ps, y, clamp, tab, kind):
    """The float64 reference is unambiguous on these inputs - asserted over EVERY crystal, output and k."""
    t = _target(y, clamp)
    for p in (pg, ps):
        r = p - t
        u, A = r @ tab.T, r.abs() @ tab.abs().T
        assert bool((u.abs() >= MARGIN * A).all()) and bool((A > 0).all())
        ra = r.abs()
        assert float(ra.min()) > 0.0 and float((ra - DELTA).abs().min()) > 1e-6 * DELTA
        if kind == "huber" and p.numel() >= 51:
            assert bool((ra < DELTA).any()) and bool((ra > DELTA).any())
    if clamp and y.numel() >= 8:
        assert bool((y < 0).any())


def _dev(x, dt):
    return None if x is None else x.to(dt).to(DEV).contiguous()


# ---- the reference and the bars --------------------------------------------------------------------------------------------------
def _e(u, fkind):
    return u ** 2 if fkind == "sq" else u.abs()


def _ref_fn(kind, pg, ps, y, clamp, beta, Bg, w, v, tab, fkind, lam):
    """float64 autograd on the CPU of the definition.  -> dict: l [B], loss, ga, gb (or None), and the fp32 bars in units of
    2^-24 (module docstring): bar_ga, bar_gb, bar_l [B], bar_loss; sa / sb: the pointwise scales (for _judge's tuple)."""
    B, S = pg.shape
    K = tab.shape[0]
    t = _target(y, clamp)
    two = ps is not None
    a = pg.clone().requires_grad_(True)
    fa, ha = _f_w(kind, a, t, v), _e((a - t) @ tab.T, fkind).mean(1)
    lp, l = fa, fa + lam * ha
    b = fb = None
    if two:
        b = ps.clone().requires_grad_(True)
        fb, hb = _f_w(kind, b, t, v), _e((b - t) @ tab.T, fkind).mean(1)
        lp, l = fa + beta * fb, fa + beta * fb + lam * (ha + beta * hb)
    row = (torch.ones(B, dtype=torch.float64) if w is None else w) / Bg
    loss = (row * l).sum()
    loss.backward()
    col = 1.0 if v is None else (v * S / v.sum())[None, :]
    sa = _elem_scale(kind, a.detach(), t, fa.detach(), S) * row[:, None] * col
    sb = None if not two else _elem_scale(kind, b.detach(), t, fb.detach(), S) * row[:, None] * col * beta
    # ---- bars ----
    has_w, has_v = w is not None, v is not None
    n = (S + 63) // 64
    c_u, c_v = n + 7, n + 6
    c_loss_p, c_grad_p = _c(kind, S)
    c_grad_p += int(has_w) + (1 + c_v + (1 if kind == "crystal_rmse" else 0) if has_v else 0)      # (_judge_w's counts)
    c_loss_p += 1 + c_v if has_v else 0
    sq = fkind == "sq"
    absT = tab.abs()

    def scales(p):
        A = (p.detach() - t).abs() @ absT.T                                       # [B,K]
        return ((2.0 * A) @ absT, (A ** 2).sum(1)) if sq else (torch.ones_like(A) @ absT, A.sum(1))

    c_g = (c_u + K if sq else K) + 4 + int(has_w)
    c_h = 2 * c_u + K + 4 if sq else c_u + K + 3
    g_a, h_a = scales(a)
    out = {"l": l.detach(), "loss": loss.detach(), "ga": a.grad, "gb": None, "sa": sa, "sb": sb, "bar_gb": None}
    out["bar_ga"] = c_grad_p * sa + c_g * (row[:, None] * lam / K) * g_a + a.grad.abs()
    h_scale = h_a
    if two:
        g_b, h_b = scales(b)
        out["gb"] = b.grad
        out["bar_gb"] = c_grad_p * sb + (c_g + 1) * (beta * row[:, None] * lam / K) * g_b + b.grad.abs()
        h_scale = h_a + beta * h_b
    out["bar_l"] = c_loss_p * lp.detach() + c_h * (lam / K) * h_scale + l.detach()
    out["bar_loss"] = (row * out["bar_l"]).sum() + (c_total(B, 0) + int(has_w)) * loss.detach()
    return out


WORST = {}                             # fkind -> the largest ratio seen (printed; DESIGN.md 9.12 quotes it)


def _judge_fn(dt, kind, out, ref, B, S, tag, fkind):
    if dt != torch.float32:
        dev = lambda x: None if x is None else x.to(DEV)
        return _judge(dt, kind, out, tuple(dev(ref[k]) for k in ("l", "loss", "ga", "gb", "sa", "sb")), B, S, tag)
    worst = 0.0
    for name, got, g, bar in (("dpg", out.dpg, ref["ga"], ref["bar_ga"]), ("dps", out.dps, ref["gb"], ref["bar_gb"])):
        if g is not None:
            worst = max(worst, bound_ratio(got.cpu(), g, bar, 1, f"{tag}.{name}"))
    if out.per is not None:
        worst = max(worst, bound_ratio(out.per.cpu(), ref["l"], ref["bar_l"], 1, tag + ".per_crystal"))
    worst = max(worst, bound_ratio(out.loss.cpu(), ref["loss"][None], ref["bar_loss"][None], 1, tag + ".loss"))
    WORST[fkind] = max(WORST.get(fkind, 0.0), worst)
    print(f"worst[{fkind}] so far: {WORST[fkind]:.3g}")
    assert worst <= 1.0, (tag, worst)


def _run_fn(dt, pg, ps, y, kind, clamp, beta, Bg, tab, fkind, lam, w=None, wi=None, v=None, per=True):
    B, S = pg.shape
    out = Out(B, S, dt, two=ps is not None, per=per)
    fn = _ops().loss_rows if dt == torch.float32 else _ops().loss_rows64
    kw = {} if tab is None else dict(functionals=tab, functional_kind=fkind, functional_weight=lam)
    fn(pg, ps, y, kind, clamp_target=clamp, beta=beta, delta=DELTA if kind == "huber" else None, dpg=out.dpg, dps=out.dps,
       per_crystal=out.per, loss=out.loss, B_global=Bg, weights=w, weight_index=wi, bin_weights=v, **kw)
    torch.cuda.synchronize()
    out.check_outside()
    return out


def _same(a, b, per=True):
    ok = torch.equal(_bits(a.dpg), _bits(b.dpg)) and torch.equal(_bits(a.loss), _bits(b.loss))
    ok = ok and (a.dps is None or torch.equal(_bits(a.dps), _bits(b.dps)))
    return ok and (not per or torch.equal(_bits(a.per), _bits(b.per)))


def _case(dt, dtn, B, S, K, fkind, which, kinds=KINDS, lam=LAM):
    """one shape, one table: clamp_target in {0, 1} (B_global = B, 3 B), one and two outputs, without and with w + bin_w, every
    pointwise kind; per_crystal = NULL (one launch) gives the two launches' bits"""
    bk = f32(BETA) if dt == torch.float32 else BETA
    tab = _table(which, K, S, dt)
    tab_d = _dev(tab, dt)
    for clamp, Bg in ((False, B), (True, 3 * B)):
        pg, ps, y, redraws = _draw(B, S, dt, clamp, tab, 100000 * B + 1000 * S + K + (7 if clamp else 0))
        print(f"[{dtn},{fkind},{which},B{B},S{S},K{K},clamp{int(clamp)}] redraws per crystal at most {redraws}")
        w_d, v_d = _weights(B, S, dt, 1000 * B + S)
        w, v = w_d.cpu().double(), v_d.cpu().double()
        pg_d, ps_d, y_d = _dev(pg, dt), _dev(ps, dt), _dev(y, dt)
        for kind in kinds:
            _assert_input_margins(pg, ps, y, clamp, tab, kind)
            for weighted in (False, True):
                fw, fv, fw_d, fv_d = (w, v, w_d, v_d) if weighted else (None, None, None, None)
                for two in (True, False):
                    tag = f"loss_rows_fn[{dtn},{fkind},{which},{kind},B{B},S{S},K{K},clamp{int(clamp)}," \
                          f"{'wv' if weighted else 'plain'},{'two' if two else 'one'}]"
                    ref = _ref_fn(kind, pg, ps if two else None, y, clamp, bk if two else 0.0, Bg, fw, fv, tab, fkind, lam)
                    out = _run_fn(dt, pg_d, ps_d if two else None, y_d, kind, clamp, BETA, Bg, tab_d, fkind, lam, w=fw_d, v=fv_d)
                    assert not bool(torch.isnan(out.dpg).any() | torch.isnan(out.per).any() | torch.isnan(out.loss).any())
                    _judge_fn(dt, kind, out, ref, B, S, tag, fkind)
                    nop = _run_fn(dt, pg_d, ps_d if two else None, y_d, kind, clamp, BETA, Bg, tab_d, fkind, lam, w=fw_d, v=fv_d,
                                  per=False)
                    assert _same(out, nop, per=False), tag + " per_crystal=None"


# =====================================================================================================================
# 1. against float64 autograd of the definition
# =====================================================================================================================
@pytest.mark.parametrize("dtn", list(DTYPES))
@pytest.mark.parametrize("fkind", FKINDS)
@pytest.mark.parametrize("which", TABLES)
@pytest.mark.parametrize("B,S,K", SHAPES)
def test_functional_loss_against_float64_autograd(B, S, K, which, fkind, dtn):
    _case(DTYPES[dtn], dtn, B, S, K, fkind, which)


@pytest.mark.parametrize("dtn", list(DTYPES))
@pytest.mark.parametrize("fkind", FKINDS)
def test_functional_loss_at_the_limits(fkind, dtn):
    """(B, S, K) = (5, 512, 512), once per kind and dtype: all eight register chunks of a lane, the longest sums"""
    _case(DTYPES[dtn], dtn, 5, 512, 512, fkind, "random", kinds=["crystal_rmse"])


@pytest.mark.parametrize("dtn", list(DTYPES))
def test_identity_table_squares_make_the_term_the_mse(dtn):
    """Known answer: with the identity table and SQ, h is the crystal's MSE - kind = "mse" with lam = 1 is twice the plain MSE
    call: loss, per-crystal values and gradients, to the bars above (float64: the project's)."""
    dt, B, S = DTYPES[dtn], 6, 65
    bk = f32(BETA) if dt == torch.float32 else BETA
    eye = torch.eye(S, dtype=torch.float64)
    pg, ps, y, _ = _draw(B, S, dt, False, eye, 99)
    ref = _ref_fn("mse", pg, ps, y, False, bk, B, None, None, eye, "sq", 1.0)
    # the float64 reference of the PLAIN call, doubled
    t = _target(y, False)
    a, b = pg.clone().requires_grad_(True), ps.clone().requires_grad_(True)
    l = _f_w("mse", a, t, None) + bk * _f_w("mse", b, t, None)
    (l.sum() / B).backward()
    for got, want in ((ref["l"], 2 * l.detach()), (ref["ga"], 2 * a.grad), (ref["gb"], 2 * b.grad)):
        assert torch.allclose(got, want, rtol=1e-13, atol=0)
    for k, want in (("l", 2 * l.detach()), ("loss", 2 * l.detach().sum() / B), ("ga", 2 * a.grad), ("gb", 2 * b.grad)):
        ref[k] = want
    out = _run_fn(dt, _dev(pg, dt), _dev(ps, dt), _dev(y, dt), "mse", False, BETA, B, _dev(eye, dt), "sq", 1.0)
    _judge_fn(dt, "mse", out, ref, B, S, f"identity[{dtn}]", "sq")
    plain = _run_fn(dt, _dev(pg, dt), _dev(ps, dt), _dev(y, dt), "mse", False, BETA, B, None, "sq", 1.0)
    rel = float(((out.loss.double() - 2 * plain.loss.double()).abs() / out.loss.double()).max())
    assert rel <= (1e-5 if dt == torch.float32 else 1e-12), rel


# =====================================================================================================================
# 2. bit for bit by construction
# =====================================================================================================================
def _some(B, S, K, dt, seed, which="random", clamp=False):
    tab = _table(which, K, S, dt, seed)
    pg, ps, y, _ = _draw(B, S, dt, clamp, tab, seed)
    return _dev(pg, dt), _dev(ps, dt), _dev(y, dt), _dev(tab, dt)


@pytest.mark.parametrize("dtn", list(DTYPES))
@pytest.mark.parametrize("kind", KINDS)
def test_no_table_and_zero_weight_are_the_weighted_entry_bit_for_bit(kind, dtn):
    """functionals=None is the call it was; a table with lam == 0, and the library entry itself with fn_w == NULL, run
    dosx_loss_rows_w's kernels: loss, per-crystal values and both gradients are its bits, with and without w / bin_w."""
    dt, B, S, K = DTYPES[dtn], 9, 65, 7
    o = _ops()
    pg, ps, y, tab = _some(B, S, K, dt, 21)
    w, v = _weights(B, S, dt, 21)
    name = "dosx_loss_rows_fn" if dt == torch.float32 else "dosx_loss_rows_fn_f64"
    for fw, fv in ((None, None), (w, None), (None, v), (w, v)):
        for p2 in (ps, None):
            for per in (True, False):
                base = _run_fn(dt, pg, p2, y, kind, False, BETA, B, None, "sq", LAM, w=fw, v=fv, per=per)
                for fkind in FKINDS:
                    zero = _run_fn(dt, pg, p2, y, kind, False, BETA, B, tab, fkind, 0.0, w=fw, v=fv, per=per)
                    assert _same(zero, base, per), (fkind, fw is not None, fv is not None, per)
                null = Out(B, S, dt, two=p2 is not None, per=per)
                o._call(name, pg.data_ptr(), o._p(p2), y.data_ptr(), B, S, B, o.LOSS_KINDS[kind], 0, BETA,
                        DELTA if kind == "huber" else 0.0, null.dpg.data_ptr(), o._p(null.dps), o._p(null.per), null.loss.data_ptr(),
                        o._p(fw), None, o._p(fv), None, 0, 1, LAM, o._stream())
                torch.cuda.synchronize()
                null.check_outside()
                assert _same(null, base, per), ("fn_w NULL", fw is not None, fv is not None, per)


@pytest.mark.parametrize("dtn", list(DTYPES))
@pytest.mark.parametrize("fkind", FKINDS)
def test_appended_zero_rows_change_nothing_beyond_the_exact_one_over_k(fkind, dtn):
    """K -> 2 K with K all-zero rows appended (and interleaved) and lam -> 2 lam: lam / K is the same number, a zero row adds +0
    to every sum - every output bit is the same."""
    dt, B, S, K = DTYPES[dtn], 6, 65, 33
    pg, ps, y, tab = _some(B, S, K, dt, 31)
    w, v = _weights(B, S, dt, 31)
    appended = torch.cat([tab, torch.zeros_like(tab)]).contiguous()
    interleaved = torch.stack([tab, torch.zeros_like(tab)], 1).reshape(2 * K, S).contiguous()
    for kind in KINDS:
        for fw, fv in ((None, None), (w, v)):
            for per in (True, False):
                a = _run_fn(dt, pg, ps, y, kind, False, BETA, B, tab, fkind, LAM, w=fw, v=fv, per=per)
                for wide in (appended, interleaved):
                    b = _run_fn(dt, pg, ps, y, kind, False, BETA, B, wide, fkind, 2 * LAM, w=fw, v=fv, per=per)
                    assert _same(a, b, per), (kind, fw is not None, per)
                c = _run_fn(dt, pg, ps, y, kind, False, BETA, B, appended, fkind, LAM, w=fw, v=fv, per=per)
                assert not torch.equal(a.dpg, c.dpg)                     # (input condition: the term is in the gradient)


@pytest.mark.parametrize("dtn", list(DTYPES))
@pytest.mark.parametrize("fkind", FKINDS)
@pytest.mark.parametrize("where", ["predictions", "target"])
def test_zero_sample_weight_takes_a_crystal_out_whatever_it_holds(where, fkind, dtn):
    """Crystal 2 holds a NaN and an inf, w_2 = 0: its rows are +0.0, loss[0] is finite and bitwise the clean value,
    per_crystal[2] is the NaN, every other row is bitwise unchanged."""
    dt, B, S, K = DTYPES[dtn], 5, 51, 51
    pg, ps, y, tab = _some(B, S, K, dt, 41, which="cumulative")
    w, v = _weights(B, S, dt, 41)
    w[2] = 0.0
    bg, bs, by = pg.clone(), ps.clone(), y.clone()
    if where == "predictions":
        bg[2, 4], bg[2, 9], bs[2, 5], bs[2, 11] = NAN, math.inf, math.inf, NAN
    else:
        by[2, 4], by[2, 9] = NAN, -math.inf
    others = torch.tensor([0, 1, 3, 4], device=DEV)
    for kind in KINDS:
        for fv in (None, v):
            for per in (True, False):
                clean = _run_fn(dt, pg, ps, y, kind, False, BETA, B, tab, fkind, LAM, w=w, v=fv, per=per)
                bad = _run_fn(dt, bg, bs, by, kind, False, BETA, B, tab, fkind, LAM, w=w, v=fv, per=per)
                for o in (clean, bad):
                    for d in (o.dpg, o.dps):
                        assert bool((_bits(d[2]) == 0).all()), (kind, per)           # +0.0: every bit clear
                assert bool(torch.isfinite(bad.loss).all()) and torch.equal(_bits(bad.loss), _bits(clean.loss))
                assert torch.equal(_bits(bad.dpg[others]), _bits(clean.dpg[others]))
                assert torch.equal(_bits(bad.dps[others]), _bits(clean.dps[others]))
                if per:
                    assert bool(torch.isnan(bad.per[2])) and bool(torch.isfinite(clean.per[2]))
                    assert torch.equal(_bits(bad.per[others]), _bits(clean.per[others]))


@pytest.mark.parametrize("dtn", list(DTYPES))
@pytest.mark.parametrize("fkind", FKINDS)
def test_a_nan_stays_in_its_crystal(fkind, dtn):
    """A NaN (or an inf) in crystal 1 reaches its l_b, loss[0] and its rows - through the table every element of them - and no
    other crystal's rows or per-crystal value."""
    dt, B, S, K = DTYPES[dtn], 6, 65, 65
    pg, ps, y, tab = _some(B, S, K, dt, 51, which="cumulative")
    others = torch.tensor([0, 2, 3, 4, 5], device=DEV)
    for bad_value in (NAN, math.inf):
        bg = pg.clone()
        bg[1, 3] = bad_value
        for kind in KINDS:
            for per in (True, False):
                clean = _run_fn(dt, pg, ps, y, kind, False, BETA, B, tab, fkind, LAM, per=per)
                bad = _run_fn(dt, bg, ps, y, kind, False, BETA, B, tab, fkind, LAM, per=per)
                assert not bool(torch.isfinite(bad.loss).any()) and not bool(torch.isfinite(bad.dpg[1]).all())
                assert torch.equal(_bits(bad.dpg[others]), _bits(clean.dpg[others]))
                assert torch.equal(_bits(bad.dps), _bits(clean.dps))             # (the other output of the same crystal too)
                if per:
                    assert not bool(torch.isfinite(bad.per[1])) and torch.equal(_bits(bad.per[others]), _bits(clean.per[others]))


@pytest.mark.parametrize("dtn", list(DTYPES))
def test_two_runs_are_bitwise_equal(dtn):
    dt, B, S, K = DTYPES[dtn], 257, 65, 40
    pg, ps, y, tab = _some(B, S, K, dt, 61, clamp=True)
    w, v = _weights(B, S, dt, 61)
    for fkind in FKINDS:
        for kind in KINDS:
            for per in (True, False):
                a = _run_fn(dt, pg, ps, y, kind, True, BETA, B, tab, fkind, LAM, w=w, v=v, per=per)
                b = _run_fn(dt, pg, ps, y, kind, True, BETA, B, tab, fkind, LAM, w=w, v=v, per=per)
                assert _same(a, b, per), (fkind, kind, per)


@pytest.mark.parametrize("dtn", list(DTYPES))
@pytest.mark.parametrize("fkind", FKINDS)
def test_a_crystals_numbers_do_not_depend_on_the_batch_or_its_place_in_it(fkind, dtn):
    """The same crystal first in a batch of 1 and last in a batch of 257 (B_global = 257 both times: the coefficient is the
    same number): its gradient rows and its per-crystal value are the same bits - and in the one-workgroup form too."""
    dt, B, S, K = DTYPES[dtn], 257, 51, 51
    pg, ps, y, tab = _some(B, S, K, dt, 71)
    for kind in KINDS:
        big = _run_fn(dt, pg, ps, y, kind, False, BETA, B, tab, fkind, LAM)
        big_solo = _run_fn(dt, pg, ps, y, kind, False, BETA, B, tab, fkind, LAM, per=False)
        one = _run_fn(dt, pg[-1:].contiguous(), ps[-1:].contiguous(), y[-1:].contiguous(), kind, False, BETA, B, tab, fkind, LAM)
        for got in (big, big_solo):
            assert torch.equal(_bits(got.dpg[-1:]), _bits(one.dpg)) and torch.equal(_bits(got.dps[-1:]), _bits(one.dps)), kind
        assert torch.equal(_bits(big.per[-1:]), _bits(one.per)), kind


# =====================================================================================================================
# 3. the wrappers
# =====================================================================================================================
def test_wrapper_checks_the_table():
    o = _ops()
    pg, ps, y, tab = _some(4, 51, 5, torch.float32, 1)
    mk = lambda *s: torch.empty(*s, device=DEV)
    kw = lambda **k: {**dict(dpg=mk(4, 51), dps=mk(4, 51), per_crystal=mk(4), loss=mk(1)), **k}
    with pytest.raises(TypeError, match="functionals"):
        o.loss_rows(pg, ps, y, "mse", **kw(functionals=tab.double()))
    with pytest.raises(TypeError, match="functionals"):
        o.loss_rows(pg, ps, y, "mse", **kw(functionals=tab.cpu()))
    with pytest.raises(TypeError, match="functionals"):
        o.loss_rows64(pg.double(), ps.double(), y.double(), "mse", dpg=mk(4, 51).double(), dps=mk(4, 51).double(),
                      loss=mk(1).double(), functionals=tab)
    for bad in (tab[:, :50], tab[0], mk(5, 102)[:, ::2], mk(513, 51), mk(0, 51)):
        with pytest.raises(ValueError, match="functionals"):
            o.loss_rows(pg, ps, y, "mse", **kw(functionals=bad))
    with pytest.raises(ValueError, match="functional_kind"):
        o.loss_rows(pg, ps, y, "mse", **kw(functionals=tab, functional_kind="l2"))
    for lam in (-1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="functional_weight"):
            o.loss_rows(pg, ps, y, "mse", **kw(functionals=tab, functional_weight=lam))
    # (the library's own refusals: tests/test_loss_functional_abi.py, without a GPU)
