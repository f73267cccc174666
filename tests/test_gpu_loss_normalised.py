"""dosx_loss_rows_fn_norm / _f64 and their descriptor forms (csrc/loss_functional.hip) on a real MI355X: the per-crystal losses
with a penalty on K functionals of the DOS whose LAST K_norm rows are divided by one floored denominator functional, against
float64 torch autograd of the definition in include/dosx.h, computed on the CPU on the same rounded inputs, table, denominator
row and floor (``clamp(min=floor)`` is D+) -

    D(x) = sum_s den[s] x_s,  D+ = max(D, floor),  plain row: u_k = F_k(p) - F_k(t),  normalised: u_k = F_k(p) / D+(p) - F_k(t) / D+(t),
    h = (1 / K) sum_k e(u_k),  l_b = f(pg_b) + beta f(ps_b) + lam (h(pg_b) + beta h(ps_b)),  loss[0] = sum_b w_b l_b / B_global

- and what holds bit for bit by construction: K_norm = 0 (dosx_loss_rows_fn's launches), lam == 0 and no table (dosx_loss_rows_w's),
the literal entry against its descriptor form, run to run, a crystal wherever it stands in whatever batch, a zero sample weight,
a NaN confined to its crystal.

float64 is held to the project's bars (tests/test_gpu_loss_rows._judge): 1e-12 relative for loss and per_crystal, 1e-10 of the
row's largest entry for the gradient rows.

fp32 is judged element by element with tests/gpu_util.bound_ratio.  Every element's bar is the pointwise term's own bar
(tests/test_gpu_loss_functional.py) PLUS the new term's bar PLUS one rounding of the result for the final addition.  The new
term's bar is counted from the kernel's summation order (the header comment of csrc/loss_functional.hip), every rounding at most
2^-24 of the magnitude it acts on, n = ceil(S / 64).  The inputs are non-negative and the denominator row positive (asserted), so
sum_s |den_s x_s| = D(x) <= D+(x): a relative error of D is at most that of D+.

  D(x), against D(x): the product (1), n - 1 additions in the lane, 6 levels of the wave reduction:               c_d = n + 6
  F_k(x), against M_k(x) = sum_s |fn_w[k,s] x_s|: the same:                                                     c_F = n + 6
  q_k(x) = F_k / D+, against Q_k(x) = M_k(x) / D+(x): c_F, the denominator's c_d, the division (1):             c_q = c_F + c_d + 1
  a normalised u_k = q_k(p) - q_k(t), against U_k = Q_k(p) + Q_k(t): c_q on either part, the subtraction (1):   c_un = c_q + 1
  a plain u_k, against A_k = sum_s |fn_w[k,s] r_s| (tests/test_gpu_loss_functional.py):                            c_up = n + 7 <= c_un
  c_k of a normalised row, against C_k = 2 U_k / D+(p) (SQ) or 1 / D+(p) (ABS): SQ 2 u_k carries c_un (the doubling is exact),
      ABS +-1 is exact (the inputs keep |u_k| >= 1e-4 U_k, far above c_un 2^-24 U_k); the denominator's c_d, the division (1):
                                                                                          c_c = [c_un] + c_d + 1
  part 1 of a gradient element, sum_k c_k fn_w[k,s], against P1_s = sum_k C_k |fn_w[k,s]| (plain rows: C_k = 2 A_k or 1, their
      own count c_up + K or K is not larger): c_c, the product (1), the K - 1 additions over k (counted as K):    c_1 = c_c + 1 + K
  A = sum_k c_k q_k(p), against Ahat = sum_k C_k Q_k(p): c_c, c_q, the product (1), K_norm - 1 additions (counted as K_norm);
  part 2, a den[s], against P2_s = [D > floor] Ahat |den[s]|: one product more:                                  c_2 = c_c + c_q + 2 + K_norm
      (the gate is exact: the inputs keep |D - floor| >= 1e-3 D, far above c_d 2^-24 D)
  the element, coef lam / K (part 1 - part 2), against G_s = coef lam / K (P1_s + P2_s): the subtraction (1), and the coefficient
      as in tests/test_gpu_loss_functional.py: 1 / B_global, lam / K, their product, times the difference (4), + 1 with sample
      weights, + 1 for the second output:                                                  c_1 + 5 [+ 1] [+ 1] on P1, c_2 + 5 [+ 1] [+ 1] on P2
  per_crystal, against lam / K (sum_k V_k^2 [+ beta ...]) (SQ) or lam / K (sum_k V_k [+ beta ...]) (ABS), V_k = U_k on normalised and
      A_k on plain rows: SQ 2 c_un + 1, ABS c_un, K - 1 additions, then lam / K, beta h(ps), the sum of the two, the product (4):
                                                                                          SQ 2 c_un + K + 4,   ABS c_un + K + 3
  loss[0]: every crystal's bar times w_b / B_global, + tests/test_gpu_loss_rows.c_total's own roundings of the final sum.

Contraction into fused multiply-adds removes roundings and never adds one, so the counts are upper bounds either way.  The largest
error / bar ratio seen per kind is printed (DESIGN.md 9.13 quotes it).

Inputs: uniform [0,1) predictions and targets (targets shifted down by 0.2 where the clamp is tested), den_floor = 1e-3 rounded to
the operands' type, every crystal drawn from a seed of its own and redrawn alone (next sub-seed, at most 64 times) until on BOTH
outputs every normalised |u_k| >= 1e-4 U_k, every plain |u_k| >= 1e-4 A_k, |D - floor| >= 1e-3 sum_s |den_s x_s| for both
predictions and the target, and the pointwise margins of tests/test_gpu_loss_rows.py hold; asserted on the CPU over every crystal
and k before anything is judged, and nothing is left out of the judgement.  The LAST crystal of every batch is the designated
floored one: its predictions are scaled by an exact power of two, 2^-12 / 2^ceil(log2 S) (2^-12 alone leaves D(p) ~ S / 2^15 above
the floor from S ~ 32 on), so that D(p) < floor - asserted - and its floored gradient (no denominator part) is judged with the
rest.  The dense random table at (5, 512, 512) does not meet the |u_k| margin (2 of 5 crystals exhaust the 64 tries): that case
runs "sq" only, where that margin is no condition; "abs" at (512, 512) runs the cumulative table."""
import functools
import math

import pytest
import torch

from tests.gpu_util import DEV, bound_ratio
from tests.test_gpu_loss_functional import _dev, _e, _same
from tests.test_gpu_loss_rows import DELTA, DTYPES, KINDS, NAN, Out, _c, _elem_scale, _judge, _ops, _target, c_total, f32
from tests.test_gpu_loss_weighted import BETA, _bits, _f_w, _weights

pytestmark = pytest.mark.gpu

# S over the lane boundaries at B = 5 with one functional and with S of them; K one over / one under S at the 64 edge; B over the
# four-crystals-per-workgroup edge and the one-workgroup form's 256 at (S, K) = (51, 51).  (5, 512, 512) runs once, below.
SHAPES = sorted({(5, S, K) for S in (2, 63, 64, 65, 201) for K in (1, S)}) + [(5, 64, 65), (5, 65, 64)] + \
    [(B, 51, 51) for B in (1, 3, 4, 257)]
FKINDS = ["sq", "abs"]
TABLES = ["cumulative", "random"]
LAM = 0.5                              # exact in fp32
MARGIN, D_MARGIN = 1e-4, 1e-3


def _floor(dt):
    return f32(1e-3) if dt == torch.float32 else 1e-3


def _knorms(K):
    """every row, about half (a mixed table), one"""
    return sorted({K, max(1, K // 2), 1}, reverse=True)


@pytest.fixture(scope="module", autouse=True)
def _own_memory_pool():
    """As tests/test_gpu_loss_weighted.py: this module allocates from a memory pool of its own, given back when it is done."""
    pool = torch.cuda.MemPool()
    with torch.cuda.use_mem_pool(pool):
        yield
    torch.cuda.synchronize()
    del pool


# ---- tables and inputs (all on the CPU; moved to the device once) ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _table(which, K, S, dt, seed=0):
    """cumulative: row k is 0.25 on the bins below the k-th of K equal steps through the first 90 % of the grid; random: dense
    uniform (-1, 1).  The denominator row: 0.25 U(0.5, 1.5), strictly positive.  Rounded to dt; on the CPU in float64."""
    g = torch.Generator().manual_seed(4242 + 7 * K + S + seed)
    if which == "cumulative":
        t = torch.zeros(K, S, dtype=torch.float64)
        for k in range(K):
            t[k, :min(S, max(1, math.ceil((k + 1) * 0.9 * S / K)))] = 0.25
    else:
        t = 2.0 * torch.rand(K, S, generator=g, dtype=torch.float64) - 1.0
    den = 0.25 * (0.5 + torch.rand(S, generator=g, dtype=torch.float64))
    return t.to(dt).double(), den.to(dt).double()


def _us(p, t, tab, den, Kn, floor):
    """one output p [.., S] against t: (u [.., K], its cancellation-free magnitude V [.., K]: A_k on plain rows, U_k on normalised)"""
    Kp = tab.shape[0] - Kn
    r = p - t
    up, Ap = r @ tab[:Kp].T, r.abs() @ tab[:Kp].abs().T
    Dp, Dt = (p @ den).clamp(min=floor)[..., None], (t @ den).clamp(min=floor)[..., None]
    un = (p @ tab[Kp:].T) / Dp - (t @ tab[Kp:].T) / Dt
    Un = (p.abs() @ tab[Kp:].abs().T) / Dp + (t.abs() @ tab[Kp:].abs().T) / Dt
    return torch.cat([up, un], -1), torch.cat([Ap, Un], -1)


def _margins_hold(p, t, tab, den, Kn, floor, u_margin=True):
    u, V = _us(p, t, tab, den, Kn, floor)
    ok = bool((V > 0).all()) and (not u_margin or bool((u.abs() >= MARGIN * V).all()))
    for x in (p, t):
        ok = ok and abs(float(x @ den) - floor) >= D_MARGIN * float((x * den).abs().sum())
    ra = (p - t).abs()
    return ok and float(ra.min()) > 0.0 and float((ra - DELTA).abs().min()) > 1e-6 * DELTA


def _floored_scale(S):
    return 2.0 ** -(12 + math.ceil(math.log2(S)))


@functools.lru_cache(maxsize=None)
def _draw(B, S, dt, clamp, which, K, Kn, seed, u_margin=True, designate=True):
    """(pg, ps, y) [B,S] rounded to dt, on the CPU in float64; crystal b from the seed (seed, b, try); the last crystal's
    predictions scaled so that D(p) < floor"""
    tab, den = _table(which, K, S, dt)
    floor = _floor(dt)
    rows, worst = [], 0
    for b in range(B):
        scale = _floored_scale(S) if designate and b == B - 1 else 1.0
        for sub in range(64):
            g = torch.Generator().manual_seed((seed * 1009 + b) * 64 + sub)
            y = torch.rand(S, generator=g, dtype=torch.float64) - (0.2 if clamp else 0.0)
            pg, ps = torch.rand(S, generator=g, dtype=torch.float64), torch.rand(S, generator=g, dtype=torch.float64)
            pg, ps, y = ((x.to(dt).double()) for x in (pg * scale, ps * scale, y))
            t = _target(y, clamp)
            if _margins_hold(pg, t, tab, den, Kn, floor, u_margin) and _margins_hold(ps, t, tab, den, Kn, floor, u_margin):
                break
        else:
            raise AssertionError(f"crystal {b}: no draw inside the margins in 64 tries")
        worst = max(worst, sub)
        rows.append((pg, ps, y))
    pg, ps, y = (torch.stack([r[i] for r in rows]) for i in range(3))
    return pg, ps, y, worst


def _assert_input_margins(pg, ps, y, clamp, tab, den, Kn, floor, kind, u_margin=True, designate=True):
    """The float64 reference is unambiguous on these inputs - asserted over EVERY crystal, output and k."""
    t = _target(y, clamp)
    assert bool((den > 0).all()) and bool((t >= 0).all())
    assert bool(((t @ den - floor).abs() >= D_MARGIN * (t.abs() @ den.abs())).all())
    for p in (pg, ps):
        assert bool((p >= 0).all())
        u, V = _us(p, t, tab, den, Kn, floor)
        assert bool((V > 0).all()) and (not u_margin or bool((u.abs() >= MARGIN * V).all()))
        D = p @ den
        assert bool(((D - floor).abs() >= D_MARGIN * (p.abs() @ den.abs())).all())
        if designate:
            assert float(D[-1]) < floor and (p.shape[0] == 1 or bool((D[:-1] > floor).all()))
        ra = (p - t).abs()
        assert float(ra.min()) > 0.0 and float((ra - DELTA).abs().min()) > 1e-6 * DELTA
        if kind == "huber" and p.numel() >= 51:
            assert bool((ra < DELTA).any()) and bool((ra > DELTA).any())
    if clamp and y.numel() >= 8:
        assert bool((y < 0).any())


# ---- the reference and the bars --------------------------------------------------------------------------------------------------
def _h(p, t, tab, den, Kn, floor, fkind):
    return _e(_us(p, t, tab, den, Kn, floor)[0], fkind).mean(-1)


def _ref_norm(kind, pg, ps, y, clamp, beta, Bg, w, v, tab, den, Kn, floor, fkind, lam):
    """float64 autograd on the CPU of the definition.  -> dict: l [B], loss, ga, gb (or None), and the fp32 bars in units of
    2^-24 (module docstring): bar_ga, bar_gb, bar_l [B], bar_loss; sa / sb: the pointwise scales (for _judge's tuple)."""
    B, S = pg.shape
    K = tab.shape[0]
    Kp = K - Kn
    t = _target(y, clamp)
    two = ps is not None
    a = pg.clone().requires_grad_(True)
    fa, ha = _f_w(kind, a, t, v), _h(a, t, tab, den, Kn, floor, fkind)
    lp, l = fa, fa + lam * ha
    b = fb = None
    if two:
        b = ps.clone().requires_grad_(True)
        fb, hb = _f_w(kind, b, t, v), _h(b, t, tab, den, Kn, floor, fkind)
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
    c_d = c_F = n + 6
    c_q = c_F + c_d + 1
    c_un = c_q + 1
    c_v = n + 6
    c_loss_p, c_grad_p = _c(kind, S)
    c_grad_p += int(has_w) + (1 + c_v + (1 if kind == "crystal_rmse" else 0) if has_v else 0)      # (_judge_w's counts)
    c_loss_p += 1 + c_v if has_v else 0
    sq = fkind == "sq"
    c_c = (c_un if sq else 0) + c_d + 1
    c_1 = c_c + 1 + K
    c_2 = c_c + c_q + 2 + Kn
    tail = 5 + int(has_w)
    c_h = 2 * c_un + K + 4 if sq else c_un + K + 3
    absT = tab.abs()

    def scales(p):
        """(P1 [B,S], P2 [B,S], sum_k V_k^2 or sum_k V_k [B]) of one output"""
        p = p.detach()
        V = _us(p, t, tab, den, Kn, floor)[1]                                      # [B,K]
        D = p @ den
        Dp = D.clamp(min=floor)[:, None]
        Ck = torch.cat([2.0 * V[:, :Kp], 2.0 * V[:, Kp:] / Dp], 1) if sq else \
            torch.cat([torch.ones(B, Kp, dtype=torch.float64), torch.ones(B, Kn, dtype=torch.float64) / Dp], 1)
        Q = (p.abs() @ absT[Kp:].T) / Dp
        Ahat = (Ck[:, Kp:] * Q).sum(1)
        P2 = torch.where(D > floor, Ahat, torch.zeros_like(Ahat))[:, None] * den.abs()[None, :]
        return Ck @ absT, P2, (V ** 2).sum(1) if sq else V.sum(1)

    p1, p2, h_a = scales(a)
    out = {"l": l.detach(), "loss": loss.detach(), "ga": a.grad, "gb": None, "sa": sa, "sb": sb, "bar_gb": None}
    out["bar_ga"] = c_grad_p * sa + (row[:, None] * lam / K) * ((c_1 + tail) * p1 + (c_2 + tail) * p2) + a.grad.abs()
    h_scale = h_a
    if two:
        p1, p2, h_b = scales(b)
        out["gb"] = b.grad
        out["bar_gb"] = c_grad_p * sb + (beta * row[:, None] * lam / K) * ((c_1 + tail + 1) * p1 + (c_2 + tail + 1) * p2) \
            + b.grad.abs()
        h_scale = h_a + beta * h_b
    out["bar_l"] = c_loss_p * lp.detach() + c_h * (lam / K) * h_scale + l.detach()
    out["bar_loss"] = (row * out["bar_l"]).sum() + (c_total(B, 0) + int(has_w)) * loss.detach()
    return out


WORST = {}                             # fkind -> the largest ratio seen (printed; DESIGN.md 9.13 quotes it)


def _judge_norm(dt, kind, out, ref, B, S, tag, fkind):
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


def _run_norm(dt, pg, ps, y, kind, clamp, beta, Bg, tab, den, Kn, floor, fkind, lam, w=None, wi=None, v=None, per=True):
    B, S = pg.shape
    out = Out(B, S, dt, two=ps is not None, per=per)
    fn = _ops().loss_rows if dt == torch.float32 else _ops().loss_rows64
    fn(pg, ps, y, kind, clamp_target=clamp, beta=beta, delta=DELTA if kind == "huber" else None, dpg=out.dpg, dps=out.dps,
       per_crystal=out.per, loss=out.loss, B_global=Bg, weights=w, weight_index=wi, bin_weights=v, functionals=tab,
       functional_kind=fkind, functional_weight=lam, functional_denominator=den, functional_norm_rows=Kn, functional_floor=floor)
    torch.cuda.synchronize()
    out.check_outside()
    return out


def _case(dt, dtn, B, S, K, Kn, fkind, which, kinds=("crystal_rmse",), lam=LAM, u_margin=True):
    """one shape, one table, one K_norm: clamp_target in {0, 1} (B_global = B, 3 B), one and two outputs, without and with w +
    bin_w, the pointwise kinds given; per_crystal = NULL (one launch) gives the two launches' bits"""
    bk = f32(BETA) if dt == torch.float32 else BETA
    tab, den = _table(which, K, S, dt)
    floor = _floor(dt)
    tab_d, den_d = _dev(tab, dt), _dev(den, dt)
    for clamp, Bg in ((False, B), (True, 3 * B)):
        pg, ps, y, redraws = _draw(B, S, dt, clamp, which, K, Kn, 100000 * B + 1000 * S + K + (7 if clamp else 0), u_margin)
        print(f"[{dtn},{fkind},{which},B{B},S{S},K{K},Kn{Kn},clamp{int(clamp)}] redraws per crystal at most {redraws}")
        w_d, v_d = _weights(B, S, dt, 1000 * B + S)
        w, v = w_d.cpu().double(), v_d.cpu().double()
        pg_d, ps_d, y_d = _dev(pg, dt), _dev(ps, dt), _dev(y, dt)
        for kind in kinds:
            _assert_input_margins(pg, ps, y, clamp, tab, den, Kn, floor, kind, u_margin)
            for weighted in (False, True):
                fw, fv, fw_d, fv_d = (w, v, w_d, v_d) if weighted else (None, None, None, None)
                for two in (True, False):
                    tag = f"loss_rows_fn_norm[{dtn},{fkind},{which},{kind},B{B},S{S},K{K},Kn{Kn},clamp{int(clamp)}," \
                          f"{'wv' if weighted else 'plain'},{'two' if two else 'one'}]"
                    ref = _ref_norm(kind, pg, ps if two else None, y, clamp, bk if two else 0.0, Bg, fw, fv, tab, den, Kn, floor,
                                    fkind, lam)
                    out = _run_norm(dt, pg_d, ps_d if two else None, y_d, kind, clamp, BETA, Bg, tab_d, den_d, Kn, floor, fkind, lam,
                                    w=fw_d, v=fv_d)
                    assert not bool(torch.isnan(out.dpg).any() | torch.isnan(out.per).any() | torch.isnan(out.loss).any())
                    _judge_norm(dt, kind, out, ref, B, S, tag, fkind)
                    nop = _run_norm(dt, pg_d, ps_d if two else None, y_d, kind, clamp, BETA, Bg, tab_d, den_d, Kn, floor, fkind, lam,
                                    w=fw_d, v=fv_d, per=False)
                    assert _same(out, nop, per=False), tag + " per_crystal=None"


# =====================================================================================================================
# 1. against float64 autograd of the definition
# =====================================================================================================================
@pytest.mark.parametrize("dtn", list(DTYPES))
@pytest.mark.parametrize("fkind", FKINDS)
@pytest.mark.parametrize("which", TABLES)
@pytest.mark.parametrize("B,S,K", SHAPES)
def test_normalised_loss_against_float64_autograd(B, S, K, which, fkind, dtn):
    for Kn in _knorms(K):
        _case(DTYPES[dtn], dtn, B, S, K, Kn, fkind, which)


@pytest.mark.parametrize("dtn", list(DTYPES))
@pytest.mark.parametrize("fkind", FKINDS)
@pytest.mark.parametrize("which", TABLES)
def test_normalised_loss_with_every_pointwise_kind(which, fkind, dtn):
    """all four pointwise kinds at (5, 65, 64) with a mixed table"""
    _case(DTYPES[dtn], dtn, 5, 65, 64, 32, fkind, which, kinds=KINDS)


@pytest.mark.parametrize("dtn", list(DTYPES))
@pytest.mark.parametrize("fkind,which", [("sq", "random"), ("sq", "cumulative"), ("abs", "cumulative")])
def test_normalised_loss_at_the_limits(fkind, which, dtn):
    """(B, S, K) = (5, 512, 512), every row normalised: all eight register chunks of a lane, the longest sums.  The dense random
    table does not meet the |u_k| margin here (module docstring): "sq" only, where it is no condition."""
    _case(DTYPES[dtn], dtn, 5, 512, 512, 512, fkind, which, u_margin=which != "random")


@pytest.mark.parametrize("fkind", FKINDS)
def test_a_normalised_term_leaves_the_scale_free(fkind):
    """Euler: with every row normalised and D > floor the term is homogeneous of degree 0 in p, so its gradient - the entry with
    lam minus the entry with lam = 0, float64 - is orthogonal to p: |sum_s p_s g_s| <= 1e-10 sum_s |p_s g_s| on every crystal."""
    dt, B, S, K = torch.float64, 6, 65, 65
    tab, den = _table("random", K, S, dt)
    pg, ps, y, _ = _draw(B, S, dt, False, "random", K, K, 81, True, False)
    assert bool(((pg @ den) > _floor(dt)).all()) and bool(((ps @ den) > _floor(dt)).all())
    args = [_dev(x, dt) for x in (pg, ps, y)]
    with_term = _run_norm(dt, *args, "crystal_rmse", False, BETA, B, _dev(tab, dt), _dev(den, dt), K, _floor(dt), fkind, LAM)
    without = _run_norm(dt, *args, "crystal_rmse", False, BETA, B, _dev(tab, dt), _dev(den, dt), K, _floor(dt), fkind, 0.0)
    for p, got, base in ((pg, with_term.dpg, without.dpg), (ps, with_term.dps, without.dps)):
        g = (got - base).cpu()
        assert float(g.abs().max()) > 1e-6                                   # (input condition: the term is in the gradient)
        dot, mag = (p * g).sum(1).abs(), (p * g).abs().sum(1)
        print(f"euler[{fkind}]: worst |sum p g| / sum |p g| = {float((dot / mag).max()):.2e}")
        assert bool((dot <= 1e-10 * mag).all())


# =====================================================================================================================
# 2. bit for bit by construction
# =====================================================================================================================
def _some(B, S, K, Kn, dt, seed, which="random", clamp=False):
    tab, den = _table(which, K, S, dt)
    pg, ps, y, _ = _draw(B, S, dt, clamp, which, K, Kn, seed)
    return _dev(pg, dt), _dev(ps, dt), _dev(y, dt), _dev(tab, dt), _dev(den, dt)


def _raw(dt, desc, pg, ps, y, kind, Bg, w, v, tab, K, fkind, lam, den, Kn, floor, per=True):
    """the library entry itself - the literal one or its descriptor form - on sentinel-guarded outputs"""
    o = _ops()
    from dostransformer_amd import _abi
    B, S = pg.shape
    out = Out(B, S, dt, two=ps is not None, per=per)
    name = "dosx_loss_rows_fn_norm" + ("_desc" if desc else "") + ("" if dt == torch.float32 else "_f64")
    head = (pg.data_ptr(), o._p(ps), y.data_ptr(), B, S, Bg, o.LOSS_KINDS[kind], 0, BETA, DELTA if kind == "huber" else 0.0,
            out.dpg.data_ptr(), o._p(out.dps), o._p(out.per), out.loss.data_ptr(), o._p(w), None, o._p(v))
    fk = o.FUNCTIONAL_KINDS[fkind]
    if desc:
        import ctypes as C
        d = _abi.FnNorm()
        d.fn_w, d.fn_den, d.K, d.K_norm, d.fn_kind, d.lam, d.den_floor = o._p(tab), o._p(den), K, Kn, fk, lam, floor
        o._call(name, *head, C.byref(d), o._stream())
    else:
        o._call(name, *head, o._p(tab), K, fk, lam, o._p(den), Kn, floor, o._stream())
    torch.cuda.synchronize()
    out.check_outside()
    return out


def _run_fn(dt, pg, ps, y, kind, Bg, tab, fkind, lam, w=None, v=None, per=True):
    """dosx_loss_rows_fn (a table) or dosx_loss_rows_w / dosx_loss_rows (none) through the wrapper"""
    B, S = pg.shape
    out = Out(B, S, dt, two=ps is not None, per=per)
    fn = _ops().loss_rows if dt == torch.float32 else _ops().loss_rows64
    kw = {} if tab is None else dict(functionals=tab, functional_kind=fkind, functional_weight=lam)
    fn(pg, ps, y, kind, clamp_target=False, beta=BETA, delta=DELTA if kind == "huber" else None, dpg=out.dpg, dps=out.dps,
       per_crystal=out.per, loss=out.loss, B_global=Bg, weights=w, bin_weights=v, **kw)
    torch.cuda.synchronize()
    out.check_outside()
    return out


@pytest.mark.parametrize("dtn", list(DTYPES))
@pytest.mark.parametrize("kind", KINDS)
def test_nothing_to_normalise_is_the_linear_entry_bit_for_bit(kind, dtn):
    """K_norm = 0 (with and without a denominator row) runs dosx_loss_rows_fn's launches; lam == 0 and fn_w == NULL run
    dosx_loss_rows_w's - through the literal entry and through its descriptor form, with and without w / bin_w."""
    dt, B, S, K = DTYPES[dtn], 9, 65, 7
    pg, ps, y, tab, den = _some(B, S, K, 3, dt, 21)
    w, v = _weights(B, S, dt, 21)
    floor = _floor(dt)
    for fw, fv in ((None, None), (w, v)):
        for p2 in (ps, None):
            for per in (True, False):
                plain = _run_fn(dt, pg, p2, y, kind, B, None, "sq", LAM, w=fw, v=fv, per=per)
                for fkind in FKINDS:
                    lin = _run_fn(dt, pg, p2, y, kind, B, tab, fkind, LAM, w=fw, v=fv, per=per)
                    for desc in (False, True):
                        for d in (den, None):
                            got = _raw(dt, desc, pg, p2, y, kind, B, fw, fv, tab, K, fkind, LAM, d, 0, floor, per=per)
                            assert _same(got, lin, per), ("K_norm 0", fkind, desc, d is None, per)
                        got = _raw(dt, desc, pg, p2, y, kind, B, fw, fv, tab, K, fkind, 0.0, den, 3, floor, per=per)
                        assert _same(got, plain, per), ("lam 0", fkind, desc, per)
                        got = _raw(dt, desc, pg, p2, y, kind, B, fw, fv, None, 0, fkind, LAM, den, 0, floor, per=per)
                        assert _same(got, plain, per), ("fn_w NULL", fkind, desc, per)
                        assert not _same(_raw(dt, desc, pg, p2, y, kind, B, fw, fv, tab, K, fkind, LAM, den, 3, floor, per=per), lin, per)


@pytest.mark.parametrize("dtn", list(DTYPES))
def test_the_literal_entry_and_its_descriptor_form_are_the_same_call(dtn):
    dt, B, S, K, Kn = DTYPES[dtn], 6, 65, 33, 17
    pg, ps, y, tab, den = _some(B, S, K, Kn, dt, 25)
    for fkind in FKINDS:
        for per in (True, False):
            a = _raw(dt, False, pg, ps, y, "crystal_rmse", B, None, None, tab, K, fkind, LAM, den, Kn, _floor(dt), per=per)
            b = _raw(dt, True, pg, ps, y, "crystal_rmse", B, None, None, tab, K, fkind, LAM, den, Kn, _floor(dt), per=per)
            c = _run_norm(dt, pg, ps, y, "crystal_rmse", False, BETA, B, tab, den, Kn, _floor(dt), fkind, LAM, per=per)
            assert _same(a, b, per) and _same(a, c, per), (fkind, per)


@pytest.mark.parametrize("dtn", list(DTYPES))
@pytest.mark.parametrize("fkind", FKINDS)
@pytest.mark.parametrize("where", ["predictions", "target"])
def test_zero_sample_weight_takes_a_crystal_out_whatever_it_holds(where, fkind, dtn):
    """Crystal 2 holds a NaN and an inf, w_2 = 0: its rows are +0.0, loss[0] is finite and bitwise the clean value,
    per_crystal[2] is the NaN, every other row is bitwise unchanged."""
    dt, B, S, K, Kn = DTYPES[dtn], 5, 51, 51, 25
    pg, ps, y, tab, den = _some(B, S, K, Kn, dt, 41, which="cumulative")
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
                clean = _run_norm(dt, pg, ps, y, kind, False, BETA, B, tab, den, Kn, _floor(dt), fkind, LAM, w=w, v=fv, per=per)
                bad = _run_norm(dt, bg, bs, by, kind, False, BETA, B, tab, den, Kn, _floor(dt), fkind, LAM, w=w, v=fv, per=per)
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
    """A NaN (or an inf) in crystal 1 reaches its l_b, loss[0] and its rows and no other crystal's rows or per-crystal value."""
    dt, B, S, K, Kn = DTYPES[dtn], 6, 65, 65, 65
    pg, ps, y, tab, den = _some(B, S, K, Kn, dt, 51, which="cumulative")
    others = torch.tensor([0, 2, 3, 4, 5], device=DEV)
    for bad_value in (NAN, math.inf):
        bg = pg.clone()
        bg[1, 3] = bad_value
        for kind in KINDS:
            for per in (True, False):
                clean = _run_norm(dt, pg, ps, y, kind, False, BETA, B, tab, den, Kn, _floor(dt), fkind, LAM, per=per)
                bad = _run_norm(dt, bg, ps, y, kind, False, BETA, B, tab, den, Kn, _floor(dt), fkind, LAM, per=per)
                assert not bool(torch.isfinite(bad.loss).any()) and not bool(torch.isfinite(bad.dpg[1]).all())
                assert torch.equal(_bits(bad.dpg[others]), _bits(clean.dpg[others]))
                assert torch.equal(_bits(bad.dps), _bits(clean.dps))             # (the other output of the same crystal too)
                if per:
                    assert not bool(torch.isfinite(bad.per[1])) and torch.equal(_bits(bad.per[others]), _bits(clean.per[others]))


@pytest.mark.parametrize("dtn", list(DTYPES))
def test_two_runs_are_bitwise_equal(dtn):
    dt, B, S, K, Kn = DTYPES[dtn], 257, 65, 40, 20
    pg, ps, y, tab, den = _some(B, S, K, Kn, dt, 61, clamp=True)
    w, v = _weights(B, S, dt, 61)
    for fkind in FKINDS:
        for kind in KINDS:
            for per in (True, False):
                a = _run_norm(dt, pg, ps, y, kind, True, BETA, B, tab, den, Kn, _floor(dt), fkind, LAM, w=w, v=v, per=per)
                b = _run_norm(dt, pg, ps, y, kind, True, BETA, B, tab, den, Kn, _floor(dt), fkind, LAM, w=w, v=v, per=per)
                assert _same(a, b, per), (fkind, kind, per)


@pytest.mark.parametrize("dtn", list(DTYPES))
@pytest.mark.parametrize("fkind", FKINDS)
def test_a_crystals_numbers_do_not_depend_on_the_batch_or_its_place_in_it(fkind, dtn):
    """The same crystal first in a batch of 1 and last in a batch of 257 (B_global = 257 both times: the coefficient is the
    same number): its gradient rows and its per-crystal value are the same bits - and in the one-workgroup form too.  (The last
    crystal is the floored one; the one before it, not floored, is compared as well.)"""
    dt, B, S, K, Kn = DTYPES[dtn], 257, 51, 51, 26
    pg, ps, y, tab, den = _some(B, S, K, Kn, dt, 71)
    for kind in KINDS:
        big = _run_norm(dt, pg, ps, y, kind, False, BETA, B, tab, den, Kn, _floor(dt), fkind, LAM)
        big_solo = _run_norm(dt, pg, ps, y, kind, False, BETA, B, tab, den, Kn, _floor(dt), fkind, LAM, per=False)
        for at in (B - 1, B - 2):
            cut = slice(at, at + 1)
            one = _run_norm(dt, pg[cut].contiguous(), ps[cut].contiguous(), y[cut].contiguous(), kind, False, BETA, B, tab, den, Kn,
                            _floor(dt), fkind, LAM)
            for got in (big, big_solo):
                assert torch.equal(_bits(got.dpg[cut]), _bits(one.dpg)) and torch.equal(_bits(got.dps[cut]), _bits(one.dps)), kind
            assert torch.equal(_bits(big.per[cut]), _bits(one.per)), kind


# =====================================================================================================================
# 3. the wrappers and the library's refusals
# =====================================================================================================================
def test_wrapper_checks_the_normalised_operands():
    o = _ops()
    pg, ps, y, tab, den = _some(4, 51, 5, 2, torch.float32, 1)
    mk = lambda *s: torch.empty(*s, device=DEV)
    kw = lambda **k: {**dict(dpg=mk(4, 51), dps=mk(4, 51), per_crystal=mk(4), loss=mk(1), functionals=tab, functional_denominator=den,
                             functional_norm_rows=2, functional_floor=1e-3), **k}
    for bad in (den.double(), den.cpu(), None):
        with pytest.raises(TypeError, match="functional_denominator"):
            o.loss_rows(pg, ps, y, "mse", **kw(functional_denominator=bad))
    for bad in (den[:50], mk(102)[::2], mk(1, 51)):
        with pytest.raises(ValueError, match="functional_denominator"):
            o.loss_rows(pg, ps, y, "mse", **kw(functional_denominator=bad))
    for bad in (None, 0.0, -1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="functional_floor"):
            o.loss_rows(pg, ps, y, "mse", **kw(functional_floor=bad))
    for bad in (-1, 6):
        with pytest.raises(ValueError, match="functional_norm_rows"):
            o.loss_rows(pg, ps, y, "mse", **kw(functional_norm_rows=bad))
    with pytest.raises(ValueError, match="functional_norm_rows"):
        o.loss_rows(pg, ps, y, "mse", **kw(functionals=None))
    with pytest.raises(ValueError, match="functional_norm_rows > 0"):
        o.loss_rows(pg, ps, y, "mse", **kw(functional_norm_rows=0))


@pytest.mark.parametrize("dtn", list(DTYPES))
@pytest.mark.parametrize("desc", [False, True], ids=["literal", "descriptor"])
def test_the_library_refuses_with_minus_22_and_its_name(desc, dtn):
    """Every refusal of include/dosx.h on live operands: -22 and a message that starts with the entry's name, before any launch -
    the NaN-filled outputs stay NaN.  (Without a GPU: tests/test_functionals_normalised_host.py.)"""
    import ctypes as C
    from dostransformer_amd import _abi, _lib
    o = _ops()
    lib = _lib.load()
    dt, B, S, K = DTYPES[dtn], 4, 51, 5
    pg, ps, y, tab, den = _some(B, S, K, 2, dt, 1)
    name = "dosx_loss_rows_fn_norm" + ("_desc" if desc else "") + ("" if dt == torch.float32 else "_f64")
    out = Out(B, S, dt)
    ok = dict(tab=tab, K=K, fk=0, lam=LAM, den=den, Kn=2, floor=1e-3)

    def refused(*words, **change):
        a = {**ok, **change}
        head = (pg.data_ptr(), ps.data_ptr(), y.data_ptr(), B, S, B, o.LOSS_KINDS["mse"], 0, BETA, 0.0, out.dpg.data_ptr(),
                out.dps.data_ptr(), out.per.data_ptr(), out.loss.data_ptr(), None, None, None)
        if desc:
            d = _abi.FnNorm()
            d.fn_w, d.fn_den, d.K, d.K_norm, d.fn_kind = o._p(a["tab"]), o._p(a["den"]), a["K"], a["Kn"], a["fk"]
            d.lam, d.den_floor = a["lam"], a["floor"]
            rc = getattr(lib, name)(*head, C.byref(d), o._stream())
        else:
            rc = getattr(lib, name)(*head, o._p(a["tab"]), a["K"], a["fk"], a["lam"], o._p(a["den"]), a["Kn"], a["floor"], o._stream())
        msg = lib.dosx_last_error().decode()
        assert rc == -22 and msg.startswith(name + ":") and all(w in msg for w in words), (rc, msg)

    refused("K_norm=-1", Kn=-1)
    refused("K_norm=6", Kn=6)
    refused("fn_den", "NULL", den=None)
    for floor in (0.0, -1e-3, math.inf, math.nan):
        refused("den_floor", floor=floor)
    refused("fn_den", "inside", den=pg[1])
    refused("fn_den", "inside", den=y[3])
    refused("fn_den", "inside", den=out.dpg[0])
    refused("K=0", K=0)                                        # (what dosx_loss_rows_fn refuses, under this entry's name)
    refused("fn_kind=2", fk=2)
    refused("lam", lam=-1.0)
    refused("fn_w", "inside", tab=ps)
    torch.cuda.synchronize()
    for t in (out.dpg, out.dps, out.per, out.loss):
        assert bool(torch.isnan(t).all())
