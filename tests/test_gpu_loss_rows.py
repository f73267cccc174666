"""dosx_loss_rows / dosx_loss_rows_f64 (csrc/loss_rows.hip) on a real MI355X: the per-crystal RMSE, MSE, MAE and Huber losses with
their gradients against float64 torch autograd on the same rounded inputs.

fp32 is judged element by element with tests/gpu_util.bound_ratio against each element's own scale, the constants derived by
counting roundings (c_rows_grad / c_rows_loss / c_total below; the RMSE kind uses tests/test_gpu_tail.py's c_edos_loss /
c_edos_grad, the algorithm is the same).  float64 is held to the bars tests/test_gpu_train64.py::
test_loss_phonon_f64_against_float64_torch applies to dosx_loss_phonon_f64: losses within 1e-12 relative, a gradient within 1e-10
of its tensor's largest entry - here per crystal row, so a wrong small crystal shows.

The inputs are placed so that the float64 reference is itself unambiguous, and the tests ASSERT that on their inputs: no
residual is 0 (MAE's kink), none lies within 1e-6 delta of +-delta (Huber's branch point) - except the planted ones, which are
exact in both formats."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.gpu_util import DEV, bound_ratio
from tests.test_gpu_tail import _edos_inputs, c_edos_grad, c_edos_loss

pytestmark = pytest.mark.gpu

KINDS = ["crystal_rmse", "mse", "mae", "huber"]
DTYPES = {"f32": torch.float32, "f64": torch.float64}
# every S at B = 5 (idle lanes, exact, one over, a partial fourth stride), every B at S = 51 and 201 (a partial last workgroup of
# four crystals, more than one workgroup, more than one stride of the final 256-thread sum)
SHAPES = [(5, S) for S in (1, 51, 63, 64, 65, 201)] + [(B, S) for S in (51, 201) for B in (1, 3, 4, 7, 130, 257)]
DELTA = 0.0625                     # exact in fp32: the reference and the kernel see the same branch point
NAN = float("nan")


def _ops():
    from dostransformer_amd import ops
    return ops


def f32(v):
    return float(np.float32(v))


# ---- rounding counts (fp32) -------------------------------------------------------------------------------------------------
def c_rows_grad(kind):
    """dp = r k (MSE, Huber's quadratic branch), +-k (MAE), +-delta k (Huber's linear branch), k = [2] [beta] inv_bglobal / S:
    the rounded 1 / B_global, beta inv_bglobal, the division by S (the factor 2 is exact): 3 for k; + the subtraction (one
    rounding of its own result) and the product, or delta k: 5 for MSE and Huber, 3 for MAE (no product, the sign is exact)."""
    return {"mse": 5, "mae": 3, "huber": 5}[kind]


def c_rows_loss(S, kind):
    """l_b = f(pg_b) + beta f(ps_b), f = sum / S, all terms of the sum non-negative (the scale is the value itself): ceil(S / 64)
    additions per lane + 6 reduction levels; per element the subtraction and what follows it - MSE: the subtraction twice under
    the square + the square: 3; MAE: the subtraction: 1; Huber: quadratic 3, linear: |r| - delta / 2 >= |r| / 2 doubles the
    subtraction's error, + its own rounding + the product with delta: 4; + sum / S, beta f, the final sum: 3."""
    return (S + 63) // 64 + 6 + {"mse": 3, "mae": 1, "huber": 4}[kind] + 3


def c_total(B, c_share):
    """loss[0] = sum_b l_b inv_bglobal: the shares' own constant + the rounded 1 / B_global and the product: 2, + ceil(B / 256)
    additions per thread + 6 reduction levels + the 2 levels over the four waves (dosx_sum's order)."""
    return c_share + 2 + (B + 255) // 256 + 6 + 2


def _c(kind, S):
    if kind == "crystal_rmse":
        return c_edos_loss(S), c_edos_grad(S)
    return c_rows_loss(S, kind), c_rows_grad(kind)


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def _inputs(B, S, dt, clamp, seed):
    """Targets with a negative share (clamp_target sets them to 0); predictions t + noise with |noise| spread over 5e-4 .. 3 of
    the target's scale inside EVERY crystal (a wrong small residual shows), never 0.  Seeded on the host: the margins the tests
    assert can be checked without a GPU."""
    g = torch.Generator().manual_seed(seed)
    r = lambda: torch.randn(B, S, generator=g, dtype=torch.float64)
    y = (r() * 0.8).to(dt)
    t = y.double().clamp(min=0.0) if clamp else y.double()
    amp = torch.logspace(-3, 0, B * S, dtype=torch.float64).reshape(S, B).t()
    noise = lambda: (lambda z: torch.sign(z) * (0.5 + z.abs()))(r()) * amp
    pg, ps = (t + noise()).to(dt).contiguous(), (t + noise()).to(dt).contiguous()
    return pg.to(DEV), ps.to(DEV), y.to(DEV)


def _target(y, clamp):
    return y.double().clamp(min=0.0) if clamp else y.double()


def _assert_margins(kind, p, t, planted=None, delta=DELTA):
    """The float64 reference is unambiguous on these inputs: no zero residual under MAE, none within 1e-6 delta of Huber's
    branch point (and both of its branches are populated) - apart from the elements marked `planted`."""
    r = (p.double() - t).abs()
    if planted is not None:
        r = r[~planted]
    if kind == "mae":
        assert float(r.min()) > 0.0
    if kind == "huber":
        assert float((r - delta).abs().min()) > 1e-6 * delta
        assert bool((r < delta).any()) and bool((r > delta).any())


def _f(kind, p, t, delta=DELTA):
    r = p - t
    if kind == "crystal_rmse":
        return torch.sqrt((r ** 2).mean(1))
    if kind == "mse":
        return (r ** 2).mean(1)
    if kind == "mae":
        return r.abs().mean(1)
    return F.huber_loss(p, t, reduction="none", delta=delta).mean(1)


def _elem_scale(kind, p, t, f, S, delta=DELTA):
    """each gradient element's own magnitude, up to the factor w / B_global"""
    r = (p - t).abs()
    if kind == "crystal_rmse":
        return r / (S * f[:, None])
    if kind == "mse":
        return 2.0 * r / S
    if kind == "mae":
        return torch.full_like(r, 1.0 / S)
    return r.clamp(max=delta) / S


def _ref(kind, pg, ps, y, clamp, beta, Bg, delta=DELTA):
    """float64 autograd on the same inputs: (l_b [B], loss, dpg, dps or None, scale of dpg, scale of dps or None)"""
    t = _target(y, clamp)
    a = pg.detach().double().clone().requires_grad_(True)           # (a fresh leaf: .double() of a float64 tensor is the tensor itself)
    fa = _f(kind, a, t, delta)
    l, b = fa, None
    if ps is not None:
        b = ps.detach().double().clone().requires_grad_(True)
        fb = _f(kind, b, t, delta)
        l = fa + beta * fb
    loss = l.sum() / Bg
    loss.backward()
    S = pg.shape[1]
    sa = _elem_scale(kind, a.detach(), t, fa.detach(), S, delta) / Bg
    sb = None if ps is None else _elem_scale(kind, b.detach(), t, fb.detach(), S, delta) * (beta / Bg)
    return l.detach(), loss.detach(), a.grad, None if b is None else b.grad, sa, sb


class Out:
    """NaN-filled outputs: dpg / dps rows 1 .. B of larger [B + 2, S] buffers, per_crystal and loss inside longer vectors."""

    def __init__(self, B, S, dt, two=True, per=True):
        nan = lambda *s: torch.full(s, NAN, dtype=dt, device=DEV)
        self.B, self.bufs = B, [nan(B + 2, S) for _ in range(2 if two else 1)]
        self.dpg, self.dps = self.bufs[0][1:B + 1], (self.bufs[1][1:B + 1] if two else None)
        self.pbuf, self.lbuf = nan(B + 8), nan(9)
        self.per, self.loss = (self.pbuf[4:4 + B] if per else None), self.lbuf[4:5]

    def check_outside(self):
        for b in self.bufs:
            assert bool(torch.isnan(b[0]).all()) and bool(torch.isnan(b[self.B + 1]).all()), "written outside the gradient rows"
        assert bool(torch.isnan(self.pbuf[:4]).all()) and bool(torch.isnan(self.pbuf[4 + self.B:]).all())
        assert bool(torch.isnan(self.lbuf[:4]).all()) and bool(torch.isnan(self.lbuf[5:]).all())
        if self.per is None:
            assert bool(torch.isnan(self.pbuf).all())


def _run(dt, pg, ps, y, kind, clamp, beta, Bg, per=True, delta=DELTA):
    B, S = pg.shape
    out = Out(B, S, dt, two=ps is not None, per=per)
    fn = _ops().loss_rows if dt == torch.float32 else _ops().loss_rows64
    fn(pg, ps, y, kind, clamp_target=clamp, beta=beta, delta=delta if kind == "huber" else None, dpg=out.dpg, dps=out.dps,
       per_crystal=out.per, loss=out.loss, B_global=Bg)
    torch.cuda.synchronize()
    out.check_outside()
    return out


def _rows_relmax(got, ref):
    """worst, over the crystals, error of a gradient row relative to the row's largest entry (an all-zero row must be exact)"""
    d, m = (got.double() - ref).abs().amax(1), ref.abs().amax(1)
    assert not bool(torch.isnan(d).any())
    assert bool((d[m == 0] == 0).all())
    return float((d[m > 0] / m[m > 0]).max()) if bool((m > 0).any()) else 0.0


def _judge(dt, kind, out, ref, B, S, tag, rows=None):
    """out against the reference (l, loss, ga, gb, sa, sb); rows: the crystals to judge (default all, and then loss[0] too)"""
    l, loss, ga, gb, sa, sb = ref
    sel = slice(None) if rows is None else rows
    pairs = [("dpg", out.dpg[sel], ga, sa)] + ([("dps", out.dps[sel], gb, sb)] if gb is not None else [])
    if dt == torch.float32:
        c_loss, c_grad = _c(kind, S)
        for name, got, g, s in pairs:
            assert bound_ratio(got, g, s, c_grad, f"{tag}.{name}") <= 1.0
        if out.per is not None:
            assert bound_ratio(out.per[sel], l, l, c_loss, tag + ".per_crystal") <= 1.0
        if rows is None:
            assert bound_ratio(out.loss, loss[None], loss[None], c_total(B, c_loss), tag + ".loss") <= 1.0
    else:
        e = [_rows_relmax(got, g) for _, got, g, _ in pairs]
        e_per = float(((out.per[sel] - l).abs() / l).max()) if out.per is not None else 0.0
        e_loss = abs(float(out.loss) - float(loss)) / float(loss) if rows is None else 0.0
        print(f"{tag}: loss {e_loss:.2e}  per_crystal {e_per:.2e}  gradients {max(e):.2e}")
        assert e_loss <= 1e-12 and e_per <= 1e-12 and max(e) <= 1e-10, (e_loss, e_per, e)


@pytest.mark.parametrize("dtn", list(DTYPES))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,S", SHAPES)
def test_loss_rows_against_float64_autograd(B, S, kind, dtn):
    """beta in {0.7, 0}, clamp_target in {0, 1}, B_global in {B, 3 B}; the one-output form; per_crystal = NULL (one launch, the
    same bits as the two); two launches on the same inputs are bitwise equal."""
    dt = DTYPES[dtn]
    for clamp in (False, True):
        pg, ps, y = _inputs(B, S, dt, clamp, 1000 * B + S + (7 if clamp else 0))
        t = _target(y, clamp)
        if clamp and B * S >= 8:
            assert bool((y < 0).any())
        _assert_margins(kind, pg, t)
        _assert_margins(kind, ps, t)
        first = None
        for beta in (0.7, 0.0):
            bk = f32(beta) if dt == torch.float32 else beta          # what the kernel reads
            for Bg in (B, 3 * B):
                tag = f"loss_rows[{dtn},{kind},B{B},S{S},clamp{int(clamp)},beta{beta:g},global{Bg}]"
                out = _run(dt, pg, ps, y, kind, clamp, beta, Bg)
                assert not bool(torch.isnan(out.dpg).any() | torch.isnan(out.dps).any() | torch.isnan(out.per).any())
                _judge(dt, kind, out, _ref(kind, pg, ps, y, clamp, bk, Bg), B, S, tag)
                if beta == 0.0:
                    assert bool((out.dps == 0).all())
                nop = _run(dt, pg, ps, y, kind, clamp, beta, Bg, per=False)
                for a, b in ((out.dpg, nop.dpg), (out.dps, nop.dps), (out.loss, nop.loss)):
                    assert torch.equal(a, b), tag + " per_crystal=None"
                if first is None:
                    first = out
                    again = _run(dt, pg, ps, y, kind, clamp, beta, Bg)
                    for a, b in ((out.dpg, again.dpg), (out.dps, again.dps), (out.per, again.per), (out.loss, again.loss)):
                        assert torch.equal(a, b), tag + " run to run"
        for Bg in (B, 3 * B):                                       # one output: ps = dps = None, beta not read
            tag = f"loss_rows[{dtn},{kind},B{B},S{S},clamp{int(clamp)},one-output,global{Bg}]"
            for per in (True, False):
                out = _run(dt, pg, None, y, kind, clamp, 123.0, Bg, per=per)
                _judge(dt, kind, out, _ref(kind, pg, None, y, clamp, 0.0, Bg), B, S, tag)


@pytest.mark.parametrize("B,S", [(1, 201), (5, 64), (7, 201), (130, 63)])
def test_rmse_with_clamp_is_bitwise_loss_edos_and_sum(B, S):
    """The yardstick against the code that exists: kind = RMSE, clamp_target, two outputs, fp32 - dpg, dps, the shares times
    1 / B_global and loss[0] are the bits of ops.loss_edos + ops.sum_to."""
    o = _ops()
    pg, ps, yft = _edos_inputs(B, S, 211)
    for beta in (0.7, 0.0):
        for Bg in (B, 3 * B):
            dpg, dps, lp = (torch.full(s, NAN, device=DEV) for s in ((B, S), (B, S), (B + 1,)))
            o.loss_edos(pg, ps, yft, beta, B, S, Bg, dpg, dps, lp)
            o.sum_to(lp, B, lp[B:])
            out = _run(torch.float32, pg, ps, yft, "crystal_rmse", True, beta, Bg)
            inv = torch.ones(1, device=DEV) / torch.full((1,), float(Bg), device=DEV)          # 1.f / (float)B_global
            assert torch.equal(out.dpg, dpg) and torch.equal(out.dps, dps), (B, S, beta, Bg)
            assert torch.equal(out.per * inv, lp[:B]) and torch.equal(out.loss, lp[B:]), (B, S, beta, Bg)
            nop = _run(torch.float32, pg, ps, yft, "crystal_rmse", True, beta, Bg, per=False)
            assert torch.equal(nop.dpg, dpg) and torch.equal(nop.dps, dps) and torch.equal(nop.loss, lp[B:])


@pytest.mark.parametrize("dtn", list(DTYPES))
@pytest.mark.parametrize("kind", KINDS)
def test_planted_cases(kind, dtn):
    """pg == t over a whole crystal: zero gradient row (RMSE: the zero rule, never 0 / 0) and a share of exactly beta f(ps); one
    r == 0 under MAE: gradient exactly 0; |r| == delta under Huber: the quadratic branch, r / (S B_global) to the bound."""
    dt, B, S, beta = DTYPES[dtn], 5, 51, 0.7
    bk = f32(beta) if dt == torch.float32 else beta
    delta = 0.25
    pg, ps, y = _inputs(B, S, dt, False, 4242)
    pg[1] = y[1]                                                     # crystal 1 predicted exactly by the first output
    y[3, 5] = y[3, 6] = 0.5
    pg[3, 5], pg[3, 6] = 0.75, 0.25                                  # r = +delta, -delta: exact in both formats
    pg[0, 3] = y[0, 3]                                               # one r == 0
    planted = torch.zeros(B, S, dtype=torch.bool, device=DEV)
    planted[1], planted[3, 5], planted[3, 6], planted[0, 3] = True, True, True, True
    _assert_margins(kind, pg, y.double(), planted, delta)
    _assert_margins(kind, ps, y.double(), None, delta)
    out = _run(dt, pg, ps, y, kind, False, beta, B, delta=delta)
    assert bool((out.dpg[1] == 0).all())
    solo = _run(dt, ps, None, y, kind, False, 0.0, B, delta=delta)  # f(ps_b) as the kernel computes it
    assert torch.equal(out.per[1:2], torch.tensor([bk], dtype=dt, device=DEV) * solo.per[1:2])
    assert float(out.dpg[0, 3]) == 0.0
    if kind == "mae":
        assert bool((out.dpg[0, :3] != 0).all())
    # the reference: a zero residual is where autograd differs by convention (sqrt'(0), sign(0) = 0 agree with torch for MAE;
    # RMSE gives NaN there), so crystal 1 is judged above and the others here; torch's huber_loss takes |r| <= delta quadratic
    rows = torch.tensor([0, 2, 3, 4], device=DEV)
    ref = _ref(kind, pg[rows], ps[rows], y[rows], False, bk, B, delta)
    if kind == "huber":
        for j, sgn in ((5, 1.0), (6, -1.0)):
            assert abs(float(ref[2][2, j]) - sgn * 0.25 / (S * B)) <= 1e-15          # row 3 is the reference's row 2
            if dt == torch.float32:
                want = torch.tensor([sgn * 0.25 / (S * B)], dtype=torch.float64, device=DEV)
                assert bound_ratio(out.dpg[3, j][None], want, want.abs(), c_rows_grad("huber"), f"huber |r| == delta [{j}]") <= 1.0
    _judge(dt, kind, out, ref, B, S, f"planted[{dtn},{kind}]", rows=rows)


@pytest.mark.parametrize("dtn", list(DTYPES))
@pytest.mark.parametrize("kind", KINDS)
def test_nonfinite_predictions_stay_in_their_crystal(kind, dtn):
    """A NaN and a +inf prediction in crystal 2 (both outputs): loss[0], per_crystal[2] and that crystal's gradient rows are not
    finite - the step guard sees them -, every other crystal's rows are finite and within the bound."""
    dt, B, S, beta = DTYPES[dtn], 5, 51, 0.7
    bk = f32(beta) if dt == torch.float32 else beta
    pg, ps, y = _inputs(B, S, dt, False, 777)
    pg[2, 4], pg[2, 9], ps[2, 5], ps[2, 11] = NAN, math.inf, math.inf, NAN
    rows = torch.tensor([0, 1, 3, 4], device=DEV)
    _assert_margins(kind, pg[rows], y.double()[rows])
    _assert_margins(kind, ps[rows], y.double()[rows])
    for per in (True, False):
        out = _run(dt, pg, ps, y, kind, False, beta, B, per=per)
        assert not bool(torch.isfinite(out.loss).any())
        assert not bool(torch.isfinite(out.dpg[2]).all()) and not bool(torch.isfinite(out.dps[2]).all())
        assert bool(torch.isfinite(out.dpg[rows]).all()) and bool(torch.isfinite(out.dps[rows]).all())
        if per:
            assert not bool(torch.isfinite(out.per[2])) and bool(torch.isfinite(out.per[rows]).all())
        _judge(dt, kind, out, _ref(kind, pg[rows], ps[rows], y[rows], False, bk, B), B, S, f"nonfinite[{dtn},{kind}]", rows=rows)


def test_nan_target_under_clamp_becomes_zero():
    """The one documented exception (as dosx_loss_edos): the clamp is fmax(y, 0), which turns a NaN TARGET into 0; without the
    clamp the NaN reaches the loss."""
    B, S = 3, 51
    pg, ps, y = _inputs(B, S, torch.float32, True, 99)
    y0 = y.clone()
    y[1, 7], y0[1, 7] = NAN, 0.0
    a, b = _run(torch.float32, pg, ps, y, "mse", True, 0.7, B), _run(torch.float32, pg, ps, y0, "mse", True, 0.7, B)
    assert torch.equal(a.dpg, b.dpg) and torch.equal(a.dps, b.dps) and torch.equal(a.per, b.per) and torch.equal(a.loss, b.loss)
    c = _run(torch.float32, pg, ps, y, "mse", False, 0.7, B)
    assert not bool(torch.isfinite(c.loss).any()) and not bool(torch.isfinite(c.per[1]))


def test_wrapper_checks_dtype_layout_and_names():
    """The wrappers refuse what the kernels cannot index: another dtype, a non-contiguous output (a column slice - row slices of a
    larger table are contiguous and are what every test above passes), a wrong element count, an unknown kind."""
    o = _ops()
    pg, ps, y = _inputs(4, 51, torch.float32, False, 1)
    mk = lambda *s: torch.empty(*s, device=DEV)
    kw = lambda **k: {**dict(dpg=mk(4, 51), dps=mk(4, 51), per_crystal=mk(4), loss=mk(1)), **k}
    with pytest.raises(TypeError):
        o.loss_rows(pg.double(), ps, y, "mse", **kw())
    with pytest.raises(TypeError):
        o.loss_rows64(pg, ps, y, "mse", **kw())
    with pytest.raises(ValueError, match="contiguous"):
        o.loss_rows(pg, ps, y, "mse", **kw(dpg=mk(4, 102)[:, :51]))
    with pytest.raises(ValueError):
        o.loss_rows(pg, ps[:3], y, "mse", **kw())
    with pytest.raises(ValueError):
        o.loss_rows(pg, None, y, "mse", **kw())                      # ps without dps
    with pytest.raises(ValueError, match="crystal_rmse"):
        o.loss_rows(pg, ps, y, "rmse", **kw())
    for bad in (None, 0.0, -1.0, math.inf):
        with pytest.raises(ValueError, match="delta"):
            o.loss_rows(pg, ps, y, "huber", delta=bad, **kw())
