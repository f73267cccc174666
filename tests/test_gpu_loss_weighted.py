"""dosx_loss_rows_w / dosx_loss_rows_w_f64 (csrc/loss_rows.hip) on a real MI355X: the per-crystal losses under sample weights
``w_b`` and energy-bin weights ``v_s`` against float64 torch autograd of the definition in include/dosx.h, computed on the CPU
on the same rounded inputs -

    V = sum_s v_s,  f(p_b) = [sqrt] (sum_s v_s e(r) / V),  l_b = f(pg_b) + beta f(ps_b),  loss[0] = sum_b w_b l_b / B_global

- and what holds bit for bit by construction: the gather out of a table, all-ones weights, a doubled weight, a zero weight,
run to run.

Inputs, margins (no residual on MAE's kink or Huber's branch point) and the judge are tests/test_gpu_loss_rows.py's: fp32 element
by element against each element's own scale - here multiplied by ``w_b`` and, with bin weights, by ``v_s S / V`` -, float64 1e-12
relative for the loss and the per-crystal values and 1e-10 of the row's largest entry for the gradient rows.

The fp32 constants are that file's rounding counts plus the roundings the weighted forms add (``_judge_w``), counted the same way:
with ``w`` the product ``w_b / B_global`` in the coefficient and ``l_b w_b`` in the share, one each; with ``bin_w`` the product
``v_s x`` on every element of sum and gradient, one each, and ``V`` in place of the exact ``S`` - a sum of S non-negative numbers
in ceil(S / 64) additions per lane and 6 reduction levels, each at most one unit of its own value."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.gpu_util import DEV, bound_ratio
from tests.test_gpu_loss_rows import (DELTA, DTYPES, KINDS, NAN, Out, _assert_margins, _c, _elem_scale, _inputs, _judge, _ops,
                                      _run, _target, c_total, f32)

pytestmark = pytest.mark.gpu

# S over the lane boundaries at B = 5; B over the four-crystals-per-workgroup edge and the one-workgroup form's 256 at S = 51
SHAPES = [(5, S) for S in (1, 63, 64, 65, 201)] + [(B, 51) for B in (1, 3, 4, 257)]
BETA = 0.7


@pytest.fixture(scope="module", autouse=True)
def _own_memory_pool():
    """The tests of this module allocate from a memory pool of their own, given back when the module is done: what the rest of the
    suite finds in torch's caching allocator - which free block a later test's tensor lands in - does not depend on this file."""
    pool = torch.cuda.MemPool()
    with torch.cuda.use_mem_pool(pool):
        yield
    torch.cuda.synchronize()
    del pool


def _seed(B, S, clamp):
    return 1000 * B + S + (7 if clamp else 0)                  # test_loss_rows_against_float64_autograd's inputs


def _weights(B, S, dt, seed):
    """w in [0.25, 4] (log-uniform), v in [0, 2] with a few exact zeros where there are bins to spare; rounded to dt on the host"""
    g = torch.Generator().manual_seed(seed + 5)
    w = (0.25 * 16.0 ** torch.rand(B, generator=g, dtype=torch.float64)).to(dt)
    v = (2.0 * torch.rand(S, generator=g, dtype=torch.float64)).clamp(min=1e-3)
    if S >= 8:
        v[torch.tensor([0, S // 3, S - 2])] = 0.0
    v = v.to(dt)
    assert float(w.min()) >= 0.25 and float(w.max()) <= 4.0 and float(v.max()) <= 2.0 and float(v.sum()) > 0
    assert int((v == 0).sum()) == (3 if S >= 8 else 0)
    return w.to(DEV), v.to(DEV)


def _f_w(kind, p, t, v, delta=DELTA):
    """f(p_b) of the definition; v None: unweighted"""
    r = p - t
    if kind in ("crystal_rmse", "mse"):
        e = r ** 2
    elif kind == "mae":
        e = r.abs()
    else:
        e = F.huber_loss(p, t, reduction="none", delta=delta)
    m = e.mean(1) if v is None else (e * v).sum(1) / v.sum()
    return torch.sqrt(m) if kind == "crystal_rmse" else m


def _ref_w(kind, pg, ps, y, clamp, beta, Bg, w, v, delta=DELTA):
    """float64 autograd ON THE CPU: (l_b, loss, dpg, dps or None, scale of dpg, scale of dps or None), moved to the device for
    the judge.  The scales: test_gpu_loss_rows._elem_scale's times w_b / B_global, and times v_s S / V under bin weights."""
    cpu = lambda x: None if x is None else x.detach().cpu().double()
    y, w, v = cpu(y), cpu(w), cpu(v)
    t = _target(y, clamp)
    S = pg.shape[1]
    a = cpu(pg).clone().requires_grad_(True)
    fa = _f_w(kind, a, t, v, delta)
    l, b, fb = fa, None, None
    if ps is not None:
        b = cpu(ps).clone().requires_grad_(True)
        fb = _f_w(kind, b, t, v, delta)
        l = fa + beta * fb
    wl = l if w is None else w * l
    loss = wl.sum() / Bg
    loss.backward()
    row = (torch.ones(pg.shape[0], dtype=torch.float64) if w is None else w)[:, None] / Bg
    col = 1.0 if v is None else (v * S / v.sum())[None, :]
    sa = _elem_scale(kind, a.detach(), t, fa.detach(), S, delta) * row * col
    sb = None if b is None else _elem_scale(kind, b.detach(), t, fb.detach(), S, delta) * row * col * beta
    dev = lambda x: None if x is None else x.to(DEV)
    return dev(l.detach()), dev(loss.detach()), dev(a.grad), dev(None if b is None else b.grad), dev(sa), dev(sb)


def _run_w(dt, pg, ps, y, kind, clamp, beta, Bg, w=None, wi=None, v=None, per=True, delta=DELTA):
    B, S = pg.shape
    out = Out(B, S, dt, two=ps is not None, per=per)
    fn = _ops().loss_rows if dt == torch.float32 else _ops().loss_rows64
    fn(pg, ps, y, kind, clamp_target=clamp, beta=beta, delta=delta if kind == "huber" else None, dpg=out.dpg, dps=out.dps,
       per_crystal=out.per, loss=out.loss, B_global=Bg, weights=w, weight_index=wi, bin_weights=v)
    torch.cuda.synchronize()
    out.check_outside()
    return out


def _judge_w(dt, kind, out, ref, B, S, tag, has_w, has_v):
    """test_gpu_loss_rows._judge with the weighted forms' roundings added to its fp32 constants (module docstring); float64: its
    bars as they are."""
    if dt != torch.float32:
        return _judge(dt, kind, out, ref, B, S, tag)
    l, loss, ga, gb, sa, sb = ref
    c_loss, c_grad = _c(kind, S)
    c_v = (S + 63) // 64 + 6                                      # V: additions per lane + reduction levels
    c_grad += int(has_w) + (1 + c_v + (1 if kind == "crystal_rmse" else 0) if has_v else 0)     # (RMSE: v_s also inside the sum)
    c_loss += 1 + c_v if has_v else 0
    for name, got, g, sc in [("dpg", out.dpg, ga, sa)] + ([("dps", out.dps, gb, sb)] if gb is not None else []):
        assert bound_ratio(got, g, sc, c_grad, f"{tag}.{name}") <= 1.0
    if out.per is not None:
        assert bound_ratio(out.per, l, l, c_loss, tag + ".per_crystal") <= 1.0
    assert bound_ratio(out.loss, loss[None], loss[None], c_total(B, c_loss) + int(has_w), tag + ".loss") <= 1.0


def _same(a, b, per=True):
    ok = torch.equal(a.dpg, b.dpg) and torch.equal(a.loss, b.loss) and (a.dps is None or torch.equal(a.dps, b.dps))
    return ok and (not per or torch.equal(a.per, b.per))


def _bits(x):
    return x.view(torch.int32 if x.dtype == torch.float32 else torch.int64)


# =====================================================================================================================
# 1. against float64 autograd of the definition
# =====================================================================================================================
@pytest.mark.parametrize("dtn", list(DTYPES))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,S", SHAPES)
def test_weighted_loss_against_float64_autograd(B, S, kind, dtn):
    """clamp_target in {0, 1} (B_global = B, 3 B), the three forms (w, v, w and v), two outputs and one, per_crystal set and
    NULL (one launch: the same bits as the two)."""
    dt = DTYPES[dtn]
    bk = f32(BETA) if dt == torch.float32 else BETA              # what the kernel reads
    for clamp, Bg in ((False, B), (True, 3 * B)):
        pg, ps, y = _inputs(B, S, dt, clamp, _seed(B, S, clamp))
        t = _target(y, clamp)
        _assert_margins(kind, pg, t)
        _assert_margins(kind, ps, t)
        w, v = _weights(B, S, dt, _seed(B, S, clamp))
        for form, (fw, fv) in (("w", (w, None)), ("v", (None, v)), ("wv", (w, v))):
            for two in (True, False):
                p2 = ps if two else None
                tag = f"loss_rows_w[{dtn},{kind},B{B},S{S},clamp{int(clamp)},{form},{'two' if two else 'one'}]"
                ref = _ref_w(kind, pg, p2, y, clamp, bk if two else 0.0, Bg, fw, fv)
                out = _run_w(dt, pg, p2, y, kind, clamp, BETA, Bg, w=fw, v=fv)
                assert not bool(torch.isnan(out.dpg).any() | torch.isnan(out.per).any() | torch.isnan(out.loss).any())
                _judge_w(dt, kind, out, ref, B, S, tag, fw is not None, fv is not None)
                if fv is not None:                                # a bin of weight 0 is out of the gradient, exactly
                    zero = fv == 0
                    assert bool((out.dpg[:, zero] == 0).all()) and (not two or bool((out.dps[:, zero] == 0).all()))
                nop = _run_w(dt, pg, p2, y, kind, clamp, BETA, Bg, w=fw, v=fv, per=False)
                assert _same(out, nop, per=False), tag + " per_crystal=None"


def test_per_crystal_is_the_unweighted_loss_of_the_crystal():
    """per_crystal[b] is NOT multiplied by w_b: under sample weights alone it is the unweighted entry's, bit for bit, and the
    gradient rows of a crystal are the unweighted ones times w_b to rounding (one more product in the coefficient)."""
    B, S = 7, 51
    for dtn, dt in DTYPES.items():
        pg, ps, y = _inputs(B, S, dt, False, 31)
        w, _ = _weights(B, S, dt, 31)
        for kind in KINDS:
            plain = _run(dt, pg, ps, y, kind, False, BETA, B)
            out = _run_w(dt, pg, ps, y, kind, False, BETA, B, w=w)
            assert torch.equal(out.per, plain.per), (dtn, kind)
            assert not torch.equal(out.dpg, plain.dpg)
            rel = ((out.dpg.double() - plain.dpg.double() * w.double()[:, None]).abs() / out.dpg.double().abs()).max()
            # the coefficient of either side carries four roundings, the last product of each one more: 2 x 4 units at the most
            assert float(rel) <= (8 * 2.0 ** -24 if dt == torch.float32 else 8 * 2.0 ** -53), (dtn, kind, float(rel))


# =====================================================================================================================
# 2. bit for bit by construction
# =====================================================================================================================
@pytest.mark.parametrize("dtn", list(DTYPES))
def test_gather_out_of_a_table_is_bitwise_the_ungathered_call(dtn):
    dt, B, S = DTYPES[dtn], 9, 51
    pg, ps, y = _inputs(B, S, dt, False, 77)
    g = torch.Generator().manual_seed(3)
    table = (0.25 + 3.75 * torch.rand(300, generator=g, dtype=torch.float64)).to(dt).to(DEV)
    table[17] = 0.0
    sel = torch.tensor([299, 0, 17, 150, 150, 3, 299, 42, 0], dtype=torch.int32, device=DEV)      # repeats, both ends, a zero
    picked = table[sel.long()].contiguous()
    _, v = _weights(B, S, dt, 77)
    for kind in KINDS:
        for fv in (None, v):
            for per in (True, False):
                for p2 in (ps, None):
                    a = _run_w(dt, pg, p2, y, kind, False, BETA, B, w=table, wi=sel, v=fv, per=per)
                    b = _run_w(dt, pg, p2, y, kind, False, BETA, B, w=picked, v=fv, per=per)
                    assert _same(a, b, per), (kind, fv is not None, per, p2 is not None)
                    assert bool((a.dpg[2] == 0).all()) and not bool((a.dpg[3] == 0).all())


@pytest.mark.parametrize("dtn", list(DTYPES))
@pytest.mark.parametrize("kind", KINDS)
def test_all_ones_is_bitwise_the_unweighted_entry(kind, dtn):
    """w = 1 with bin_w = None: multiplying by 1.0 is exact - loss, per-crystal values and both gradients are ops.loss_rows's."""
    dt = DTYPES[dtn]
    for B, S in ((5, 65), (257, 51)):
        for clamp in (False, True):
            pg, ps, y = _inputs(B, S, dt, clamp, _seed(B, S, clamp))
            ones = torch.ones(B, dtype=dt, device=DEV)
            table, sel = torch.ones(3, dtype=dt, device=DEV), (torch.arange(B, dtype=torch.int32, device=DEV) % 3).contiguous()
            for Bg in (B, 3 * B):
                for p2 in (ps, None):
                    for per in (True, False):
                        plain = _run(dt, pg, p2, y, kind, clamp, BETA, Bg, per=per)
                        assert _same(_run_w(dt, pg, p2, y, kind, clamp, BETA, Bg, w=ones, per=per), plain, per), (B, S, clamp, Bg, per)
                        assert _same(_run_w(dt, pg, p2, y, kind, clamp, BETA, Bg, w=table, wi=sel, per=per), plain, per)


@pytest.mark.parametrize("dtn", list(DTYPES))
@pytest.mark.parametrize("kind", KINDS)
def test_doubling_one_weight_doubles_that_crystals_rows_and_nothing_else(kind, dtn):
    """A power-of-two scale is exact in every operation on the path (inputs of order 1: nothing near the subnormals)."""
    dt, B, S = DTYPES[dtn], 6, 65
    pg, ps, y = _inputs(B, S, dt, False, 55)
    w, v = _weights(B, S, dt, 55)
    w2 = w.clone()
    w2[4] = w[4] * 2
    others = torch.tensor([0, 1, 2, 3, 5], device=DEV)
    for fv in (None, v):
        for per in (True, False):
            a = _run_w(dt, pg, ps, y, kind, False, BETA, B, w=w, v=fv, per=per)
            b = _run_w(dt, pg, ps, y, kind, False, BETA, B, w=w2, v=fv, per=per)
            assert torch.equal(b.dpg[4], 2 * a.dpg[4]) and torch.equal(b.dps[4], 2 * a.dps[4]), (kind, per)
            assert bool((a.dpg[4] != 0).any())
            assert torch.equal(b.dpg[others], a.dpg[others]) and torch.equal(b.dps[others], a.dps[others])
            if per:
                assert torch.equal(a.per, b.per)                      # the crystals' own losses do not know their weights
            assert float(b.loss) > float(a.loss)


@pytest.mark.parametrize("dtn", list(DTYPES))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("where", ["predictions", "target"])
def test_zero_weight_takes_a_crystal_out_whatever_it_holds(where, kind, dtn):
    """Crystal 2 holds a NaN and an inf (in both predictions, or in its target), w_2 = 0: its gradient rows are +0.0, loss[0] is
    finite and bitwise the value with ordinary numbers there, per_crystal[2] is the NaN, every other row is bitwise unchanged."""
    dt, B, S = DTYPES[dtn], 5, 51
    pg, ps, y = _inputs(B, S, dt, False, 777)
    w, v = _weights(B, S, dt, 777)
    w[2] = 0.0
    bg, bs, by = pg.clone(), ps.clone(), y.clone()
    if where == "predictions":
        bg[2, 4], bg[2, 9], bs[2, 5], bs[2, 11] = NAN, math.inf, math.inf, NAN
    else:
        by[2, 4], by[2, 9] = NAN, -math.inf
    others = torch.tensor([0, 1, 3, 4], device=DEV)
    table = torch.cat([w, w.new_full((3,), 9.0)])
    sel = torch.arange(B, dtype=torch.int32, device=DEV)
    for fv in (None, v):
        for per in (True, False):
            for kw in (dict(w=w), dict(w=table, wi=sel)):
                clean = _run_w(dt, pg, ps, y, kind, False, BETA, B, v=fv, per=per, **kw)
                bad = _run_w(dt, bg, bs, by, kind, False, BETA, B, v=fv, per=per, **kw)
                for o in (clean, bad):
                    for d in (o.dpg, o.dps):
                        assert bool((_bits(d[2]) == 0).all()), (kind, per)           # +0.0: every bit clear
                assert bool(torch.isfinite(bad.loss).all()) and torch.equal(bad.loss, clean.loss)
                assert torch.equal(bad.dpg[others], clean.dpg[others]) and torch.equal(bad.dps[others], clean.dps[others])
                if per:
                    assert bool(torch.isnan(bad.per[2])) and bool(torch.isfinite(clean.per[2]))
                    assert torch.equal(bad.per[others], clean.per[others])
    # input condition: with w_2 = 1 the same batch poisons loss[0] and the crystal's rows
    w[2] = 1.0
    hot = _run_w(dt, bg, bs, by, kind, False, BETA, B, w=w)
    assert not bool(torch.isfinite(hot.loss).any()) and not bool(torch.isfinite(hot.dpg[2]).all())


def test_a_nan_in_a_bin_of_weight_zero_is_out_of_sums_and_gradients():
    dt, B, S = torch.float32, 4, 51
    pg, ps, y = _inputs(B, S, dt, False, 12)
    _, v = _weights(B, S, dt, 12)
    zero = int((v == 0).nonzero()[1])
    bg = pg.clone()
    bg[1, zero] = NAN
    for kind in KINDS:
        a, b = _run_w(dt, pg, ps, y, kind, False, BETA, B, v=v), _run_w(dt, bg, ps, y, kind, False, BETA, B, v=v)
        assert _same(a, b), kind


@pytest.mark.parametrize("dtn", list(DTYPES))
def test_two_runs_are_bitwise_equal(dtn):
    dt, B, S = DTYPES[dtn], 257, 65
    pg, ps, y = _inputs(B, S, dt, True, 5)
    w, v = _weights(B, S, dt, 5)
    table = torch.cat([w, w.flip(0)])
    sel = (torch.arange(B, dtype=torch.int32, device=DEV) * 2).contiguous()
    for kind in KINDS:
        for per in (True, False):
            a = _run_w(dt, pg, ps, y, kind, True, BETA, B, w=table, wi=sel, v=v, per=per)
            b = _run_w(dt, pg, ps, y, kind, True, BETA, B, w=table, wi=sel, v=v, per=per)
            assert _same(a, b, per), (kind, per)


# =====================================================================================================================
# 3. the wrappers
# =====================================================================================================================
def test_wrapper_checks_the_weights():
    o = _ops()
    pg, ps, y = _inputs(4, 51, torch.float32, False, 1)
    mk = lambda *s: torch.empty(*s, device=DEV)
    kw = lambda **k: {**dict(dpg=mk(4, 51), dps=mk(4, 51), per_crystal=mk(4), loss=mk(1)), **k}
    w, v, wi = torch.ones(4, device=DEV), torch.ones(51, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    with pytest.raises(TypeError, match="weights"):
        o.loss_rows(pg, ps, y, "mse", **kw(weights=w.double()))
    with pytest.raises(TypeError, match="weights"):
        o.loss_rows(pg, ps, y, "mse", **kw(weights=w.cpu()))
    with pytest.raises(TypeError, match="weights"):
        o.loss_rows64(pg.double(), ps.double(), y.double(), "mse", dpg=mk(4, 51).double(), dps=mk(4, 51).double(),
                      loss=mk(1).double(), weights=w)
    with pytest.raises(ValueError, match="weight_index"):
        o.loss_rows(pg, ps, y, "mse", **kw(weights=torch.ones(9, device=DEV)))           # a table without its selection
    with pytest.raises(ValueError, match="weights"):
        o.loss_rows(pg, ps, y, "mse", **kw(weights=torch.ones(8, device=DEV)[::2]))
    with pytest.raises(ValueError, match="weight_index"):
        o.loss_rows(pg, ps, y, "mse", **kw(weight_index=wi))                             # a selection without its table
    with pytest.raises(TypeError, match="weight_index"):
        o.loss_rows(pg, ps, y, "mse", **kw(weights=w, weight_index=wi.long()))
    with pytest.raises(ValueError, match="weight_index"):
        o.loss_rows(pg, ps, y, "mse", **kw(weights=w, weight_index=wi[:3]))
    with pytest.raises(TypeError, match="bin_weights"):
        o.loss_rows(pg, ps, y, "mse", **kw(bin_weights=v.double()))
    with pytest.raises(ValueError, match="bin_weights"):
        o.loss_rows(pg, ps, y, "mse", **kw(bin_weights=v[:50]))
    with pytest.raises(ValueError, match="bin_weights"):
        o.loss_rows(pg, ps, y, "mse", **kw(bin_weights=torch.ones(102, device=DEV)[::2]))
    # (the library's own refusals - w_index without w, w or bin_w inside an operand: tests/test_loss_weighted_abi.py, without a GPU)
