"""The tail of every training step - the final LayerNorm family, the losses (csrc/rowops.hip), the flat AdamW step (csrc/adamw.hip) and the small
utilities around them (csrc/graph_ops.hip: embed / reduce rows, act_bwd, graph pooling, seg_count_scale) - each kernel called
directly and held element by element to a float64 torch reference on the same fp32 inputs: |got - ref64| <= c * 2^-24 * scale64
(gpu_util.bound_ratio), scale64 the element's own operand magnitude, c counted from the kernel's roundings (the derivation stands
next to each constant).  Hyper-parameters that the C ABI takes as `float` are rounded to fp32 before the reference sees them.
Outputs are pre-filled with NaN, the surroundings of strided / padded operands with a sentinel, and both are checked; where a
comment in the kernels or the trainer relies on bitwise equality the check is torch.equal.

Out of scope: a zero residual.  sse == 0 (or a crystal predicted exactly) gives 0 * inf = NaN in the loss kernels exactly as
torch.sqrt(F.mse_loss(...)).backward() does in the reference; the generators keep a noise floor and the tests assert sse64 > 0.

Summation depths: a lane adds 4 values per 256-column step (<= 4 steps up to 1024 columns), a 6-level butterfly adds the 64
lanes of a wave (4 levels for the 16 lanes of a quarter wave)."""
import math

import numpy as np
import pytest
import torch

from tests.gpu_util import (DEV, H_GRAPH, H_ROW4, ROWS, SENT, _in_slice, _norm64, _outside_untouched, _rows, bound_ratio, ops, rnd)
from tests.test_gpu_rowops import C_NORM, _check_norm

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _nan(*shape):
    return torch.full(shape, NAN, device=DEV)


def f32(v):
    """The value the C ABI receives for a `float` parameter, as a Python float (exact in float64)."""
    return float(np.float32(v))


def _rstd(M, seed):
    return (torch.rand(M, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 4 + 0.25).float().to(DEV)


# =====================================================================================================================
# A. LayerNorm family
# =====================================================================================================================

# y = xhat gamma + beta: the error of xhat (C_NORM, against (|x| + mean|x|) rstd) times |gamma|, + the product and the sum
C_LN_Y = C_NORM + 2
# dx = rstd (dh - mean(dh) - xhat mean(dh xhat)), dh = dy gamma.  The two row means: the product dy gamma, the product with xhat,
# <= 12 additions along a lane (4 column blocks x (2 pair levels + the accumulate)), <= 6 butterfly levels, the rounded 1/H and
# the product with it: <= 22; the bracket: dy gamma, two subtractions, xhat s2: 4; the product with rstd: 1
C_LN_DX = 28
# the forms whose dy is itself a rounded product (ddos w; dy scale alpha behind the PReLU): <= 2 more on every term
C_LN_DX2 = C_LN_DX + 2
# column sums of one partial row, H <= 256: a quarter wave adds its 2 rows (product + add each), the 16 quarter waves are added in
# order: 2 x 2 + 16 = 20; wider: a wave adds its 8 rows, then the 4 waves: 8 x 2 + 3 = 19.  The partial rows are summed in float64.
C_LN_COL = 20
# ... with dy a rounded product of up to two factors (rowdot: ddos w; PReLU: dy scale alpha): 8 x (2 + 2) + 3 = 35 at most
C_LN_COL2 = 36
# dw = sum_r ddos (xhat gamma + beta): product, sum, product, add per row: 8 x 4 + 3 = 35 (wide), 2 x 4 + 16 = 24 (H <= 256)
C_LN_DW = 36
# db = sum_r ddos: 2 + 16 additions (H <= 256), 8 + 3 (wide; the wave sum adds zeros)
C_LN_DB = 20
# dos = (xhat gamma + beta) . w + b: the error of xhat (C_NORM) times |gamma w|, + per term product, sum, product: 3, + <= 16
# additions along a lane, 6 butterfly levels and the bias: 26
C_LN_DOT = C_NORM + 26


def c_ln_dalpha(W):
    """dalpha = sum over y < 0 of dy y: a lane adds <= 4 ceil(W / 256) elements per row (each term: xhat gamma, + beta, dy scale,
    dy y: 4 roundings) over the 8 rows of its wave, + 6 butterfly levels + 3 for the 4 waves."""
    return 8 * 4 * ((W + 255) // 256) + 4 + 6 + 3


def _affine(H, seed):
    return 1.0 + 0.5 * rnd(H, seed=seed), rnd(H, seed=seed + 1)


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("H", H_ROW4)
def test_layernorm(H, M):
    o = ops()
    x = _rows(M, H, 101)
    gam, bet = _affine(H, 102)
    y, xhat, rstd = _nan(M, H), _nan(M, H), _nan(M)
    o.layernorm(x, gam, bet, y, xhat, rstd, M, H)
    torch.cuda.synchronize()
    x64 = x.double()
    tag = f"layernorm[H{H},M{M}]"
    _check_norm(xhat, rstd, x64.abs(), x64, tag)
    xh64, _, rs64 = _norm64(x64)
    sx = (x64.abs() + x64.abs().mean(1, keepdim=True)) * rs64
    assert bound_ratio(y, xh64 * gam.double() + bet.double(), sx * gam.double().abs() + bet.double().abs(), C_LN_Y, tag + ".y") <= 1.0
    y2 = _nan(M, H)
    o.layernorm(x, gam, bet, y2, None, None, M, H)           # xhat / rstd are optional
    torch.cuda.synchronize()
    assert torch.equal(y, y2)


def _ln_bwd_ref(dy64, xh64, rs64, g64):
    """dx of the LayerNorm backward and its per-element scale, from the gradient dy64 in front of gamma."""
    dh = dy64 * g64
    dx = rs64 * (dh - dh.mean(1, keepdim=True) - xh64 * (dh * xh64).mean(1, keepdim=True))
    sc = rs64 * (dh.abs() + dh.abs().mean(1, keepdim=True) + xh64.abs() * (dh * xh64).abs().mean(1, keepdim=True))
    return dx, sc


def _partials_ok(part, M, unspecified=()):
    """ceil(M / 32) partial rows, each fully written (columns in `unspecified` excepted)."""
    assert part.shape[0] == (M + 31) // 32
    keep = torch.ones(part.shape[1], dtype=torch.bool, device=DEV)
    for c in unspecified:
        keep[c] = False
    return not bool(torch.isnan(part[:, keep]).any())


LN_BWD_ROWS = [1, 3, 31, 32, 33, 2051]


@pytest.mark.parametrize("M", LN_BWD_ROWS)
@pytest.mark.parametrize("H", H_ROW4)
def test_layernorm_bwd(H, M):
    o = ops()
    dy, xhat, rstd = _rows(M, H, 111, special=False), rnd(M, H, seed=112), _rstd(M, 113)
    gam = rnd(H, seed=114)
    nblk = (M + 31) // 32
    dx = _nan(M, H)
    buf = torch.full((nblk + 2, 2 * H), SENT, device=DEV)    # a sentinel row behind the partial rows
    part = buf[:nblk]
    part.fill_(NAN)
    o.layernorm_bwd(dy, xhat, rstd, gam, dx, part, M, H)
    torch.cuda.synchronize()
    dy64, xh64, rs64, g64 = dy.double(), xhat.double(), rstd.double()[:, None], gam.double()
    ref, sc = _ln_bwd_ref(dy64, xh64, rs64, g64)
    tag = f"layernorm_bwd[H{H},M{M}]"
    assert bound_ratio(dx, ref, sc, C_LN_DX, tag + ".dx") <= 1.0
    assert _partials_ok(part, M) and bool((buf[nblk:] == SENT).all()), tag
    ps = part.double().sum(0)
    assert bound_ratio(ps[:H], (dy64 * xh64).sum(0), (dy64 * xh64).abs().sum(0), C_LN_COL, tag + ".dgamma") <= 1.0
    assert bound_ratio(ps[H:], dy64.sum(0), dy64.abs().sum(0), C_LN_COL, tag + ".dbeta") <= 1.0


SB = [(1, 1), (1, 4), (5, 1), (51, 3), (11, 3), (201, 10)]


@pytest.mark.parametrize("S,Bq", SB)
@pytest.mark.parametrize("H", H_ROW4)
def test_ln_rowdot(H, S, Bq):
    """dos[bq, s] = LayerNorm(x[(s, bq)]) . w + b with xhat / rstd saved."""
    o = ops()
    M = S * Bq
    x = _rows(M, H, 121)
    (gam, bet), w, b = _affine(H, 122), rnd(H, seed=124), rnd(1, seed=125)
    xhat, rstd = _nan(M, H), _nan(M)
    buf = torch.full((Bq * S + 8,), SENT, device=DEV)
    dos = buf[4:4 + Bq * S].view(Bq, S)
    dos.fill_(NAN)
    o.ln_rowdot(x, gam, bet, w, b, xhat, rstd, dos, S, Bq, H)
    torch.cuda.synchronize()
    x64, g64, b64, w64 = x.double(), gam.double(), bet.double(), w.double()
    tag = f"ln_rowdot[H{H},S{S},Bq{Bq}]"
    _check_norm(xhat, rstd, x64.abs(), x64, tag)
    xh64, _, rs64 = _norm64(x64)
    sx = (x64.abs() + x64.abs().mean(1, keepdim=True)) * rs64
    ref = ((xh64 * g64 + b64) @ w64 + b.double()).reshape(S, Bq).t()
    sc = ((sx * g64.abs() + b64.abs()) @ w64.abs() + b.double().abs()).reshape(S, Bq).t()
    assert bound_ratio(dos, ref, sc, C_LN_DOT, tag + ".dos") <= 1.0
    assert bool((buf[:4] == SENT).all()) and bool((buf[4 + Bq * S:] == SENT).all())


@pytest.mark.parametrize("S,Bq", SB + [(31, 1), (32, 1), (33, 1)])
@pytest.mark.parametrize("H", H_ROW4)
def test_ln_rowdot_bwd(H, S, Bq):
    """Row r = s * Bq + bq reads ddos[bq, s]; dx row by row, the partial rows [dgamma | dbeta | dw | db] summed in float64."""
    o = ops()
    M = S * Bq
    xhat, rstd = rnd(M, H, seed=131), _rstd(M, 132)
    (gam, bet), w = _affine(H, 133), rnd(H, seed=135)
    ddos = (rnd(Bq, S, seed=136).double() * torch.logspace(-2, 2, M, dtype=torch.float64, device=DEV).reshape(Bq, S)).float()
    nblk = (M + 31) // 32
    dx = _nan(M, H)
    buf = torch.full((nblk + 2, 3 * H + 1), SENT, device=DEV)
    part = buf[:nblk]
    part.fill_(NAN)
    o.ln_rowdot_bwd(ddos, xhat, rstd, gam, bet, w, dx, part, S, Bq, H)
    torch.cuda.synchronize()
    dr = ddos.double().t().reshape(-1)[:, None]                        # [M, 1]
    xh64, rs64, g64, b64, w64 = xhat.double(), rstd.double()[:, None], gam.double(), bet.double(), w.double()
    dy64 = dr * w64
    ref, sc = _ln_bwd_ref(dy64, xh64, rs64, g64)
    tag = f"ln_rowdot_bwd[H{H},S{S},Bq{Bq}]"
    assert bound_ratio(dx, ref, sc, C_LN_DX2, tag + ".dx") <= 1.0
    assert _partials_ok(part, M) and bool((buf[nblk:] == SENT).all()), tag
    ps = part.double().sum(0)
    assert bound_ratio(ps[:H], (dy64 * xh64).sum(0), (dy64 * xh64).abs().sum(0), C_LN_COL2, tag + ".dgamma") <= 1.0
    assert bound_ratio(ps[H:2 * H], dy64.sum(0), dy64.abs().sum(0), C_LN_COL2, tag + ".dbeta") <= 1.0
    y64 = xh64 * g64 + b64
    assert bound_ratio(ps[2 * H:3 * H], (dr * y64).sum(0), (dr.abs() * ((xh64 * g64).abs() + b64.abs())).sum(0), C_LN_DW,
                       tag + ".dw") <= 1.0
    assert bound_ratio(ps[3 * H:], dr.sum()[None], dr.abs().sum()[None], C_LN_DB, tag + ".db") <= 1.0


def _prelu_case(M, W, seed):
    """xhat, gamma, beta with gamma = beta = 0 at column W // 2 (y = xhat gamma + beta is an exact zero there) and no other y so
    close to zero that fp32 and float64 could disagree about its sign."""
    xhat = rnd(M, W, seed=seed)
    gam, bet = _affine(W, seed + 1)
    c0 = W // 2
    gam[c0] = 0.0
    bet[c0] = 0.0
    for _ in range(4):
        mag = (xhat.double() * gam.double()).abs() + bet.double().abs()
        amb = ((xhat.double() * gam.double() + bet.double()).abs() < 2.0 ** -18 * mag)
        amb[:, c0] = False
        if not bool(amb.any()):
            break
        xhat[amb] += 0.25
    assert not bool(amb.any())
    return xhat, gam, bet, c0


def _ln_prelu_check(dz, part, d64, xh64, rs64, g64, b64, al64, M, W, tag):
    """d64: the (gathered, scaled) gradient behind the PReLU, float64."""
    y64 = xh64 * g64 + b64
    neg = y64 < 0                                           # y == 0 passes the gradient through (the reference's ln >= 0)
    dy64 = torch.where(neg, al64 * d64, d64)
    ref, sc = _ln_bwd_ref(dy64, xh64, rs64, g64)
    assert bound_ratio(dz, ref, sc, C_LN_DX2, tag + ".dz") <= 1.0
    assert _partials_ok(part, M, unspecified=(2 * W, 2 * W + 1, 2 * W + 2)), tag
    ps = part.double().sum(0)
    # (where alpha = 0 the kernel's d * 0 is an exact zero and so is the scale of that term)
    assert bound_ratio(ps[:W], (dy64 * xh64).sum(0), (dy64 * xh64).abs().sum(0), C_LN_COL2, tag + ".dgamma") <= 1.0
    assert bound_ratio(ps[W:2 * W], dy64.sum(0), dy64.abs().sum(0), C_LN_COL2, tag + ".dbeta") <= 1.0
    ymag = (xh64 * g64).abs() + b64.abs()
    assert bound_ratio(ps[2 * W + 3:], torch.where(neg, d64 * y64, torch.zeros_like(d64)).sum()[None],
                       torch.where(neg, d64.abs() * ymag, torch.zeros_like(d64)).sum()[None], c_ln_dalpha(W), tag + ".dalpha") <= 1.0


@pytest.mark.parametrize("alpha", [0.25, 0.0])
@pytest.mark.parametrize("M", [1, 33, 2051])
@pytest.mark.parametrize("W", [4, 12, 128, 256, 260, 512, 516, 1024])
def test_ln_prelu_bwd(W, M, alpha):
    """LayerNorm -> PReLU backward, plain and with gathered gradient rows (row r reads dy[idx[r]] * scale[idx[r]]); rows of up
    to 512 floats take the lean kernel, wider ones ln_bwd_wide_kernel<2>.  An exact zero of y sits in column W // 2: every form
    passes the gradient through there (dbeta / dgamma of that column see dy, not alpha dy)."""
    o = ops()
    xhat, gam, bet, c0 = _prelu_case(M, W, 141)
    rstd = _rstd(M, 144)
    al = torch.tensor([alpha], device=DEV)
    nblk = o.ln_prelu_bwd_partial_rows(M)
    xh64, rs64, g64, b64, al64 = xhat.double(), rstd.double()[:, None], gam.double(), bet.double(), f32(alpha)
    dy = _rows(M, W, 145, special=False)
    dz, part = _nan(M, W), _nan(nblk, 2 * W + 4)
    o.ln_prelu_bwd(dy, xhat, rstd, gam, bet, al, dz, part, M, W)
    torch.cuda.synchronize()
    tag = f"ln_prelu_bwd[W{W},M{M},alpha{alpha}]"
    _ln_prelu_check(dz, part, dy.double(), xh64, rs64, g64, b64, al64, M, W, tag)
    # the zero column: its dbeta is the plain column sum of dy whatever alpha is
    assert bound_ratio(part.double().sum(0)[W + c0][None], dy.double()[:, c0].sum()[None], dy.double()[:, c0].abs().sum()[None],
                       C_LN_COL2, tag + ".dbeta[y==0]") <= 1.0
    # gathered: Nn source rows, the index repeats rows and skips others (row 1 and every 5th are never read)
    Nn = max(3, M // 2)
    gen = torch.Generator().manual_seed(146)
    idx = torch.randint(0, Nn, (M,), generator=gen)
    idx = torch.where((idx % 5 == 4) | (idx == 1), torch.zeros_like(idx), idx).to(torch.int32).to(DEV)
    dyn = _rows(Nn, W, 147, special=False)
    scale = (torch.rand(Nn, generator=gen, dtype=torch.float64) + 0.1).float().to(DEV)
    for sc in (scale, None):
        dz, part = _nan(M, W), _nan(nblk, 2 * W + 4)
        o.ln_prelu_bwd_gather(dyn, idx, sc, xhat, rstd, gam, bet, al, dz, part, M, W)
        torch.cuda.synchronize()
        d64 = dyn.double()[idx.long()] * (sc.double()[idx.long()][:, None] if sc is not None else 1.0)
        gtag = f"ln_prelu_bwd_gather[W{W},M{M},alpha{alpha},scale{int(sc is not None)}]"
        _ln_prelu_check(dz, part, d64, xh64, rs64, g64, b64, al64, M, W, gtag)
        assert bound_ratio(part.double().sum(0)[W + c0][None], d64[:, c0].sum()[None], d64[:, c0].abs().sum()[None], C_LN_COL2,
                           gtag + ".dbeta[y==0]") <= 1.0


# =====================================================================================================================
# B. losses
# =====================================================================================================================

def c_sse(count):
    """sse2_kernel / loss_phonon_fused_kernel: ceil(count / 1024) sequential additions per lane + 6 butterfly levels + 16
    sequential wave sums + 2 (subtract, square).  All terms are non-negative: the scale is the sum itself."""
    return (count + 1023) // 1024 + 6 + 16 + 2


def c_phonon_loss(count):
    """loss = r0 + beta r1, r = sqrt(sse inv_count): half the relative error of sse (the square root), + the rounded
    1 / count_global, the product, sqrtf, beta r1, the sum: 5."""
    return c_sse(count) / 2 + 5


def c_phonon_grad(count):
    """dpg = (pg - y) k, k = [beta] inv_count / r: the error of r (half that of sse, + inv_count, product, sqrtf: 3), + inv_count,
    beta inv_count, the division, the subtraction (one rounding of its own result), the product: 5."""
    return c_sse(count) / 2 + 8


def _phonon_inputs(count, mag, seed):
    """targets |N(0,1)| mag, predictions target + noise, noise amplitudes spread over 1e-3 .. 1 of mag."""
    y = rnd(count, seed=seed).abs() * mag
    amp = torch.logspace(-3, 0, count, dtype=torch.float64, device=DEV) * mag
    pg = (y.double() + rnd(count, seed=seed + 1).double() * amp).float()
    ps = (y.double() + rnd(count, seed=seed + 2).double() * amp).float()
    return pg, ps, y


def _phonon_ref(pg, ps, y, beta, count_global):
    a, b, y64 = pg.double().requires_grad_(True), ps.double().requires_grad_(True), y.double()
    s0, s1 = ((a - y64) ** 2).sum(), ((b - y64) ** 2).sum()
    assert float(s0.detach()) > 0 and float(s1.detach()) > 0                   # (sse64 > 0: a zero residual is out of scope)
    loss = torch.sqrt(s0 / count_global) + beta * torch.sqrt(s1 / count_global)
    loss.backward()
    k0 = 1.0 / (count_global * torch.sqrt(s0.detach() / count_global))
    k1 = beta / (count_global * torch.sqrt(s1.detach() / count_global))
    return loss.detach(), a.grad, b.grad, (a.detach() - y64).abs() * k0, (b.detach() - y64).abs() * k1, s0.detach(), s1.detach()


PHONON_COUNTS = [1, 51, 1023, 1024, 1025, 64 * 51, 512 * 51]


@pytest.mark.parametrize("beta", [0.7, 0.0])
@pytest.mark.parametrize("mag", [1e-3, 1.0, 30.0])
@pytest.mark.parametrize("count", PHONON_COUNTS)
def test_phonon_loss(count, mag, beta):
    """sse2, loss_phonon_bwd (count_global = count and 3 count), the fused loss_phonon (bitwise the two-phase result) and the
    two-shard form of the data-parallel trainer."""
    o = ops()
    b32 = f32(beta)
    pg, ps, y = _phonon_inputs(count, mag, 201)
    tag = f"[count{count},mag{mag:g},beta{beta:g}]"
    sse = _nan(2)
    o.sse2(pg, ps, y, sse, count)
    torch.cuda.synchronize()
    loss64, ga, gb, sa, sb, s0, s1 = _phonon_ref(pg, ps, y, b32, count)
    assert bound_ratio(sse, torch.stack([s0, s1]), torch.stack([s0, s1]), c_sse(count), "sse2" + tag) <= 1.0
    two_phase = None
    for cg in (count, 3 * count):
        loss64, ga, gb, sa, sb, _, _ = _phonon_ref(pg, ps, y, b32, cg)
        dpg, dps, loss = _nan(count), _nan(count), _nan(1)
        o.loss_phonon_bwd(pg, ps, y, sse, beta, cg, dpg, dps, loss, count)
        torch.cuda.synchronize()
        t = f"loss_phonon_bwd[count{count},global{cg},mag{mag:g},beta{beta:g}]"
        assert bound_ratio(loss, loss64[None], loss64[None], c_phonon_loss(count), t + ".loss") <= 1.0
        assert bound_ratio(dpg, ga, sa, c_phonon_grad(count), t + ".dpg") <= 1.0
        assert bound_ratio(dps, gb, sb, c_phonon_grad(count), t + ".dps") <= 1.0
        if cg == count:
            two_phase = (dpg, dps, loss)
    # fused: one launch, same summation order -> bitwise the two-phase result; sse / loss optional
    fsse, fdpg, fdps, floss = _nan(2), _nan(count), _nan(count), _nan(1)
    o.loss_phonon(pg, ps, y, fsse, beta, fdpg, fdps, floss, count)
    torch.cuda.synchronize()
    assert torch.equal(fsse, sse) and torch.equal(floss, two_phase[2]), "loss_phonon" + tag
    assert torch.equal(fdpg, two_phase[0]) and torch.equal(fdps, two_phase[1]), "loss_phonon" + tag
    gdpg, gdps = _nan(count), _nan(count)
    o.loss_phonon(pg, ps, y, None, beta, gdpg, gdps, None, count)
    torch.cuda.synchronize()
    assert torch.equal(gdpg, fdpg) and torch.equal(gdps, fdps), "loss_phonon(sse=None, loss=None)" + tag
    if count < 2:
        return
    # two shards: sse2 per block, the pairs added on the host in float64, the gradient per block with the global count
    n1 = count // 3 + 1
    blocks = [(0, n1), (n1, count)]
    tot = torch.zeros(2, dtype=torch.float64)
    for lo, hi in blocks:
        part = _nan(2)
        o.sse2(pg[lo:hi].contiguous(), ps[lo:hi].contiguous(), y[lo:hi].contiguous(), part, hi - lo)
        torch.cuda.synchronize()
        tot += part.double().cpu()
    sse_g = tot.float().to(DEV)
    loss64, ga, gb, sa, sb, _, _ = _phonon_ref(pg, ps, y, b32, count)
    for lo, hi in blocks:
        n = hi - lo
        dpg, dps, loss = _nan(n), _nan(n), _nan(1)
        o.loss_phonon_bwd(pg[lo:hi].contiguous(), ps[lo:hi].contiguous(), y[lo:hi].contiguous(), sse_g, beta, count, dpg, dps, loss, n)
        torch.cuda.synchronize()
        t = f"loss_phonon_shard[count{count},rows{lo}:{hi},mag{mag:g},beta{beta:g}]"
        # (the block sums carry c_sse of their own length, the float64 sum is rounded to fp32 once)
        assert bound_ratio(loss, loss64[None], loss64[None], c_phonon_loss(count) + 1, t + ".loss") <= 1.0
        assert bound_ratio(dpg, ga[lo:hi], sa[lo:hi], c_phonon_grad(count) + 1, t + ".dpg") <= 1.0
        assert bound_ratio(dps, gb[lo:hi], sb[lo:hi], c_phonon_grad(count) + 1, t + ".dps") <= 1.0


def c_edos_loss(S):
    """one wave per crystal: a = sum (t - p)^2 is off by ceil(S / 64) additions per lane + 6 butterfly levels + 2 (subtract,
    square), halved by the square root; + a / S, sqrtf, beta r1, the sum, the rounded 1 / B_global and the product: 6."""
    return ((S + 63) // 64 + 8) / 2 + 6


def c_edos_grad(S):
    """k = [beta] inv_bglobal / (S r): the error of r (half that of a, + the division by S and sqrtf: 2), + inv_bglobal, beta
    inv_bglobal, S r, the division, the subtraction (one rounding of its own result), the product: 6."""
    return ((S + 63) // 64 + 8) / 2 + 8


def _edos_inputs(B, S, seed):
    """Fourier-filtered targets with a negative share (the loss clamps them to 0); predictions clamp(target) + noise."""
    yft = rnd(B, S, seed=seed) * 0.8
    t = yft.double().clamp(min=0.0)
    amp = torch.logspace(-3, 0, B * S, dtype=torch.float64, device=DEV).reshape(S, B).t()        # every crystal sees the range
    pg = (t + rnd(B, S, seed=seed + 1).double() * amp).float().contiguous()
    ps = (t + rnd(B, S, seed=seed + 2).double() * amp).float().contiguous()
    return pg, ps, yft


@pytest.mark.parametrize("beta", [0.5, 0.0])
@pytest.mark.parametrize("B,S", [(1, 201), (3, 51), (4, 201), (5, 64), (7, 201), (64, 201), (130, 63)])
def test_edos_loss(B, S, beta):
    o = ops()
    b32 = f32(beta)
    pg, ps, yft = _edos_inputs(B, S, 211)
    assert bool((yft < 0).any())
    t64 = torch.where(yft < 0, torch.zeros_like(yft), yft).double()
    one = None
    for Bg in (B, 2 * B + 1):
        a, b = pg.double().requires_grad_(True), ps.double().requires_grad_(True)
        ra, rb = torch.sqrt(((t64 - a) ** 2).mean(1)), torch.sqrt(((t64 - b) ** 2).mean(1))
        assert float(ra.detach().min()) > 0 and float(rb.detach().min()) > 0   # (no crystal predicted exactly)
        (ra.sum() / Bg + b32 * rb.sum() / Bg).backward()
        dpg, dps, lp = _nan(B, S), _nan(B, S), _nan(B)
        o.loss_edos(pg, ps, yft, beta, B, S, Bg, dpg, dps, lp)
        torch.cuda.synchronize()
        tag = f"loss_edos[B{B},S{S},global{Bg},beta{beta:g}]"
        ref_lp = ((ra + b32 * rb) / Bg).detach()
        assert bound_ratio(lp, ref_lp, ref_lp, c_edos_loss(S), tag + ".loss") <= 1.0
        ka, kb = 1.0 / (Bg * S * ra.detach()[:, None]), b32 / (Bg * S * rb.detach()[:, None])
        assert bound_ratio(dpg, a.grad, (a.detach() - t64).abs() * ka, c_edos_grad(S), tag + ".dpg") <= 1.0
        assert bound_ratio(dps, b.grad, (b.detach() - t64).abs() * kb, c_edos_grad(S), tag + ".dps") <= 1.0
        if Bg == B:
            one = (dpg, dps, lp)
    # two shards with B_global = B: one wave per crystal, so bitwise what one call on all B rows writes
    B1 = B // 2
    if B1 == 0:
        return
    dpg, dps, lp = _nan(B, S), _nan(B, S), _nan(B)
    for lo, hi in ((0, B1), (B1, B)):
        o.loss_edos(pg[lo:hi], ps[lo:hi], yft[lo:hi], beta, hi - lo, S, B, dpg[lo:hi], dps[lo:hi], lp[lo:hi])
    torch.cuda.synchronize()
    assert torch.equal(dpg, one[0]) and torch.equal(dps, one[1]) and torch.equal(lp, one[2])


@pytest.mark.parametrize("n", [1, 63, 64, 255, 256, 257, 513, 4097])
def test_sum_to(n):
    o = ops()
    buf = torch.full((n + 8,), SENT, device=DEV)
    src = buf[4:4 + n]
    src.copy_((rnd(n, seed=221).double() * torch.logspace(-3, 3, n, dtype=torch.float64, device=DEV)).float())
    dbuf = torch.full((9,), SENT, device=DEV)
    dbuf[4] = NAN
    o.sum_to(src, n, dbuf[4:5])
    torch.cuda.synchronize()
    # ceil(n / 256) additions along a lane + 6 butterfly levels + 2 for the 4 waves
    assert bound_ratio(dbuf[4:5], src.double().sum()[None], src.double().abs().sum()[None], (n + 255) // 256 + 8, f"sum_to[n{n}]") <= 1.0
    assert bool((dbuf[:4] == SENT).all()) and bool((dbuf[5:] == SENT).all())


# =====================================================================================================================
# C. AdamW
# =====================================================================================================================
# One step in fp32 (division and square root are correctly rounded: no fast-math in the build):
#   gr = g gs                               1 rounding (none when gs = 1)
#   m' = m + (gr - m)(1 - b1)               gr, the difference, the product (both x 0.1), the sum: <= 4 against |m| + |gr|
#                                           (1.f - b1 is exact for 0.9 / 0.999)
#   v' = v b2 + (1 - b2) gr gr              gr twice, two products, the sum (v b2 one product + the sum): <= 6 against v' itself
#   denom = sqrt(v') inv_bc2s + eps         half of v' (3), sqrtf, the rounded inv_bc2s, the product, the sum: 7
#   p' = p decay - step_size (m' / denom)   decay = 1.f - lr wd: half an ulp of 1; p decay: 1; the final difference 1 on both terms.
#                                           update term: m' 4 + denom 7 + division + rounded step_size + product + difference: 15
C_ADAM_M, C_ADAM_V, C_ADAM_P = 4, 6, 16
ADAM_B1, ADAM_B2, ADAM_EPS = 0.9, 0.999, 1e-8
ADAM_CAP = 4096 * 256 * 4                   # floats one sweep of the capped grid covers


def _adam_ref(p, g, m, v, step, lr, wd, gs):
    """float64 update from the fp32 state and the fp32-rounded hyper-parameters; returns (p', m', v') and their scales."""
    lr, wd, gs, b1, b2, eps = f32(lr), f32(wd), f32(gs), f32(ADAM_B1), f32(ADAM_B2), f32(ADAM_EPS)
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    gr = g * gs
    m1 = m + (gr - m) * (1.0 - b1)
    v1 = v * b2 + (1.0 - b2) * gr * gr
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    denom = torch.sqrt(v1) / math.sqrt(bc2) + eps
    p1 = p * (1.0 - lr * wd) - (lr / bc1) * m1 / denom
    # (+ a floor under v': a squared gradient below 2^-100 is in or near fp32's subnormal range, where relative precision ends)
    return (p1, m1, v1), (p.abs() + (lr / bc1) * (m.abs() + gr.abs()) / denom, m.abs() + gr.abs(), v1 + 2.0 ** -100)


def _adam_state(n, step, seed):
    """Flat buffers of n rounded up to 4, + 8 floats, sentinel-filled behind n: |p| over 1e-4 .. 10, |g| over 1e-8 .. 100 with 100
    zero gradients (fewer at small n); zero moments at step 1, moments of the gradients' own magnitude otherwise."""
    gen = torch.Generator().manual_seed(seed)
    npad = (n + 3) // 4 * 4 + 8
    u = lambda: torch.rand(n, generator=gen, dtype=torch.float64)
    r = lambda: torch.randn(n, generator=gen, dtype=torch.float64)
    gmag = 10.0 ** (u() * 10 - 8)
    g = r() * gmag
    g[torch.randperm(n, generator=gen)[:min(100, n // 2)]] = 0.0
    vals = [r() * 10.0 ** (u() * 5 - 4), g]
    if step == 1:
        vals += [torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)]
    else:
        vals += [0.5 * r() * gmag, (r() * gmag) ** 2 * u()]
    out = []
    for t in vals:
        b = torch.full((npad,), SENT, device=DEV)
        b[:n] = t.float().to(DEV)
        out.append(b)
    return out


def _adam_step_check(o, n, p, g, m, v, step, lr, wd, gs, tag):
    p0, g0, m0, v0 = p.clone(), g.clone(), m.clone(), v.clone()
    o.adamw(p, g, m, v, n, lr, ADAM_B1, ADAM_B2, ADAM_EPS, wd, step, gs)
    torch.cuda.synchronize()
    (p1, m1, v1), (sp, sm, sv) = _adam_ref(p0[:n], g0[:n], m0[:n], v0[:n], step, lr, wd, gs)
    assert bound_ratio(m[:n], m1, sm, C_ADAM_M, tag + ".m") <= 1.0
    assert bound_ratio(v[:n], v1, sv, C_ADAM_V, tag + ".v") <= 1.0
    assert bound_ratio(p[:n], p1, sp, C_ADAM_P, tag + ".p") <= 1.0
    for t in (p, m, v):
        assert bool((t[n:] == SENT).all()), tag + ": written behind n"
    assert torch.equal(g, g0), tag + ": gradient changed"


ADAM_SMALL = [(1, 1e-2, 1.0, 1e-3), (2, 0.0, 0.125, 1e-3), (1000, 1e-2, 1.0 / 3.0, 1e-4), (100000, 0.0, 1.0 / 3.0, 1e-3)]
ADAM_LARGE = [(1, 1e-2, 1.0 / 3.0, 1e-3), (1000, 0.0, 0.125, 1e-4)]


@pytest.mark.parametrize("step,wd,gs,lr", ADAM_SMALL)
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1003, 1024])
def test_adamw_step(n, step, wd, gs, lr):
    o = ops()
    p, g, m, v = _adam_state(n, step, 301 + n)
    _adam_step_check(o, n, p, g, m, v, step, lr, wd, gs, f"adamw[n{n},step{step},wd{wd:g},gs{gs:.3g},lr{lr:g}]")


@pytest.mark.parametrize("step,wd,gs,lr", ADAM_LARGE)
@pytest.mark.parametrize("n", [ADAM_CAP - 1, ADAM_CAP + 4 * 256 * 3 + 3, 2 * ADAM_CAP + 5])
def test_adamw_step_beyond_the_grid_cap(n, step, wd, gs, lr):
    """The last size without the grid-stride loop; one partial extra sweep + tail; two full sweeps + tail (the tail is addressed
    by the global thread id)."""
    o = ops()
    p, g, m, v = _adam_state(n, step, 311)
    _adam_step_check(o, n, p, g, m, v, step, lr, wd, gs, f"adamw[n{n},step{step},wd{wd:g},gs{gs:.3g},lr{lr:g}]")


@pytest.mark.parametrize("n", [3, 1003, ADAM_CAP + 7])
@pytest.mark.parametrize("wd,lr", [(1e-2, 1e-3), (0.0, 1e-3)])
def test_adamw_zero_gradient_on_zero_moments(n, wd, lr):
    """m' = v' = 0, the update term is 0 / eps = 0: p' is exactly the fp32 product p * decay, decay = 1.f - lr * wd in fp32."""
    o = ops()
    p, g, m, v = _adam_state(n, 1, 321)
    g[:n] = 0.0
    p0 = p.clone()
    o.adamw(p, g, m, v, n, lr, ADAM_B1, ADAM_B2, ADAM_EPS, wd, 1, 1.0 / 3.0)
    torch.cuda.synchronize()
    decay = np.float32(1.0) - np.float32(lr) * np.float32(wd)
    assert torch.equal(p[:n], p0[:n] * torch.tensor(decay, device=DEV))
    assert bool((m[:n] == 0).all()) and bool((v[:n] == 0).all())
    assert bool((p[n:] == SENT).all()) and bool((m[n:] == SENT).all()) and bool((v[n:] == SENT).all())


def test_adamw_trajectory():
    """20 steps at n = 1003; each step's float64 reference starts from the kernel's own fp32 state of the step before, so the
    bound does not compound."""
    o = ops()
    n = 1003
    p, _, m, v = _adam_state(n, 1, 331)
    for step in range(1, 21):
        g = _adam_state(n, 1, 340 + step)[1]
        _adam_step_check(o, n, p, g, m, v, step, 1e-3, 1e-2, 0.125, f"adamw_trajectory[step{step}]")


# =====================================================================================================================
# D. the small utilities of the same step (graph_ops.hip)
# =====================================================================================================================

@pytest.mark.parametrize("rows", [1, 7, 8, 9, 64, 70])
@pytest.mark.parametrize("width", [1, 3, 51, 64, 201, 256])
def test_embed_rows_and_backward(width, rows):
    """out = table[idx] (exact copy); dtable[t] = sum of the dout rows with idx == t, in row order (8-wide unroll + remainder).
    Table row 5 is never indexed: an exact zero."""
    o = ops()
    T = 7
    tab = _rows(T, width, 401, special=False)
    gen = torch.Generator().manual_seed(402 + rows)
    idx = torch.randint(0, T - 1, (rows,), generator=gen)
    idx = torch.where(idx == 5, torch.full_like(idx, 6), idx).to(torch.int32).to(DEV)
    out = _nan(rows, width)
    o.embed_rows(tab, idx, out, rows, width)
    torch.cuda.synchronize()
    assert torch.equal(out, tab[idx.long()])
    for pad in (0, 5):
        ld = width + pad
        dbuf = torch.full((rows, ld), SENT, device=DEV)
        dout = _rows(rows, width, 403, special=False)
        dbuf[:, :width] = dout
        dtab = _nan(T, width)
        o.embed_rows_bwd(dbuf.data_ptr(), ld, idx, dtab, rows, T, width)
        torch.cuda.synchronize()
        z = torch.zeros(T, width, dtype=torch.float64, device=DEV)
        ref = z.clone().index_add_(0, idx.long(), dout.double())
        sc = z.clone().index_add_(0, idx.long(), dout.double().abs())
        # a chain of one addition per matching row, the first one onto 0 exact (a row indexed once is an exact copy)
        depth = int(torch.bincount(idx.long(), minlength=T).max()) - 1
        assert bound_ratio(dtab, ref, sc, depth, f"embed_rows_bwd[width{width},rows{rows},ld{ld}]") <= 1.0
        assert bool((dtab[5] == 0).all())


@pytest.mark.parametrize("n_out,width", [(5, 32), (31, 32), (32, 32), (33, 32), (3, 516)])
@pytest.mark.parametrize("n_red", [1, 7, 8, 9, 128])
def test_reduce_rows(n_red, n_out, width):
    """dst[i] (+)= sum_j src[i stride_out + j stride_red] with the two stride patterns of the heads' backward, strided source and
    destination rows, n_out * width / 4 lanes on either side of one workgroup."""
    o = ops()
    R = n_out * n_red
    sbuf, src = _in_slice(R, width)
    src.copy_(_rows(R, width, 411, special=False))
    s64 = src.double()
    for pattern in ("out-major", "red-major"):
        if pattern == "out-major":                           # (stride_out, stride_red) = (n_red, 1): rows i * n_red + j
            so, sr, v = n_red, 1, s64.reshape(n_out, n_red, width)
            ref, sc = v.sum(1), v.abs().sum(1)
        else:                                                # (1, n_out): rows i + j * n_out
            so, sr, v = 1, n_out, s64.reshape(n_red, n_out, width)
            ref, sc = v.sum(0), v.abs().sum(0)
        for acc in (0, 1):
            dbuf, dst = _in_slice(n_out, width, pad=12)
            d0 = _rows(n_out, width, 412, special=False) if acc else _nan(n_out, width)
            dst.copy_(d0)
            o.reduce_rows(src.data_ptr(), sbuf.stride(0), dst.data_ptr(), dbuf.stride(0), n_out, n_red, so, sr, width, accumulate=bool(acc))
            torch.cuda.synchronize()
            # n_red sequential additions, the first onto 0 exact, + the accumulate (n_red = 1 without it: an exact copy)
            assert bound_ratio(dst, ref + (d0.double() if acc else 0.0), sc + (d0.double().abs() if acc else 0.0), n_red - 1 + acc,
                               f"reduce_rows[{pattern},n_red{n_red},n_out{n_out},width{width},acc{acc}]") <= 1.0
            assert _outside_untouched(dbuf, width) and _outside_untouched(sbuf, width)


ACT_CAP = 8192 * 256 * 4                    # floats one sweep of grid_1d's capped grid covers


@pytest.mark.parametrize("n", [4, 1020, 1024, 1028, ACT_CAP + 1028])
@pytest.mark.parametrize("slope", [0.01, 0.0, 1.0])
def test_act_bwd(slope, n):
    """out = y > 0 ? dy : slope dy, one multiplication: bitwise the fp32 expression.  y holds exact 0.0, -0.0, denormals of both
    signs (a denormal > 0 is positive) at both ends of the buffer."""
    o = ops()
    y, dy = rnd(n, seed=421), rnd(n, seed=422)
    special = torch.tensor([0.0, -0.0, 1e-40, -1e-40], device=DEV)
    for at in (0, n - 4):
        y[at:at + 4] = special
    buf = torch.full((n + 8,), SENT, device=DEV)
    out = buf[4:4 + n]
    out.fill_(NAN)
    o.act_bwd(dy, y, slope, out)
    torch.cuda.synchronize()
    s32 = torch.tensor(slope, dtype=torch.float32)
    ref = torch.where(y.cpu() > 0, dy.cpu(), s32 * dy.cpu())
    assert torch.equal(out.cpu().view(torch.int32), ref.view(torch.int32))
    for at in (0, n - 4):
        assert torch.equal(out[at:at + 4].cpu(), torch.stack([s32 * dy[at].cpu(), s32 * dy[at + 1].cpu(), dy[at + 2].cpu(), s32 * dy[at + 3].cpu()]))
    assert bool((buf[:4] == SENT).all()) and bool((buf[4 + n:] == SENT).all())


def _sizes(sizes):
    if sizes == "many":
        return torch.randint(1, 13, (300,), generator=torch.Generator().manual_seed(31)).tolist()
    return sizes


POOL_SIZES = [[1], [6], [1, 7, 3, 7, 2], "many", [3, 400, 2]]


@pytest.mark.parametrize("sizes", POOL_SIZES, ids=lambda s: s if isinstance(s, str) else "-".join(map(str, s)))
@pytest.mark.parametrize("H", H_GRAPH)
def test_graph_pool_and_backward(H, sizes):
    """pooled[b] = sum of crystal b's node rows (64 / min(64, H / 4) rows per wave step, summed over the row slots by a butterfly);
    backward: dx[n] (+)= dpool[node_graph[n]], exact zero rows for ghost nodes (node_graph >= num_graphs)."""
    o = ops()
    sizes = _sizes(sizes)
    B, N = len(sizes), sum(sizes)
    x = _rows(N, H, 431, special=False)
    ptr = torch.tensor([0] + list(np.cumsum(sizes)), dtype=torch.int32, device=DEV)
    node_graph = torch.repeat_interleave(torch.arange(B), torch.tensor(sizes)).to(DEV)
    obuf, pooled = _in_slice(B, H)
    pooled.fill_(NAN)
    o.graph_pool(x, ptr, pooled.data_ptr(), obuf.stride(0), B, H)
    torch.cuda.synchronize()
    z = torch.zeros(B, H, dtype=torch.float64, device=DEV)
    rps = 64 // min(64, H // 4)
    # a slot adds ceil(n / rps) rows in order, log2(rps) butterfly levels add the slots
    depth = (max(sizes) + rps - 1) // rps + int(math.log2(rps))
    tag = f"[H{H},B{B},N{N}]"
    assert bound_ratio(pooled, z.clone().index_add_(0, node_graph, x.double()), z.clone().index_add_(0, node_graph, x.double().abs()),
                       depth, "graph_pool" + tag) <= 1.0
    assert _outside_untouched(obuf, H)
    # backward; the last 3 nodes are ghosts of a padded batch
    Ng = N + 3
    ng = torch.cat([node_graph, torch.tensor([B, B + 1, B], device=DEV)]).to(torch.int32)
    dbuf, dp = _in_slice(B, H)
    dp.copy_(_rows(B, H, 432, special=False))
    ref = torch.cat([dp.double()[node_graph], torch.zeros(3, H, dtype=torch.float64, device=DEV)])
    for acc in (0, 1):
        dx0 = _rows(Ng, H, 433, special=False) if acc else _nan(Ng, H)
        dx = dx0.clone()
        o.graph_pool_bwd(dp.data_ptr(), dbuf.stride(0), ng, dx, Ng, H, bool(acc), num_graphs=B)
        torch.cuda.synchronize()
        if acc:                                              # one addition
            assert bound_ratio(dx, ref + dx0.double(), ref.abs() + dx0.double().abs(), 1, f"graph_pool_bwd{tag[:-1]},acc1]") <= 1.0
            assert torch.equal(dx[N:], dx0[N:])
        else:                                                # a copy
            assert torch.equal(dx, ref.float())
        assert _outside_untouched(dbuf, H)


@pytest.mark.parametrize("mean", [0, 1])
@pytest.mark.parametrize("N", [1, 37, 2051])
@pytest.mark.parametrize("H", H_GRAPH)
def test_seg_count_scale(H, N, mean):
    """out[n] = c_n src[n]: c_n the segment length (mean 0) or [segment not empty] (mean 1); nodes of degree 0, src rows strided."""
    o = ops()
    deg = torch.randint(0, 9, (N,), generator=torch.Generator().manual_seed(441))
    deg[::3] = 0
    rowptr = torch.cat([torch.zeros(1, dtype=torch.int64), deg.cumsum(0)]).to(torch.int32).to(DEV)
    sbuf, src = _in_slice(N, H)
    src.copy_(_rows(N, H, 442, special=False))
    out = _nan(N, H)
    o.seg_count_scale(src, sbuf.stride(0), rowptr, mean, out, N, H)
    torch.cuda.synchronize()
    cn = ((deg > 0).double() if mean else deg.double()).to(DEV)[:, None]
    # one product (exact where c_n is 0 or 1)
    assert bound_ratio(out, src.double() * cn, src.double().abs() * cn, 1, f"seg_count_scale[H{H},N{N},mean{mean}]") <= 1.0
    assert bool((out[deg.to(DEV) == 0] == 0).all()) and _outside_untouched(sbuf, H)
