"""The row kernels (csrc/graph_ops.hip, csrc/rowops.hip), the K != V attention building blocks (csrc/attention_kv.hip),
ops.attention_weights, the batched copy and the fill, each called directly and held element by element to a float64 torch
reference on the same fp32 inputs: |got - ref64| <= c * 2^-24 * scale64 (gpu_util.bound_ratio), scale64 the element's own
operand magnitude.  The shapes sit where one-wave-per-row kernels go wrong: H around the 256-column step of their loops,
row counts that are not a multiple of the 4 rows of a workgroup, strided operands inside sentinel-filled buffers, the
accumulate flags, masks and optional outputs present and absent.

Summation depth behind most constants: a lane adds 4 values per 256-column step (<= 4 steps up to H = 1024) and a 6-level
butterfly adds the 64 lanes, so a row sum is rounded <= 13 times along any path (<= 21 for a dot product: mul + add per term)."""
import itertools

import pytest
import torch

from tests.gpu_util import (DEV, H_GRAPH, H_ROW4, LN_EPS, ROWS, SENT, _in_slice, _norm64, _outside_untouched, _rows, bound_ratio, ops,
                            rnd)

pytestmark = pytest.mark.gpu


# row normalisations: the mean is off by <= 13 eps mean|x| (summation depth) + 1 (division); the two-pass variance by <= 13 + 3
# (subtraction, square, division) + 1 (+ eps), halved by the square root, + 1 ulp of rsqrtf, + (mean error / spread)^2 <= 10 eps
# on the offset row; xhat = (x - mean) rstd adds 2 roundings.  24 covers each: xhat against (|x| + mean|x|) rstd, rstd against itself
C_NORM = 24


def _check_norm(xhat, rstd, mag64, x64, what, in_err64=None):
    """xhat / rstd of the rows x64 against the float64 normalisation; mag64: each element's |operands| (|x|, or |z|+|p|+|q|);
    in_err64: a bound on the kernel's own rounding of each input element, in units of eps (None: the input is exact).  An input
    error dx moves the variance by 2 mean(d dx) (d = x - mean), so rstd by rstd^3 mean(|d| dx): on a row sitting on a large
    offset that term dominates."""
    xh64, mean64, rs64 = _norm64(x64)
    scale = (mag64 + mag64.mean(1, keepdim=True)) * rs64
    rs_scale = rs64
    if in_err64 is not None:
        rs_scale = rs64 * (1.0 + rs64 ** 2 * ((x64 - mean64).abs() * in_err64).mean(1, keepdim=True))
    assert bound_ratio(xhat, xh64, scale, C_NORM, what + ".xhat") <= 1.0
    assert bound_ratio(rstd.reshape(-1, 1), rs64, rs_scale, C_NORM, what + ".rstd") <= 1.0


def _stats_ok(st, out, what):
    """LayerNorm statistics (mean, rstd) of the out rows as stored (the kernel re-reads what it wrote)."""
    y = out.double()
    mean64 = y.mean(1)
    rstd64 = 1.0 / torch.sqrt(((y - mean64[:, None]) ** 2).mean(1) + LN_EPS)
    # mean: 13 summation levels + the division, against mean|out|; rstd: as the row normalisations
    return (bound_ratio(st[:, 0], mean64, y.abs().mean(1), 16, what + ".mean") <= 1.0
            and bound_ratio(st[:, 1], rstd64, rstd64, C_NORM, what + ".rstd") <= 1.0)


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("H", H_GRAPH)
def test_mask_residual(H, M):
    """out = (res or 0) + a o (mask or 1) [+ LayerNorm statistics of out]: every combination of mask / res / stats, contiguous and
    strided (lda / ldr / ldo != H inside sentinel buffers) operands."""
    o = ops()
    a0, r0 = _rows(M, H, 1), _rows(M, H, 3, special=False)
    m0 = (torch.rand(M, H, generator=torch.Generator().manual_seed(2)) > 0.3).float().to(DEV) / 0.7
    for masked, res, stats, strided in itertools.product((False, True), repeat=4):
        if strided:
            (abuf, a), (rbuf, r), (obuf, out) = _in_slice(M, H), _in_slice(M, H), _in_slice(M, H)
            a.copy_(a0)
            r.copy_(r0)
        else:
            a, r, out = a0.clone(), r0.clone(), torch.full((M, H), float("nan"), device=DEV)
        st = torch.full((M, 2), float("nan"), device=DEV) if stats else None
        o.mask_residual(a, m0 if masked else None, r if res else None, out, st, M, H)
        torch.cuda.synchronize()
        am = a0.double() * (m0.double() if masked else 1.0)
        tag = f"mask_residual[H{H},M{M},mask{int(masked)},res{int(res)},stats{int(stats)},strided{int(strided)}]"
        # one rounding of the product a * mask, one of the sum (or the one of a fused multiply-add)
        assert bound_ratio(out, am + (r0.double() if res else 0.0), am.abs() + (r0.double().abs() if res else 0.0), 2, tag) <= 1.0
        if strided:
            assert _outside_untouched(obuf, H) and _outside_untouched(abuf, H) and _outside_untouched(rbuf, H), tag
        if stats:
            assert _stats_ok(st, out, tag), tag


@pytest.mark.parametrize("M", [1, 5, 2051])
@pytest.mark.parametrize("W", [256, 512, 1024])
def test_mask_residual_in_place(W, M):
    """a is out (both declared without __restrict__): the dropped feed-forward activation h <- h o mask exactly as
    functional.py calls it (res and stats absent), and in place on a strided slice with the residual and the statistics."""
    o = ops()
    h0 = _rows(M, W, 5)
    m = (torch.rand(M, W, generator=torch.Generator().manual_seed(6)) > 0.25).float().to(DEV) / 0.75
    am = h0.double() * m.double()
    h = h0.clone()
    o.mask_residual(h, m, None, h, None, M, W)
    torch.cuda.synchronize()
    assert bound_ratio(h, am, am.abs(), 1, f"mask_residual_in_place[W{W},M{M}]") <= 1.0          # one rounded product
    buf, s = _in_slice(M, W)
    s.copy_(h0)
    r = _rows(M, W, 7, special=False)
    st = torch.full((M, 2), float("nan"), device=DEV)
    o.mask_residual(s, m, r, s, st, M, W)
    torch.cuda.synchronize()
    tag = f"mask_residual_in_place_strided[W{W},M{M}]"
    assert bound_ratio(s, am + r.double(), am.abs() + r.double().abs(), 2, tag) <= 1.0           # product + sum
    assert _outside_untouched(buf, W)
    assert _stats_ok(st, s, tag)


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("H", H_GRAPH)
def test_rownorm(H, M):
    o = ops()
    x = _rows(M, H, 11)
    xhat, rstd = torch.full((M, H), float("nan"), device=DEV), torch.full((M,), float("nan"), device=DEV)
    o.rownorm(x, xhat, rstd, M, H)
    torch.cuda.synchronize()
    _check_norm(xhat, rstd, x.double().abs(), x.double(), f"rownorm[H{H},M{M}]")


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("H", H_GRAPH)
def test_rownorm_bwd(H, M):
    """dx (+)= rstd (g - mean(g) - xhat mean(g xhat)): accumulate 0 on a NaN-filled dx, 1 on a filled one."""
    o = ops()
    g, xhat = _rows(M, H, 21, special=False), rnd(M, H, seed=22)
    rstd = (torch.rand(M, generator=torch.Generator().manual_seed(23), dtype=torch.float64) * 4 + 0.25).float().to(DEV)
    g64, xh64, rs64 = g.double(), xhat.double(), rstd.double()[:, None]
    ref = rs64 * (g64 - g64.mean(1, keepdim=True) - xh64 * (g64 * xh64).mean(1, keepdim=True))
    scale = rs64 * (g64.abs() + g64.abs().mean(1, keepdim=True) + xh64.abs() * (g64 * xh64).abs().mean(1, keepdim=True))
    for acc in (0, 1):
        dx0 = _rows(M, H, 24, special=False) if acc else torch.full((M, H), float("nan"), device=DEV)
        dx = dx0.clone()
        o.rownorm_bwd(g, xhat, rstd, dx, M, H, acc)
        torch.cuda.synchronize()
        # the two row means: <= 21 roundings (dot-product depth); 3 in the bracket, 1 for rstd, 1 for the accumulate add
        assert bound_ratio(dx, ref + (dx0.double() if acc else 0.0), scale + (dx0.double().abs() if acc else 0.0), 28,
                           f"rownorm_bwd[H{H},M{M},acc{acc}]") <= 1.0


@pytest.mark.parametrize("sizes", [[1], [6], [1, 7, 3, 7, 2], "many"])
@pytest.mark.parametrize("H", H_GRAPH)
def test_dense_normalize_slots(H, sizes):
    """kvhat[(pos, b)] = rownorm(x[graph_ptr[b] + pos]) for a real node, zeros for a padded slot and for the spare row n_max*B;
    rstd_nodes written for every node; bitwise the result of dense_normalize on the same batch.  Crystals of one node, of
    exactly n_max nodes, and 300 crystals of 1..12 nodes."""
    o = ops()
    if sizes == "many":
        sizes = torch.randint(1, 13, (300,), generator=torch.Generator().manual_seed(31)).tolist()
    B, n_max, N = len(sizes), max(sizes), sum(sizes)
    x = _rows(N, H, 32)
    ptr = torch.tensor([0] + list(itertools.accumulate(sizes)), dtype=torch.int32, device=DEV)
    rows = n_max * B + 1
    kv, rs = torch.full((rows, H), float("nan"), device=DEV), torch.full((N,), float("nan"), device=DEV)
    o.dense_normalize_slots(x, ptr, kv, rs, B, n_max, H)
    torch.cuda.synchronize()
    pos = torch.cat([torch.arange(s) for s in sizes])
    crystal = torch.repeat_interleave(torch.arange(B), torch.tensor(sizes))
    dense_row = (pos * B + crystal).to(torch.int32).to(DEV)
    xh64, _, rs64 = _norm64(x.double())
    ref = torch.zeros(rows, H, dtype=torch.float64, device=DEV)
    scale = torch.zeros(rows, H, dtype=torch.float64, device=DEV)          # padded slots and the spare row: exactly zero
    ref[dense_row.long()] = xh64
    scale[dense_row.long()] = (x.double().abs() + x.double().abs().mean(1, keepdim=True)) * rs64
    tag = f"dense_normalize_slots[H{H},B{B},n_max{n_max}]"
    assert bound_ratio(kv, ref, scale, C_NORM, tag + ".kvhat") <= 1.0
    assert bound_ratio(rs[:, None], rs64, rs64, C_NORM, tag + ".rstd") <= 1.0
    assert bool((kv[-1] == 0).all())
    kv2, rs2 = torch.full((rows, H), float("nan"), device=DEV), torch.full((N,), float("nan"), device=DEV)
    o.dense_normalize(x, dense_row, kv2, rs2, N, H, rows)
    torch.cuda.synchronize()
    assert torch.equal(kv, kv2) and torch.equal(rs, rs2)


@pytest.mark.parametrize("E", ROWS)
@pytest.mark.parametrize("W", H_ROW4)
def test_gather_add_rownorm(W, E):
    """xhat = rownorm(z + p[src] + q[dst]) with p / q strided column slices of wider node tables; the row lives in registers
    (W / 256 float4 per lane, W <= 1024)."""
    o = ops()
    Nn = 37
    (pbuf, p), (qbuf, q) = _in_slice(Nn, W), _in_slice(Nn, W, pad=12)
    p.copy_(_rows(Nn, W, 41, special=False))
    q.copy_(_rows(Nn, W, 42, special=False))
    z = _rows(E, W, 43)
    gen = torch.Generator().manual_seed(44)
    src = torch.randint(0, Nn, (E,), generator=gen, dtype=torch.int32).to(DEV)
    dst = torch.randint(0, Nn, (E,), generator=gen, dtype=torch.int32).to(DEV)
    xhat, rstd = torch.full((E, W), float("nan"), device=DEV), torch.full((E,), float("nan"), device=DEV)
    o.gather_add_rownorm(z, p, q, src, dst, xhat, rstd, E, W)
    torch.cuda.synchronize()
    ps, qd = p.double()[src.long()], q.double()[dst.long()]
    mag = z.double().abs() + ps.abs() + qd.abs()
    # the three-term input sum is rounded twice in fp32: <= 2 eps (|z| + |p| + |q|) per element
    _check_norm(xhat, rstd, mag, z.double() + ps + qd, f"gather_add_rownorm[W{W},E{E}]", in_err64=2 * mag)
    assert _outside_untouched(pbuf, W) and _outside_untouched(qbuf, W)


@pytest.mark.parametrize("S,Bq", [(1, 1), (3, 1), (1, 4), (5, 1), (51, 3), (201, 10)])
@pytest.mark.parametrize("H", H_ROW4)
def test_rowdot_and_backward(H, S, Bq):
    """dos[bq, s] = x[(s, bq)] . w + b; backward: dx = ddos w and per-workgroup partial rows [dw | db] (32 rows each) whose sum
    is the weight / bias gradient."""
    o = ops()
    M = S * Bq
    x, w, b = _rows(M, H, 51, special=False), rnd(H, seed=52), rnd(1, seed=53)
    dos = torch.full((Bq, S), float("nan"), device=DEV)
    o.rowdot(x, w, b, dos, S, Bq, H)
    torch.cuda.synchronize()
    x64, w64 = x.double(), w.double()
    y64 = (x64 @ w64 + b.double()).reshape(S, Bq).t()
    sc = (x64.abs() @ w64.abs() + b.double().abs()).reshape(S, Bq).t()
    # <= 16 multiply-adds along a lane (4 per 256-column step) + 6 butterfly levels + the bias
    assert bound_ratio(dos, y64, sc, 24, f"rowdot[H{H},S{S},Bq{Bq}]") <= 1.0
    ddos = (rnd(Bq, S, seed=54).double() * torch.logspace(-2, 2, M, dtype=torch.float64, device=DEV).reshape(Bq, S)).float()
    nblk = (M + 31) // 32
    dx = torch.full((M, H), float("nan"), device=DEV)
    part = torch.full((nblk, H + 1), float("nan"), device=DEV)
    o.rowdot_bwd(ddos, x, w, dx, part, S, Bq, H)
    torch.cuda.synchronize()
    dy = ddos.double().t().reshape(-1)                     # row r = s * Bq + bq reads ddos[bq, s]
    tag = f"rowdot_bwd[H{H},S{S},Bq{Bq}]"
    assert bound_ratio(dx, dy[:, None] * w64, (dy[:, None] * w64).abs(), 1, tag + ".dx") <= 1.0       # one rounded product
    ps = part.double().sum(0)                              # (the partial rows summed in float64)
    # a wave adds its 8 rows (product + add each), the 4 waves of a workgroup are added: <= 19 roundings
    assert bound_ratio(ps[:H], dy @ x64, dy.abs() @ x64.abs(), 20, tag + ".dw") <= 1.0
    assert bound_ratio(ps[H:], dy.sum()[None], dy.abs().sum()[None], 12, tag + ".db") <= 1.0          # 8 + 3 additions


def _scores(rows, Nk, scale, seed):
    """Score rows of their own magnitudes; row 0 all equal, row 1 with scale * S near +-80, row 2 all near +80."""
    S = rnd(rows, Nk, seed=seed).double() * torch.logspace(-1, 1.5, rows, dtype=torch.float64, device=DEV)[:, None]
    g = torch.Generator().manual_seed(seed + 1)
    if rows >= 3:
        S[0] = 3.7
        S[1] = ((80.0 * torch.sign(torch.randn(Nk, generator=g, dtype=torch.float64)) + torch.rand(Nk, generator=g, dtype=torch.float64))
                / scale).to(DEV)
        S[2] = ((80.0 - 0.5 * torch.rand(Nk, generator=g, dtype=torch.float64)) / scale).to(DEV)
    return S.float()


def _softmax_scale(P64, a64):
    """scale64 of a softmax P = softmax(a): P (K + 8), K = 1 + 2 max|a| over the row, + a floor below which fp32 underflows."""
    return P64 * (1.0 + 2.0 * a64.abs().amax(-1, keepdim=True) + 8.0) + 2.0 ** -100


# e_j = exp(a_j - max) is off by <= eps (2K + 2) relative (the rounded argument: eps (|a_j| + |max| + |a_j - max|); expf <= 2 ulp);
# P = e / sum e by twice that (the sum carries every e_j's error) + <= 22 roundings of the sum (16 per lane at 1000 keys + 6
# levels) + the reciprocal and the product: <= eps (4K + 28) <= 4 eps (K + 8)
C_SOFTMAX = 4


@pytest.mark.parametrize("rows", [1, 3, 5, 2051])
@pytest.mark.parametrize("Nk", [1, 5, 63, 64, 65, 321, 1000])
def test_softmax_fwd_bwd(Nk, rows):
    """P = softmax(scale S) row by row; dS = scale P o (dP - sum(dP o P)), dP = dPd o mask, with and without the mask."""
    o = ops()
    for scale in (1.0, 384 ** -0.5):
        sc32 = float(torch.tensor(scale, dtype=torch.float32))                # the kernel takes the scale as an fp32 value
        S = _scores(rows, Nk, sc32, seed=61)
        P = torch.full((rows, Nk), float("nan"), device=DEV)
        o.softmax_fwd(S, P, rows, Nk, scale)
        torch.cuda.synchronize()
        a64 = sc32 * S.double()
        P64 = torch.softmax(a64, -1)
        assert bound_ratio(P, P64, _softmax_scale(P64, a64), C_SOFTMAX, f"softmax_fwd[Nk{Nk},rows{rows},scale{scale:.3g}]") <= 1.0
        if rows >= 3:
            assert bool((P[0] == P[0, 0]).all())                              # the all-equal row: uniform, bitwise
        dPd = _rows(rows, Nk, 62, special=False)
        for masked in (False, True):
            m = (torch.rand(rows, Nk, generator=torch.Generator().manual_seed(63)) > 0.3).float().to(DEV) / 0.7 if masked else None
            dS = torch.full((rows, Nk), float("nan"), device=DEV)
            o.softmax_bwd(P, m, dPd, dS, rows, Nk, scale)
            torch.cuda.synchronize()
            p64 = P.double()
            dP = dPd.double() * (m.double() if masked else 1.0)
            ref = sc32 * p64 * (dP - (dP * p64).sum(-1, keepdim=True))
            # (+ a floor: a weight P below 2^-100 gives a result in or near fp32's subnormal range, where relative precision ends)
            sc = abs(sc32) * p64 * (dP.abs() + (dP * p64).abs().sum(-1, keepdim=True)) + 2.0 ** -100
            # the row sum: <= 16 products + adds per lane + 6 levels; the dP product, the subtraction, two products
            assert bound_ratio(dS, ref, sc, 40, f"softmax_bwd[Nk{Nk},rows{rows},scale{scale:.3g},mask{int(masked)}]") <= 1.0


KV_SHAPES = [(51, 4, 41, 4, 384), (51, 6, 9, 2, 512), (7, 3, 70, 1, 260), (1, 1, 1, 1, 4), (33, 2, 17, 2, 1024),
             (5, 3, 12, 3, 100), (201, 2, 41, 2, 256), (4, 6, 3, 2, 12)]


@pytest.mark.parametrize("Sq,Bq,Nk,Bk,H", KV_SHAPES)
def test_attn_dp_pv_tv(Sq, Bq, Nk, Bk, H):
    """dP = X . V^T, out = (A o mask) . V, out (+)= (A o mask)^T . X with query batch entry bq reading crystal bq % Bk (Bq = Bk and
    Bq = 3 Bk): rows (s, bq) at s * Bq + bq, keys (j, bk) at j * Bk + bk, weights [Bq, Sq, Nk]."""
    o = ops()
    X, V = _rows(Sq * Bq, H, 71, special=False), _rows(Nk * Bk, H, 72, special=False)
    A = torch.rand(Bq, Sq, Nk, generator=torch.Generator().manual_seed(73)).to(DEV)
    mask = (torch.rand(Bq, Sq, Nk, generator=torch.Generator().manual_seed(74)) > 0.3).float().to(DEV) / 0.7
    X64 = X.double().reshape(Sq, Bq, H).transpose(0, 1)                                               # [Bq, Sq, H]
    V64 = V.double().reshape(Nk, Bk, H)[:, torch.arange(Bq, device=DEV) % Bk].transpose(0, 1)          # [Bq, Nk, H]
    shape = f"Sq{Sq},Bq{Bq},Nk{Nk},Bk{Bk},H{H}"
    dP = torch.full((Bq, Sq, Nk), float("nan"), device=DEV)
    o.attn_dp(X, V, dP, Sq, Bq, Nk, Bk, H)
    torch.cuda.synchronize()
    # <= 16 multiply-adds along a lane + 6 butterfly levels
    assert bound_ratio(dP, X64 @ V64.transpose(1, 2), X64.abs() @ V64.abs().transpose(1, 2), 24, f"attn_dp[{shape}]") <= 1.0
    n_terms = (Bq // Bk) * Sq
    Xr = X.double().reshape(Sq, Bq // Bk, Bk, H)                          # [s, i, bk, h]: query rows of crystal bk, bq = bk + i Bk
    for masked in (False, True):
        Am = A.double() * (mask.double() if masked else 1.0)
        out = torch.full((Sq * Bq, H), float("nan"), device=DEV)
        o.attn_pv(A, mask if masked else None, V, out, Sq, Bq, Nk, Bk, H)
        torch.cuda.synchronize()
        # a chain of Nk fused multiply-adds in key order + the mask product
        assert bound_ratio(out, (Am @ V64).transpose(0, 1).reshape(Sq * Bq, H),
                           (Am.abs() @ V64.abs()).transpose(0, 1).reshape(Sq * Bq, H), Nk + 1, f"attn_pv[{shape},mask{int(masked)}]") <= 1.0
        Ar = Am.reshape(Bq // Bk, Bk, Sq, Nk)                             # [i, bk, s, j]
        tv = torch.einsum("ibsj,sibh->jbh", Ar, Xr).reshape(Nk * Bk, H)
        tvs = torch.einsum("ibsj,sibh->jbh", Ar.abs(), Xr.abs()).reshape(Nk * Bk, H)
        for acc in (0, 1):
            o0 = _rows(Nk * Bk, H, 75, special=False) if acc else torch.full((Nk * Bk, H), float("nan"), device=DEV)
            out = o0.clone()
            o.attn_tv(A, mask if masked else None, X, out, Sq, Bq, Nk, Bk, H, accumulate=bool(acc))
            torch.cuda.synchronize()
            # a chain of (Bq / Bk) Sq fused multiply-adds onto the (pre-filled) row + the mask product
            assert bound_ratio(out, tv + (o0.double() if acc else 0.0), tvs + (o0.double().abs() if acc else 0.0), n_terms + 1,
                               f"attn_tv[{shape},mask{int(masked)},acc{acc}]") <= 1.0


@pytest.mark.parametrize("Sq,Bq,Nk,Bk", [(51, 4, 9, 4), (33, 3, 65, 1), (7, 2, 330, 2), (1, 1, 1, 1)])
@pytest.mark.parametrize("H", [16, 64, 128, 256, 260, 384, 512])
def test_attention_weights(H, Sq, Bq, Nk, Bk):
    """ops.attention_weights on both sides of ATTN_MAX_H: the MFMA attention kernel (RAW_Q | NO_RESIDUAL) up to 256 columns,
    attn_dp + softmax_fwd beyond."""
    o = ops()
    assert o.ATTN_MAX_H == 256
    q, k = rnd(Sq * Bq, H, seed=81), rnd(Nk * Bk, H, seed=82)
    probs = torch.full((Bq, Sq, Nk), float("nan"), device=DEV)
    keep = o.attention_weights(q, k, probs, Sq, Bq, Nk, Bk, H)
    torch.cuda.synchronize()
    del keep
    scale = H ** -0.5
    Q = q.double().reshape(Sq, Bq, H).transpose(0, 1)                                                   # [Bq, Sq, H]
    Kt = k.double().reshape(Nk, Bk, H)[:, torch.arange(Bq, device=DEV) % Bk].permute(1, 2, 0)           # [Bq, H, Nk]
    a64 = scale * (Q @ Kt)
    P64 = torch.softmax(a64, -1)
    D = scale * (Q.abs() @ Kt.abs()).amax(-1, keepdim=True)         # the scores' own magnitude: scale sum |q||k|, row maximum
    # a score is a sum of H products in some order (the MFMA tiles' or, beyond 256, <= 32 roundings along a lane + butterfly):
    # <= dot eps D in the exponent argument; the shift and expf add eps (2K + 2) as in C_SOFTMAX; P carries twice the worst
    # argument error + <= 22 roundings of the row sum
    dot = 32 if H > o.ATTN_MAX_H else H
    sc = P64 * (2 * dot * D + 2 * (1 + 2 * a64.abs().amax(-1, keepdim=True)) + 32) + 2.0 ** -100
    branch = "mfma" if H <= o.ATTN_MAX_H else "dp+softmax"
    assert bound_ratio(probs, P64, sc, 2, f"attention_weights[{branch},H{H},Sq{Sq},Bq{Bq},Nk{Nk},Bk{Bk}]") <= 1.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.int32])
@pytest.mark.parametrize("n_jobs", [0, 1, 24, 25, 49])
def test_copy_many(n_jobs, dtype):
    """24 jobs per launch: every job bitwise equal to copy_ (random bit patterns, NaN payloads included), 16-byte aligned (vector
    path) and 4-byte aligned (scalar path) pointers, nothing written around a destination."""
    o = ops()
    lengths = [1, 3, 1023, 1025, 1 << 20]
    gen = torch.Generator().manual_seed(91)
    pairs, checks = [], []
    for i in range(n_jobs):
        n = lengths[i % len(lengths)]
        off = 1 if i % 3 == 2 else 4                    # element offset 1: not 16-byte aligned
        bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (n + 8,), generator=gen, dtype=torch.int32).to(DEV)
        dbuf = torch.full((n + 8,), 0x5EAD, dtype=torch.int32, device=DEV)
        src = (bits if dtype == torch.int32 else bits.view(torch.float32))[off:off + n]
        dst = (dbuf if dtype == torch.int32 else dbuf.view(torch.float32))[off:off + n]
        pairs.append((dst, src))
        checks.append((dbuf, off, n, bits))
    if n_jobs >= 25:                                    # an empty pair among them (the wrapper drops it)
        pairs.insert(7, (torch.empty(0, dtype=dtype, device=DEV), torch.empty(0, dtype=dtype, device=DEV)))
    o.copy_many(pairs)
    torch.cuda.synchronize()
    for dbuf, off, n, bits in checks:
        assert torch.equal(dbuf[off:off + n], bits[off:off + n])
        assert bool((dbuf[:off] == 0x5EAD).all()) and bool((dbuf[off + n:] == 0x5EAD).all())


@pytest.mark.parametrize("n", [1, 3, 255, 257, 1000, (1 << 20) + 3])
def test_fill(n):
    o = ops()
    for v in (2.5, -0.0):
        buf = torch.full((n + 9,), SENT, device=DEV)
        o.fill(buf[1:1 + n], v)
        torch.cuda.synchronize()
        assert torch.equal(buf[1:1 + n].view(torch.int32), torch.full((n,), v, device=DEV).view(torch.int32))   # bitwise, -0.0 too
        assert float(buf[0]) == SENT and bool((buf[1 + n:] == SENT).all())
