"""Long-double host references, bounds and guarded buffers shared by the float64 kernel tests (tests/test_gpu_f64_kernels.py,
tests/test_gpu_baselines64.py).  Nothing here touches the GPU at import; `python -m tests.f64_ref` prints, on the host alone,
the error of a plain float64 numpy restatement of the LayerNorm-type and edge-feature formulas against long double over the
inputs the tests use - the figures behind the constants C_* of tests/test_gpu_f64_kernels.py (4 x the worst ratio), never
taken from a kernel."""
import contextlib

import numpy as np
import torch

L = np.longdouble
U64 = 2.0 ** -53
SENT = 12345.0
DEV = "cuda"
LN_EPS = 1e-5
SLOPE_PRELU = 0.25


def need_long_double():
    assert np.finfo(L).eps <= 2.0 ** -63, "the host reference needs a long double wider than double"


def ld(t):
    """A tensor (or array) as a long-double numpy array on the host."""
    return (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).astype(L)


# ---- guarded buffers ------------------------------------------------------------------------------------------------
def guarded(*shape):
    """A NaN-filled contiguous float64 buffer, 16-byte aligned, between two sentinel pairs; -> (view, whole allocation)."""
    n = int(np.prod(shape))
    whole = torch.full((n + 4,), SENT, dtype=torch.float64, device=DEV)
    whole[2:2 + n] = float("nan")
    return whole[2:2 + n].view(*shape), whole


def assert_guards(name, view, whole):
    assert bool((whole[:2] == SENT).all()) and bool((whole[-2:] == SENT).all()), f"{name}: written outside the buffer"
    assert not bool(torch.isnan(view).any()), f"{name}: elements left unwritten"


@contextlib.contextmanager
def guarded_alloc(ops):
    """Scope in which every buffer the ops wrappers allocate (ops.alloc64: their outputs and scratch) is a guarded one;
    yields the list of (view, whole) handed out, in order."""
    made = []

    def alloc(device, *shape):
        made.append(guarded(*shape))
        return made[-1][0]

    before, ops.alloc64 = ops.alloc64, alloc
    try:
        yield made
    finally:
        ops.alloc64 = before


def in_slice(t, left=3, right=5, fill=SENT):
    """The 2-D tensor t as the column slice [:, left:left + W] of a wider buffer filled with `fill`; -> (slice, buffer)."""
    M, W = t.shape
    buf = torch.full((M, left + W + right), fill, dtype=t.dtype, device=t.device)
    buf[:, left:left + W] = t
    return buf[:, left:left + W], buf


def outside_untouched(buf, left, W, fill=SENT):
    keep = torch.ones_like(buf, dtype=torch.bool)
    keep[:, left:left + W] = False
    return bool((buf[keep] == fill).all())


# ---- bounds ---------------------------------------------------------------------------------------------------------
def bound_ratio(got, ref, bound):
    """Worst element-wise |got - ref| / bound in long double; <= 1 passes.  A zero bound demands the exact value; NaN fails."""
    err = np.abs(ld(got) - ref)
    if err.size == 0:
        return 0.0
    bound = np.broadcast_to(np.asarray(bound, dtype=L), err.shape)
    pos = bound > 0
    r = np.where(pos, err / np.where(pos, bound, L(1)), np.where(err > 0, L(np.inf), L(0)))
    r = np.where(np.isnan(err), L(np.inf), r)
    return float(np.max(r))


def sum_bound(n, mag):
    """(n + 4) 2^-53 sum|terms|: a sum of n float64 terms in any order errs by at most (n - 1 + a few roundings per term)
    2^-53 of the sum of their magnitudes; n (scalar or per element) is the element's own term count."""
    return (np.asarray(n, dtype=L) + L(4)) * L(U64) * mag


def check_sum(got, ref, mag, n):
    """Assert the sum bar per element (no element exempt); -> the worst error / bound."""
    err = np.abs(ld(got) - ref)
    bound = sum_bound(n, mag)
    worst = bound_ratio(got, ref, bound)
    assert bool(np.all(err <= bound)), worst
    return worst


# ---- inputs of the one-wave-per-row kernels ------------------------------------------------------------------------
ROW_M = [1, 2, 3, 4, 5, 9]
ROW_W = [1, 7, 63, 64, 65, 118, 1023, 1024]
# (M, W, with alpha) -> seeds skipped because the long-double reference breaks the sign guard there.  M 4, W 1: the only value of
# the 1e8 row gives y = beta = -0.012, under the guard's 2^-40 x 1e8 rstd
ROW_SEED_BUMP = {(4, 1, True): 1}


def row_values(M, W, seed):
    """[M, W] float64 rows on the host with magnitudes spread over 1e-2 .. 1e2; from M >= 2 the last row is constant
    (variance 0), from M >= 3 the one before sits on a common offset of 1e8 (a one-pass variance loses it all)."""
    g = torch.Generator().manual_seed(seed)
    z = (torch.randn(M, W, generator=g, dtype=torch.float64) * 3.0 + 0.5) * torch.logspace(-2, 2, M, dtype=torch.float64)[:, None]
    if M >= 2:
        z[M - 1] = 0.7
    if M >= 3:
        z[M - 2] = 1e8 + torch.randn(W, generator=g, dtype=torch.float64)
    return z


def ln_inputs(M, W, with_alpha):
    """-> z, gamma, beta, alpha (or None), dout on the host."""
    seed = 100000 * M + 10 * W + int(with_alpha) + 7 * ROW_SEED_BUMP.get((M, W, with_alpha), 0)
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    z = row_values(M, W, seed + 1)
    gamma, beta, dout = 1.0 + 0.5 * r(W), r(W), r(M, W)
    alpha = torch.tensor([SLOPE_PRELU], dtype=torch.float64) if with_alpha else None
    return z, gamma, beta, alpha, dout


def _np(t, T):
    return None if t is None else t.detach().cpu().numpy().astype(T)


def ln_forward(z, gamma, beta, alpha, T):
    """Two-pass LayerNorm (+ PReLU) of float64 operands in arithmetic T.  -> dict: xhat, rstd, out, and y (before PReLU);
    with the per-element scales of the bound C 2^-53 scale:
      xhat:  mean|z| rstd + |xhat|                     (the row's mean errs by 2^-53 mean|z|, the product by |xhat|)
      rstd:  rstd (1 + rstd^2 mean|z - mean| mean|z|)   (d rstd = -rstd^3 dvar / 2, dvar from the mean's error)
      out:   slope (scale_xhat |gamma| + |beta|),  slope = |alpha| where y < 0 else 1."""
    z, gamma, beta, a = _np(z, T), _np(gamma, T), _np(beta, T), _np(alpha, T)
    W = z.shape[1]
    mean = z.sum(1, keepdims=True) / T(W)
    t = z - mean
    rstd = T(1) / np.sqrt((t * t).sum(1, keepdims=True) / T(W) + T(LN_EPS))
    xhat = t * rstd
    r = dict(xhat=xhat, rstd=rstd[:, 0])
    mz = np.abs(z).mean(1, keepdims=True)
    sx = mz * rstd + np.abs(xhat)
    r["scale_xhat"], r["scale_rstd"] = sx, (rstd * (T(1) + rstd * rstd * np.abs(t).mean(1, keepdims=True) * mz))[:, 0]
    if gamma is not None:
        y = xhat * gamma + beta
        neg = (y < 0) if a is not None else np.zeros(y.shape, bool)
        r["y"], r["neg"] = y, neg
        r["out"] = np.where(neg, (a[0] if a is not None else T(0)) * y, y)
        r["scale_out"] = np.where(neg, np.abs(a[0]) if a is not None else T(1), T(1)) * (sx * np.abs(gamma) + np.abs(beta))
        r["guard"] = np.abs(y) >= T(2.0 ** -40) * (sx * np.abs(gamma) + np.abs(beta))     # stricter than |xhat gamma| + |beta|
    return r


def ln_backward(dout, xhat, rstd, gamma, beta, alpha, T):
    """LayerNorm (+ PReLU) backward from the stored xhat / rstd in arithmetic T.  -> dict: dz, p0 = g xhat, p1 = g, sa (the
    row's dalpha term), neg (the gate), and the scales
      dz:  rstd (|dxh| + mean|dxh| + |xhat| mean|dxh xhat|),  dxh = g gamma
      sa:  sum over y < 0 of |dout| (|xhat gamma| + |beta|)."""
    dout, xh, rs, gamma, beta, a = (_np(t, T) for t in (dout, xhat, rstd, gamma, beta, alpha))
    rs = rs[:, None]
    if a is not None:
        y = xh * gamma + beta
        neg = y < 0
        g = np.where(neg, dout * a[0], dout)
        sa = np.where(neg, dout * y, T(0)).sum(1)
        ssa = np.where(neg, np.abs(dout) * (np.abs(xh * gamma) + np.abs(beta)), T(0)).sum(1)
        guard = np.abs(y) >= T(2.0 ** -40) * (np.abs(xh * gamma) + np.abs(beta))
    else:
        neg, g, sa, ssa, guard = np.zeros(xh.shape, bool), dout, np.zeros(xh.shape[0], T), np.zeros(xh.shape[0], T), np.ones(xh.shape, bool)
    dxh = g * gamma if gamma is not None else g
    s1, s2 = dxh.mean(1, keepdims=True), (dxh * xh).mean(1, keepdims=True)
    dz = rs * (dxh - s1 - xh * s2)
    sdz = rs * (np.abs(dxh) + np.abs(dxh).mean(1, keepdims=True) + np.abs(xh) * np.abs(dxh * xh).mean(1, keepdims=True))
    return dict(dz=dz, p0=g * xh, p1=g, sa=sa, neg=neg, scale_dz=sdz, scale_sa=ssa, guard=guard)


# ---- edge features --------------------------------------------------------------------------------------------------
EDGE_E = [1, 255, 256, 257]
R_MAX = 4.0
EDGE_SPECIAL = [(0.0, 0.0, 0.0), (2.0, 0.0, 0.0), (0.0, -1.0, 0.0), (4.0, 0.0, 0.0), (0.0, 0.0, -5.0), (3.0, 4.0, 0.0), (0.0, 0.0, 4.0)]


def edge_vectors(E):
    """[E, 3] float64 on the host: the known-answer vectors first (as many as fit, the last of them also at E - 1), then random
    directions with lengths spread evenly over (0, 1.2 r_max)."""
    g = torch.Generator().manual_seed(900 + E)
    d = torch.randn(E, 3, generator=g, dtype=torch.float64)
    d = d / d.norm(dim=1, keepdim=True)
    lens = (torch.arange(E, dtype=torch.float64) + torch.rand(E, generator=g, dtype=torch.float64)) / E * (1.2 * R_MAX)
    v = d * lens[torch.randperm(E, generator=g)][:, None]
    k = min(E, len(EDGE_SPECIAL) - 1)
    v[:k] = torch.tensor(EDGE_SPECIAL[:k], dtype=torch.float64)
    if E > len(EDGE_SPECIAL):
        v[E - 1] = torch.tensor(EDGE_SPECIAL[-1], dtype=torch.float64)
    return v


def edge_feat(vec, r_max, T):
    """[cut, cut sqrt(3) v / |v|] in arithmetic T; the bound is C 2^-53 x (1 for cut, sqrt(3) for the three components)."""
    v = _np(vec, T)
    pi = T(np.pi) if T is not L else L(4) * np.arctan(L(1))
    ln = np.sqrt((v * v).sum(1))
    inv = T(1) / np.maximum(ln, T(1e-12))
    u = T(2) * (ln / T(r_max) - T(1))
    cut = (T(1) - np.cos(pi * u)) / T(2)
    cut = np.where(u > 0, T(0), cut)
    cut = np.where(u < -1, T(1), cut)
    return np.concatenate([cut[:, None], cut[:, None] * (np.sqrt(T(3)) * (v * inv[:, None]))], 1)


EDGE_SCALE = np.array([1.0] + 3 * [np.sqrt(3.0)])

# ---- dense rows -----------------------------------------------------------------------------------------------------
# (counts per crystal, nmax): a full crystal, an empty one, B nmax in {1, 3, 4, 5}, and a crystal with more nodes than nmax
DENSE_CASES = [([4, 1, 0, 3], 4), ([1], 1), ([3], 3), ([1, 0, 1], 1), ([2, 0], 2), ([4], 4), ([1, 1, 0, 1], 1), ([5], 5),
               ([1, 1, 1, 1, 1], 1), ([6, 1], 4)]


def dense_inputs(counts, nmax, H):
    """-> x [N, H], dout [B nmax, H], dx0 [N, H] (the gradient already there) on the host."""
    N, B = sum(counts), len(counts)
    seed = 1000 * H + 10 * N + nmax
    g = torch.Generator().manual_seed(seed)
    return (row_values(N, H, seed + 1), torch.randn(B * nmax, H, generator=g, dtype=torch.float64),
            torch.randn(N, H, generator=g, dtype=torch.float64))


def dense_rows(x, counts, nmax, T):
    """to_dense_batch + LayerNorm without affine in arithmetic T: -> rows [B nmax, H] (zero for the padding), their scale,
    rstd [N], its scale, node_of_row [B nmax] (-1: padding), reached [N]."""
    f = ln_forward(x, None, None, None, T)
    B, H = len(counts), x.shape[1]
    ptr = np.concatenate([[0], np.cumsum(counts)])
    node = np.full(B * nmax, -1)
    for b in range(B):
        k = min(counts[b], nmax)
        node[b * nmax:b * nmax + k] = np.arange(ptr[b], ptr[b] + k)
    rows, scale = np.zeros((B * nmax, H), T), np.zeros((B * nmax, H), T)
    rows[node >= 0], scale[node >= 0] = f["xhat"][node[node >= 0]], f["scale_xhat"][node[node >= 0]]
    reached = np.zeros(x.shape[0], bool)
    reached[node[node >= 0]] = True
    return rows, scale, f["rstd"], f["scale_rstd"], node, reached


# ---- the host-only measurement behind C_* ----------------------------------------------------------------------------
def _ratio(a64, ref, scale):
    return bound_ratio(a64, ref, L(U64) * scale)


def measure():
    """Worst |float64 numpy restatement - long double| / (2^-53 scale) per kernel family over the tests' own inputs, and the
    number of elements that break the sign guard (must be 0)."""
    need_long_double()
    worst = dict(layernorm=0.0, layernorm_bwd=0.0, dense_rows=0.0, dense_rows_bwd=0.0, edge_feat=0.0)
    broken = 0
    for M in ROW_M:
        for W in ROW_W:
            for wa in (False, True):
                z, gamma, beta, alpha, dout = ln_inputs(M, W, wa)
                a, b = ln_forward(z, gamma, beta, alpha, np.float64), ln_forward(z, gamma, beta, alpha, L)
                broken += int((~b["guard"]).sum()) if wa else 0
                worst["layernorm"] = max([worst["layernorm"]] + [_ratio(a[k], b[k], b["scale_" + k]) for k in ("xhat", "rstd", "out")])
                xh, rs = torch.from_numpy(a["xhat"]), torch.from_numpy(a["rstd"])
                a, b = ln_backward(dout, xh, rs, gamma, beta, alpha, np.float64), ln_backward(dout, xh, rs, gamma, beta, alpha, L)
                broken += int((~b["guard"]).sum())
                worst["layernorm_bwd"] = max(worst["layernorm_bwd"], _ratio(a["dz"], b["dz"], b["scale_dz"]),
                                             _ratio(a["sa"], b["sa"], b["scale_sa"]))
    for counts, nmax in DENSE_CASES:
        for H in (ROW_W if (counts, nmax) in (DENSE_CASES[0], DENSE_CASES[-1]) else [65]):
            x, dout, dx0 = dense_inputs(counts, nmax, H)
            a, b = dense_rows(x, counts, nmax, np.float64), dense_rows(x, counts, nmax, L)
            worst["dense_rows"] = max(worst["dense_rows"], _ratio(a[0], b[0], b[1]), _ratio(a[2], b[2], b[3]))
            node = b[4]
            live = node >= 0
            xh, rs = torch.from_numpy(a[0][live]), torch.from_numpy(a[2][node[live]])
            fa, fb = (ln_backward(dout[torch.from_numpy(live)], xh, rs, None, None, None, T) for T in (np.float64, L))
            for acc in (False, True):
                base = ld(dx0)[node[live]] if acc else L(0)
                got = fa["dz"] + (dx0.numpy()[node[live]] if acc else 0.0)
                worst["dense_rows_bwd"] = max(worst["dense_rows_bwd"], _ratio(got, fb["dz"] + base, fb["scale_dz"] + np.abs(base)))
    for E in EDGE_E:
        v = edge_vectors(E)
        worst["edge_feat"] = max(worst["edge_feat"], _ratio(edge_feat(v, R_MAX, np.float64), edge_feat(v, R_MAX, L), L(1) * EDGE_SCALE))
    return worst, broken


if __name__ == "__main__":
    w, broken = measure()
    for k, v in w.items():
        print(f"{k}: worst restatement error / (2^-53 scale) = {v:.3f}  ->  C = {4 * v:.3f}")
    print(f"elements that break the sign guard: {broken}")
