"""The elementwise, row and graph kernels of the float64 program (csrc/f64.hip; dense_rows64, dense_rows64_bwd and index_sum64 of
csrc/f64_attention.hip) on a real MI355X, at their edges: row tails and widths of the one-wave-per-row kernels, operands that
are column slices of wider buffers, absent optional operands, both accumulate settings, a purpose-built batch of crystals, and
every grid-stride kernel once past its grid cap of 8192 x 256 threads.  tests/test_gpu_f64.py holds the ordinary shapes.

Reference: long double on the host from the same float64 operands (tests/f64_ref.py).  Bars, per element, no element exempt:
  * copies, selections, single products and quotients: bitwise the same IEEE operation in float64 numpy / torch;
  * sums of n terms: |got - ref| <= (n + 4) 2^-53 sum|terms|, n the element's own term count (f64_ref.sum_bound);
  * LayerNorm-type kernels and edge_feat_sh1_64: |got - ref| <= C 2^-53 scale with the scales written down in f64_ref.ln_forward,
    f64_ref.ln_backward (dense_rows64 / dense_rows_bwd64: the same without affine, + |dx| already there when accumulating) and
    f64_ref.edge_feat (1 for cut, sqrt(3) for the components).  C is 4 x the worst error / (2^-53 scale) of a plain float64 numpy
    restatement of the same formulas against long double over these tests' own inputs, measured on the host alone
    (`python -m tests.f64_ref`), never from a kernel:
        layernorm64       5.714 (the constant row at W = 63: its float64 mean is not the constant)  -> C = 22.857
        layernorm_bwd64   2.269  -> C = 9.077
        dense_rows64      5.714  -> C = 22.857
        dense_rows_bwd64  2.068  -> C = 8.274
        edge_feat_sh1_64  3.788  -> C = 15.151
  * past the grid cap: small-integer operands, every sum exact, torch.equal against float64 torch.
The PReLU gate of the LayerNorm kernels: the inputs are chosen (and it is asserted) so that the long-double y = xhat gamma + beta
is nowhere within 2^-40 of its own scale of zero, so the kernel's gate cannot differ and no element is exempt.
Every kernel runs twice, bitwise equal; every output and scratch buffer lies between sentinels and starts as NaN.
ops.reduce_rows64 is left as it is (it never accumulates): the kernel's accumulate branch is tested through the C entry."""
import math
import types

import numpy as np
import pytest
import torch

from tests import f64_ref as R
from tests.f64_ref import DEV, L, SENT, U64, ld

pytestmark = pytest.mark.gpu

C_LN, C_LN_BWD, C_DENSE, C_DENSE_BWD, C_EDGE = 4 * 5.714, 4 * 2.269, 4 * 5.714, 4 * 2.068, 4 * 3.788
CAP = 8192 * 256                    # threads of a capped grid: flat index of the first element of a second pass
ROWS, COLS = 8200, 257              # past the cap, a width that does not divide 256


def _ops():
    from dostransformer_amd import ops
    return ops


def _dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


def _bits(t):
    return t.contiguous().view(torch.int64)


def _same(a, b):
    """Bitwise equal (NaN and the sign of zero included)."""
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _run(fn, nan_ok=False):
    """fn() with every buffer the wrappers allocate guarded: sentinels intact, and no NaN left in what fn returns."""
    with R.guarded_alloc(_ops()) as made:
        out = fn()
    torch.cuda.synchronize()
    for i, (_, whole) in enumerate(made):
        assert bool((whole[:2] == SENT).all()) and bool((whole[-2:] == SENT).all()), f"allocation {i}: written outside the buffer"
    outs = [t for t in (out if isinstance(out, (tuple, list)) else [out]) if torch.is_tensor(t)]
    assert nan_ok or not any(bool(torch.isnan(t).any()) for t in outs), "elements left unwritten"
    return out


def _twice(fn, nan_ok=False):
    a, b = _run(fn, nan_ok), _run(fn, nan_ok)
    la, lb = (list(t) if isinstance(t, (tuple, list)) else [t] for t in (a, b))
    assert all(_same(x, y) for x, y in zip(la, lb) if torch.is_tensor(x)), "two runs differ"
    return a


def _out_slice(M, W, base=None, left=2, right=6):
    """A caller-owned output: the column slice [:, left:left + W] of a sentinel-filled buffer, NaN (or `base`) inside."""
    buf = torch.full((M, left + W + right), SENT, dtype=torch.float64, device=DEV)
    buf[:, left:left + W] = float("nan") if base is None else base
    return buf[:, left:left + W], buf, left


def _out_flat(base_or_shape):
    """A caller-owned contiguous guarded output, NaN or holding `base`."""
    if torch.is_tensor(base_or_shape):
        view, whole = R.guarded(*base_or_shape.shape)
        view.copy_(base_or_shape)
    else:
        view, whole = R.guarded(*base_or_shape)
    return view, whole


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _spread(M, W, seed):
    """Rows whose magnitudes span 1e-3 .. 1e3: a wrong small row has to show next to large ones."""
    return _randn(M, W, seed=seed) * torch.logspace(-3, 3, max(M, 1), dtype=torch.float64)[:M, None]


# =====================================================================================================================
# 1. one wave per row, 4 rows per workgroup
# =====================================================================================================================
@pytest.mark.parametrize("with_alpha", [False, True])
@pytest.mark.parametrize("W", R.ROW_W)
def test_layernorm64_rows_and_widths(W, with_alpha):
    """layernorm64 / layernorm_bwd64 at M in {1, 2, 3, 4, 5, 9}: a constant row (rstd = 1 / sqrt(1e-5), xhat 0) and a row on an
    offset of 1e8 included.  The backward reads the host's float64 xhat / rstd, so its reference has the same operands."""
    R.need_long_double()
    o = _ops()
    worst = dict(xhat=0.0, rstd=0.0, out=0.0, dz=0.0, dalpha=0.0)
    for M in R.ROW_M:
        z, gamma, beta, alpha, dout = R.ln_inputs(M, W, with_alpha)
        ref = R.ln_forward(z, gamma, beta, alpha, L)
        assert not with_alpha or bool(ref["guard"].all()), "an input within 2^-40 of a sign change of y"
        zd, gd, bd, ad, dd = _dev(z, gamma, beta, alpha, dout)
        got = dict(zip(("xhat", "rstd", "out"), _twice(lambda: o.layernorm64(zd, gd, bd, ad))))
        for k in ("xhat", "rstd", "out"):
            r = R.bound_ratio(got[k], ref[k], L(C_LN * U64) * ref["scale_" + k])
            worst[k] = max(worst[k], r)
            assert r <= 1.0, (k, M, W, r)
        if M >= 2:                              # the constant row: variance 0 in any arithmetic
            assert float(got["rstd"][M - 1]) == pytest.approx(1e-5 ** -0.5, rel=1e-12)
        host = R.ln_forward(z, gamma, beta, alpha, np.float64)
        xh, rs = torch.from_numpy(host["xhat"]), torch.from_numpy(host["rstd"])
        ref = R.ln_backward(dout, xh, rs, gamma, beta, alpha, L)
        assert bool(ref["guard"].all()), "a stored xhat within 2^-40 of a sign change of y"
        xd, rd = _dev(xh, rs)
        dz, part = _twice(lambda: o.layernorm_bwd64(dd, xd, rd, gd, bd, ad))
        assert tuple(part.shape) == (M, 2 * W + 1)
        g = np.where(ref["neg"], dout.numpy() * R.SLOPE_PRELU, dout.numpy())          # float64: the kernel's own two products
        assert _same(part[:, :W].cpu(), torch.from_numpy(g * xh.numpy())) and _same(part[:, W:2 * W].cpu(), torch.from_numpy(g))
        for k, got_k, ref_k, sc in (("dz", dz, ref["dz"], ref["scale_dz"]), ("dalpha", part[:, 2 * W], ref["sa"], ref["scale_sa"])):
            r = R.bound_ratio(got_k, ref_k, L(C_LN_BWD * U64) * sc)
            worst[k] = max(worst[k], r)
            assert r <= 1.0, (k, M, W, r)
    print(f"layernorm64 W{W} alpha={with_alpha}: worst error / bound " + ", ".join(f"{k} {w:.3f}" for k, w in worst.items()))


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("act", ["relu", "leaky", "prelu"])
def test_act_bwd64_strides_and_zeros(act, wide):
    """dz bitwise the selection / single product; PReLU's part under the sum bar with n = the row's negative entries.  z also
    as a column slice (ld > W: act64_bwd_kernel indexes dy with W and z with ld).  z == 0.0 and z == -0.0 under a live dy: ReLU
    and leaky take the <= 0 side, PReLU the >= 0 side and adds nothing to part."""
    R.need_long_double()
    o = _ops()
    code = dict(relu=o.ACT64_RELU, leaky=o.ACT64_LEAKY, prelu=o.ACT64_PRELU)[act]
    a = 0.2
    alpha = torch.tensor([a], dtype=torch.float64, device=DEV)
    worst = 0.0
    for M in R.ROW_M:
        for W in [1, 45, 64, 65, 200]:
            z, dy = _spread(M, W, 7 * M + W), _randn(M, W, seed=11 * M + W)
            z[M - 1, 0], z[M // 2, W - 1] = 0.0, -0.0
            if W > 1:
                z[0, W // 2] = -0.0
            assert float(dy[M - 1, 0]) != 0.0 and float(dy[M // 2, W - 1]) != 0.0
            zd, dyd = _dev(z, dy)
            if wide:
                zd, zbuf = R.in_slice(zd, 3, 5)
                assert zd.stride(0) == W + 8
            dz, part = _twice(lambda: o.act_bwd64(dyd, zd, code, alpha if act == "prelu" else None))
            zn, dn = z.numpy(), dy.numpy()
            want = dict(relu=np.where(zn > 0, dn, 0.0), leaky=np.where(zn > 0, dn, dn * 0.01), prelu=np.where(zn >= 0, dn, dn * a))[act]
            assert _same(dz.cpu(), torch.from_numpy(want)), (act, M, W)
            if act == "prelu":
                neg = zn < 0
                t = np.where(neg, ld(dy) * ld(z), L(0))
                worst = max(worst, R.check_sum(part[:, 0], t.sum(1), np.abs(t).sum(1), neg.sum(1)))
            else:
                assert part is None
    if act == "prelu":
        print(f"act_bwd64 prelu wide={wide}: worst part error / bound {worst:.3f}")


@pytest.mark.parametrize("M", [0, 1, 255, 256, 257, 512, 513])
def test_colsum64_around_the_row_block(M):
    """DOSX_COLSUM64_ROWS = 256 rows per partial sum: one block, one full block, the second and third block's first row."""
    R.need_long_double()
    o = _ops()
    assert o.COLSUM64_ROWS == 256
    worst = 0.0
    for N in [1, 63, 64, 65, 130]:
        full = _spread(M + 1, N, 3 * M + N).to(DEV)
        base = _randn(N, seed=5 * M + N)
        for sliced in (False, True):
            src = R.in_slice(full, 1, 4)[0] if sliced else full
            for acc in (False, True):
                def run():
                    out, whole = _out_flat(base.to(DEV)) if acc else _out_flat((N,))
                    if M:
                        o.colsum64(src[:M], out, accumulate=acc)
                    else:                       # no rows: an empty tensor has no address, so the C entry with a live one
                        o._call("dosx_colsum_f64", src.data_ptr(), 0, N, src.stride(0), None, out.data_ptr(), int(acc), o._stream())
                    torch.cuda.synchronize()
                    R.assert_guards("colsum64 out", out, whole)
                    return out
                out = _twice(run)
                t = ld(full[:M])
                ref, mag = t.sum(0) + (ld(base) if acc else 0), np.abs(t).sum(0) + (np.abs(ld(base)) if acc else 0)
                worst = max(worst, R.check_sum(out, ref, mag, M + int(acc)))
                if M == 0:                      # an empty sum: zero, or what was there
                    assert torch.equal(out.cpu(), base if acc else torch.zeros(N, dtype=torch.float64))
    print(f"colsum64 M{M}: worst error / bound {worst:.3f}")


def _wgrad_case(M, seed):
    """N = 70, K = 29 + 5: dy, a gathered segment x[idx] and a plain one e, each the first M rows of a live buffer (also returned:
    no rows have no address of their own); the long-double dw and the sums of magnitudes."""
    N, Hx, He = 70, 29, 5
    dy, x, e = _randn(M + 1, N, seed=seed).to(DEV), _randn(40, Hx, seed=seed + 1).to(DEV), _randn(M + 1, He, seed=seed + 2).to(DEV)
    idx = torch.randint(0, 40, (M + 1,), generator=torch.Generator().manual_seed(seed + 3)).to(torch.int32).to(DEV)
    X = torch.cat([x[idx[:M].long()], e[:M]], 1)
    t = ld(dy[:M])[:, :, None] * ld(X)[:, None, :]                         # [M, N, K]
    return N, Hx + He, dy, x, e, idx, t.sum(0), np.abs(t).sum(0)


def _wgrad_entry(M, dy, segs, dw, accumulate, nsplit, partials):
    """dosx_wgrad_f64 through its C entry, the descriptor filled as ops.wgrad64 fills it."""
    import ctypes as C
    from dostransformer_amd import _lib
    o = _ops()
    d = _lib.Wgrad64()
    d.M, (d.N, d.K), d.nseg = M, dw.shape, len(segs)
    d.dy, d.lddy = dy.data_ptr(), dy.stride(0)
    for i, s in enumerate(segs):
        d.x[i] = s
    d.dw, d.ldd, d.accumulate, d.nsplit = dw.data_ptr(), dw.stride(0), int(accumulate), nsplit
    d.partials = None if partials is None else partials.data_ptr()
    o._call("dosx_wgrad_f64", C.byref(d), o._stream())


@pytest.mark.parametrize("M", [0, 1, 511, 1023, 1024, 1025, 1027])
def test_wgrad64_around_the_first_split(M):
    """_WGRAD64_ROWS = 512 rows per split: no rows, one split up to M = 1023, two from 1024, chunks rounded up to a multiple of
    4 (1025, 1027: 516 + the rest).  N = 70, K = 34 (no multiples of 64), a gathered and a plain segment, dw a column slice.
    M = 0 goes through the C entry with the operands' live addresses (an empty tensor has none): dw zero, or unchanged."""
    R.need_long_double()
    o = _ops()
    assert o._WGRAD64_ROWS == 512
    N, K, dy, x, e, idx, ref, mag = _wgrad_case(M, 40 + M)
    base = _randn(N, K, seed=M + 1)
    for acc in (False, True):
        def run():
            dw, buf, left = _out_slice(N, K, base.to(DEV) if acc else None)
            if M:
                o.wgrad64(M, dy[:M], [o.seg64(x, o.rowmap(idx=idx[:M])), o.seg64(e[:M])], dw, accumulate=acc)
            else:
                _wgrad_entry(0, dy, [o.seg64(x, o.rowmap(idx=idx)), o.seg64(e)], dw, acc, 1, None)
            torch.cuda.synchronize()
            assert R.outside_untouched(buf, left, K) and dw.stride(0) > K
            return dw
        dw = _twice(run)
        worst = R.check_sum(dw, ref + (ld(base) if acc else 0), mag + (np.abs(ld(base)) if acc else 0), M + int(acc))
        if M == 0:
            assert torch.equal(dw.cpu(), base if acc else torch.zeros(N, K, dtype=torch.float64))
        print(f"wgrad64 M{M} accumulate={acc}: worst error / bound {worst:.3f}")


def test_wgrad64_fewer_live_splits_than_requested():
    """Through the C entry: M = 9 with 8 splits asked for gives chunks of 4 rows, so 3 row ranges hold rows; the reduction must
    add those 3 and not the 5 partial slabs that were never written (they stay NaN here)."""
    R.need_long_double()
    o = _ops()
    M = 9
    N, K, dy, x, e, idx, ref, mag = _wgrad_case(M, 77)

    def run():
        dw, buf, left = _out_slice(N, K)
        part, whole = R.guarded(8, N, K)
        _wgrad_entry(M, dy, [o.seg64(x, o.rowmap(idx=idx)), o.seg64(e)], dw, False, 8, part)
        torch.cuda.synchronize()
        assert R.outside_untouched(buf, left, K) and bool((whole[:2] == SENT).all()) and bool((whole[-2:] == SENT).all())
        assert not bool(torch.isnan(part[:3]).any()) and bool(torch.isnan(part[3:]).all())
        return dw
    print(f"wgrad64 M9 in 8 splits: worst error / bound {R.check_sum(_twice(run), ref, mag, M):.3f}")


# =====================================================================================================================
# 2. graph kernels on a purpose-built batch
# =====================================================================================================================
GRAPH_H = [1, 12, 64, 65]


def _crystal(g, n, ei):
    ei = torch.tensor(ei)
    return {"x": torch.rand(n, 118, generator=g, dtype=torch.float64), "edge_index": ei,
            "edge_vec": (torch.rand(ei.shape[1], 3, generator=g, dtype=torch.float64) * 2 - 1) * 3.0,
            "system": torch.tensor(1), "phdos": torch.rand(1, 51, generator=g, dtype=torch.float64)}


@pytest.fixture(scope="module")
def graph():
    """6 crystals, 85 nodes, 168 edges: one atom with only a self edge; a crystal with an isolated node (no edge in or out) and
    a triple edge; an ordinary one; 70 atoms whose node 0 has 70 incoming edges (more than a wave); a small ring; and a last
    crystal whose last node - the last of the batch - has no incoming edge, so the row pointers close on an empty segment."""
    from dostransformer_amd.batch import collate, graph_meta
    g = torch.Generator().manual_seed(1)
    big = [list(range(70)) + list(range(70)), [0] * 70 + [(i + 1) % 70 for i in range(70)]]
    cs = [_crystal(g, 1, [[0], [0]]), _crystal(g, 4, [[0, 0, 0, 1, 2], [1, 1, 1, 0, 2]]),
          _crystal(g, 5, [[i % 5 for i in range(17)], [(3 * i + 1) % 5 for i in range(17)]]), _crystal(g, 70, big),
          _crystal(g, 3, [[0, 1, 2, 0], [1, 2, 0, 2]]), _crystal(g, 2, [[1], [0]])]
    gb = collate(cs)
    m = graph_meta(gb, DEV)
    src, dst = m.src.cpu().numpy().astype(np.int64), m.dst.cpu().numpy().astype(np.int64)
    N, E, B = m.num_nodes, m.num_edges, m.num_graphs
    assert (N, E, B) == (85, 168, 6)
    deg_in, deg_out = np.bincount(dst, minlength=N), np.bincount(src, minlength=N)
    assert deg_in.max() > 64 and deg_in[N - 1] == 0 and deg_in[4] == 0 and deg_out[4] == 0 and deg_in[2] >= 3
    return types.SimpleNamespace(m=m, src=src, dst=dst, N=N, E=E, B=B, deg_in=deg_in, deg_out=deg_out,
                                 node_graph=gb.batch.numpy().astype(np.int64))


def _scatter(rows, index, n):
    """Long-double sums of rows by index: (sum, sum of magnitudes, count) per target."""
    rows = ld(rows)
    ref, mag = np.zeros((n, rows.shape[1]), L), np.zeros((n, rows.shape[1]), L)
    np.add.at(ref, index, rows)
    np.add.at(mag, index, np.abs(rows))
    return ref, mag, np.bincount(index, minlength=n)


@pytest.mark.parametrize("H", GRAPH_H)
def test_segment_mean64_and_its_backward(graph, H):
    R.need_long_double()
    o, m = _ops(), graph.m
    N, E = graph.N, graph.E
    msg = _spread(E, H, 3 + H)
    ref, mag, cnt = _scatter(msg, graph.dst, N)
    div = np.maximum(cnt, 1).astype(L)[:, None]
    msg_d = msg.to(DEV)
    agg = _twice(lambda: o.segment_mean64(msg_d, m.rowptr_dst, N))
    w0 = R.check_sum(agg, ref / div, mag / div, cnt[:, None])              # in-degree 0: exactly 0
    assert tuple(agg.shape) == (N, H) and bool((agg[N - 1] == 0).all()) and bool((agg[4] == 0).all())
    dagg, res = _spread(N, H, 5 + H), _randn(E, H, seed=7 + H)
    dagg_d = R.in_slice(dagg.to(DEV), H + 1, 2)[0]                         # dcat2[:, H:] of the program: row stride > H
    res_d = res.to(DEV)
    out = _twice(lambda: o.segment_mean_bwd64(dagg_d, m.dst, m.rowptr_dst, res_d, E))
    v = ld(dagg)[graph.dst] / div[graph.dst]
    w1 = R.check_sum(out, ld(res) + v, np.abs(ld(res)) + np.abs(v), 2)
    out = _twice(lambda: o.segment_mean_bwd64(dagg_d, m.dst, m.rowptr_dst, None, E))
    want = dagg.numpy()[graph.dst] / np.maximum(cnt, 1).astype(np.float64)[graph.dst][:, None]       # one IEEE division
    assert _same(out.cpu(), torch.from_numpy(want))
    print(f"segment_mean64 H{H}: worst error / bound forward {w0:.3f}, backward {w1:.3f}")


@pytest.mark.parametrize("H", GRAPH_H)
def test_gather_bwd64_optional_bases(graph, H):
    """dx[n] = base0[n] + base1[n] + sum over the edges out of n of dcat[e, :H] + sum over the edges into n of dcat[e, H:2H],
    dcat 3H wide, each base present or absent and a column slice of a wider buffer with its own row stride."""
    R.need_long_double()
    o, m = _ops(), graph.m
    N, E = graph.N, graph.E
    dcat = _spread(E, 3 * H, 9 + H)
    b0, b1 = _randn(N, H, seed=11 + H), _spread(N, H, 13 + H)
    dcat_d = dcat.to(DEV)
    b0_d, b1_d = R.in_slice(b0.to(DEV), 2, 3)[0], R.in_slice(b1.to(DEV), 2 * H, 1)[0]
    s_ref, s_mag, s_cnt = _scatter(dcat[:, :H], graph.src, N)
    d_ref, d_mag, d_cnt = _scatter(dcat[:, H:2 * H], graph.dst, N)
    worst = 0.0
    for use0 in (True, False):
        for use1 in (True, False):
            dx = _twice(lambda: o.gather_bwd64(dcat_d, m, b0_d if use0 else None, b1_d if use1 else None, N, H))
            ref = s_ref + d_ref + (ld(b0) if use0 else 0) + (ld(b1) if use1 else 0)
            mag = s_mag + d_mag + (np.abs(ld(b0)) if use0 else 0) + (np.abs(ld(b1)) if use1 else 0)
            worst = max(worst, R.check_sum(dx, ref, mag, (s_cnt + d_cnt + int(use0) + int(use1))[:, None]))
            if not (use0 or use1):
                assert bool((dx[4] == 0).all())                            # the isolated node: no term at all
    print(f"gather_bwd64 H{H}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("H", GRAPH_H)
def test_graph_pool64_and_rows_add64(graph, H):
    R.need_long_double()
    o, m = _ops(), graph.m
    N, E, B = graph.N, graph.E, graph.B
    x = _spread(N, H, 15 + H)
    ref, mag, cnt = _scatter(x, graph.node_graph, B)
    x_d = x.to(DEV)
    pool = _twice(lambda: o.graph_pool64(x_d, m.graph_ptr, B))
    w0 = R.check_sum(pool, ref, mag, cnt[:, None])
    # rows_add64: a and b column slices with different row strides; one operand: a copy, bitwise
    a_n, b_n, a_e, b_e = _spread(N, H, 17 + H), _randn(N, H, seed=19 + H), _randn(E, H, seed=21 + H), _spread(E, H, 23 + H)
    an_d, bn_d = R.in_slice(a_n.to(DEV), 1, 2)[0], R.in_slice(b_n.to(DEV), H + 3, 0)[0]
    ae_d, be_d = R.in_slice(a_e.to(DEV), 4, 4)[0], R.in_slice(b_e.to(DEV), 0, 7)[0]
    src_i, dst_i = m.src, m.dst
    assert _same(_twice(lambda: o.rows_add64(E, ae_d)), ae_d)
    assert _same(_twice(lambda: o.rows_add64(E, an_d, ia=dst_i)), an_d[dst_i.long()])
    back = _twice(lambda: o.rows_add64(N, pool, ia=m.node_graph))          # the program's broadcast of the pooled rows
    assert _same(back, pool[m.node_graph.long()])
    w1 = 0.0
    for a, b, ia, ib, ra, rb in [(ae_d, be_d, None, None, ld(a_e), ld(b_e)),
                                 (an_d, be_d, dst_i, None, ld(a_n)[graph.dst], ld(b_e)),
                                 (ae_d, bn_d, None, src_i, ld(a_e), ld(b_n)[graph.src]),
                                 (an_d, bn_d, dst_i, src_i, ld(a_n)[graph.dst], ld(b_n)[graph.src])]:
        out = _twice(lambda: o.rows_add64(E, a, b, ia=ia, ib=ib))
        assert tuple(out.shape) == (E, H)
        w1 = max(w1, R.check_sum(out, ra + rb, np.abs(ra) + np.abs(rb), 2))
    print(f"graph_pool64 H{H}: worst error / bound {w0:.3f}; rows_add64 {w1:.3f}")


@pytest.mark.parametrize("H", GRAPH_H)
def test_reduce_rows64_strides_and_accumulate(graph, H):
    """The program's two patterns - sum over the crystals of an energy (stride_out B, stride_red 1) and over the energies of a
    crystal (1, B) - and their transposes, n_red 0 (zeros) and 1 (a copy), src and out= column slices; the kernel's accumulate
    through the C entry (ops.reduce_rows64 never asks for it)."""
    R.need_long_double()
    o = _ops()
    S, B = 7, graph.B
    t = _spread(S * B, H, 25 + H)
    t_d = R.in_slice(t.to(DEV), 2, 1)[0]
    tl = ld(t)
    worst = 0.0
    for n_out, n_red, so, sr in [(S, B, B, 1), (B, S, 1, B), (B, S, S, 1), (S, B, 1, S), (S, 0, B, 1), (S, 1, B, 1)]:
        rows = np.arange(n_out)[:, None] * so + np.arange(n_red)[None, :] * sr
        ref, mag = tl[rows].sum(1), np.abs(tl[rows]).sum(1)
        out = _twice(lambda: o.reduce_rows64(t_d, n_out, n_red, so, sr))
        worst = max(worst, R.check_sum(out, ref, mag, n_red))
        base = _randn(n_out, H, seed=27 + H)

        def run(acc):
            dst, buf, left = _out_slice(n_out, H, base.to(DEV) if acc else None)
            if acc:
                o._call("dosx_reduce_rows_f64", t_d.data_ptr(), t_d.stride(0), dst.data_ptr(), dst.stride(0), n_out, n_red, so, sr,
                        H, 1, o._stream())
            else:
                assert o.reduce_rows64(t_d, n_out, n_red, so, sr, out=dst) is dst
            torch.cuda.synchronize()
            assert R.outside_untouched(buf, left, H)
            return dst
        worst = max(worst, R.check_sum(_twice(lambda: run(False)), ref, mag, n_red))
        worst = max(worst, R.check_sum(_twice(lambda: run(True)), ref + ld(base), mag + np.abs(ld(base)), n_red + 1))
    print(f"reduce_rows64 H{H}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("H", GRAPH_H)
def test_index_sum64_missing_index_and_accumulate(graph, H):
    """idx = the nodes' crystals with two more targets than crystals (indices that never occur: zero, or left alone when
    accumulating), then every row to one index; src and out column slices."""
    R.need_long_double()
    o = _ops()
    N, n_dst = graph.N, graph.B + 2
    src = _spread(N, H, 29 + H)
    src_d = R.in_slice(src.to(DEV), 3, 2)[0]
    base = _randn(n_dst, H, seed=31 + H)
    worst = 0.0
    for idx in (graph.node_graph, np.full(N, 3)):
        idx_d = torch.from_numpy(idx.astype(np.int32)).to(DEV)
        ref, mag, cnt = _scatter(src, idx, n_dst)
        for acc in (False, True):
            def run():
                out, buf, left = _out_slice(n_dst, H, base.to(DEV) if acc else None)
                assert o.index_sum64(src_d, idx_d, out, accumulate=acc) is out
                torch.cuda.synchronize()
                assert R.outside_untouched(buf, left, H)
                return out
            out = _twice(run)
            worst = max(worst, R.check_sum(out, ref + (ld(base) if acc else 0), mag + (np.abs(ld(base)) if acc else 0),
                                           (cnt + int(acc))[:, None]))
            assert torch.equal(out[n_dst - 1].cpu(), base[n_dst - 1] if acc else torch.zeros(H, dtype=torch.float64))
    print(f"index_sum64 H{H}: worst error / bound {worst:.3f}")


def _dense_cases():
    wide = (R.DENSE_CASES[0], R.DENSE_CASES[-1])
    return [(c, n, H) for c, n in R.DENSE_CASES for H in (R.ROW_W if (c, n) in wide else [65])]


@pytest.mark.parametrize("counts,nmax,H", _dense_cases(), ids=lambda v: "-".join(map(str, v)) if isinstance(v, list) else str(v))
def test_dense_rows64_and_its_backward(counts, nmax, H):
    """to_dense_batch + LayerNorm without affine: a crystal that fills all nmax slots, an empty one, B nmax in {1, 3, 4, 5}.
    include/dosx.h promises out[b nmax + j] for j < nmax only, so of a crystal with more than nmax nodes (counts [6, 1], nmax
    4) the first nmax are normalised and the others are not reached: their rstd and, in the backward, their dx stay untouched -
    as does the dx of every node when its row is padding.  Padding rows are exact zeros."""
    R.need_long_double()
    o = _ops()
    B, N = len(counts), sum(counts)
    x, dout, dx0 = R.dense_inputs(counts, nmax, H)
    rows, srows, rstd, srstd, node, reached = R.dense_rows(x, counts, nmax, L)
    assert reached.all() == (max(counts) <= nmax)
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device=DEV)
    x_d, dout_d = _dev(x, dout)
    out, rs = _twice(lambda: o.dense_rows64(x_d, ptr, B, nmax), nan_ok=True)
    assert not bool(torch.isnan(out).any()) and tuple(out.shape) == (B * nmax, H) and tuple(rs.shape) == (N,)
    w0 = R.bound_ratio(out, rows, L(C_DENSE * U64) * srows)                # padding: scale 0, exact zeros
    live_n = torch.from_numpy(reached)
    assert bool(torch.isnan(rs.cpu()[~live_n]).all()) and not bool(torch.isnan(rs.cpu()[live_n]).any())
    w1 = R.bound_ratio(rs.cpu()[live_n], rstd[reached], L(C_DENSE * U64) * srstd[reached])
    assert w0 <= 1.0 and w1 <= 1.0, (w0, w1)
    # backward from the host's float64 rows / rstd
    h_rows, _, h_rstd, _, _, _ = R.dense_rows(x, counts, nmax, np.float64)
    live = node >= 0
    ref = R.ln_backward(dout[torch.from_numpy(live)], torch.from_numpy(h_rows[live]), torch.from_numpy(h_rstd[node[live]]),
                        None, None, None, L)
    xh_d, hr_d = _dev(torch.from_numpy(h_rows), torch.from_numpy(h_rstd))
    w2 = 0.0
    for acc in (False, True):
        def run():
            dx, whole = _out_flat(dx0.to(DEV))
            assert o.dense_rows_bwd64(dout_d, xh_d, hr_d, ptr, dx, B, nmax, accumulate=acc) is dx
            torch.cuda.synchronize()
            R.assert_guards("dense_rows_bwd64 dx", dx, whole)
            return dx
        dx = _twice(run).cpu()
        assert _same(dx[~live_n], dx0[~live_n])                            # nodes the call does not reach
        base = ld(dx0)[node[live]] if acc else L(0)
        r = R.bound_ratio(dx[torch.from_numpy(node[live])], ref["dz"] + base, L(C_DENSE_BWD * U64) * (ref["scale_dz"] + np.abs(base)))
        w2 = max(w2, r)
        assert r <= 1.0, (acc, r)
    print(f"dense_rows64 {counts} nmax{nmax} H{H}: worst error / bound rows {w0:.3f}, rstd {w1:.3f}, dx {w2:.3f}")


# =====================================================================================================================
# 3. edge_feat_sh1_64
# =====================================================================================================================
@pytest.mark.parametrize("E", R.EDGE_E)
def test_edge_feat_sh1_64_known_answers_and_random_vectors(E):
    """r_max = 4.  The zero vector gives [1, 0, 0, 0]; |v| <= 2 gives cut == 1.0 exactly; |v| >= 4 gives four exact zeros; the
    rest against long double: C 2^-53 x (1 for cut, sqrt(3) for the components)."""
    R.need_long_double()
    o = _ops()
    v = R.edge_vectors(E)
    v_d = v.to(DEV)
    out = _twice(lambda: o.edge_feat_sh1_64(v_d, R.R_MAX)).cpu()
    assert tuple(out.shape) == (E, 4)
    ln = ld(v)
    ln = np.sqrt((ln * ln).sum(1))
    assert out[0].tolist() == [1.0, 0.0, 0.0, 0.0]
    if E > len(R.EDGE_SPECIAL):
        s3 = math.sqrt(3.0)
        assert out[1].tolist() == [1.0, s3, 0.0, 0.0] and out[2].tolist() == [1.0, 0.0, -s3, 0.0]
        assert all(out[i].tolist() == [0.0, 0.0, 0.0, 0.0] for i in (3, 4, 5, E - 1))
        assert (ln < 2).sum() > E // 8 and (ln > 4).sum() > E // 16 and ((ln > 2) & (ln < 4)).sum() > E // 4
    assert bool((out[torch.from_numpy((ln <= 2).astype(bool)), 0] == 1.0).all())
    assert bool((out[torch.from_numpy((ln >= 4).astype(bool))] == 0.0).all())
    worst = R.bound_ratio(out, R.edge_feat(v, R.R_MAX, L), L(C_EDGE * U64) * R.EDGE_SCALE)
    print(f"edge_feat_sh1_64 E{E}: worst error / bound {worst:.3f}")
    assert worst <= 1.0


# =====================================================================================================================
# 4. past the grid cap: 8200 x 257 elements > 8192 x 256 threads, small integers, every sum exact
# =====================================================================================================================
def _ints(*shape, seed, lo=-8, hi=9, mult=1):
    return (torch.randint(lo, hi, shape, generator=torch.Generator().manual_seed(seed)) * mult).double().to(DEV)


def _i32(a):
    return torch.as_tensor(a).to(torch.int32).to(DEV)


def _exact(name, got, want):
    """The first element of the second pass and the last one by name, then all of them."""
    assert got.shape == want.shape and got.numel() > CAP, name
    g, w = got.reshape(-1), want.reshape(-1)
    assert float(g[CAP]) == float(w[CAP]), f"{name}: flat element 2^21, the first of the grid's second pass"
    assert float(g[-1]) == float(w[-1]), f"{name}: the last element"
    assert torch.equal(got, want), name


def _segments(n, pattern):
    """Sorted targets with the given cycle of segment lengths: (index [E] int64 on the device, pointers [n + 1], counts)."""
    cnt = torch.tensor(pattern).repeat((n + len(pattern) - 1) // len(pattern))[:n]
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), cnt.cumsum(0)])
    return torch.repeat_interleave(torch.arange(n), cnt).to(DEV), ptr, cnt.to(DEV)


def test_past_the_grid_cap_segment_mean64():
    o = _ops()
    dst, ptr, cnt = _segments(ROWS, [0, 1, 2, 4, 3])
    msg = _ints(dst.numel(), COLS, seed=1)
    agg = _twice(lambda: o.segment_mean64(msg, _i32(ptr), ROWS))
    want = torch.zeros(ROWS, COLS, dtype=torch.float64, device=DEV).index_add(0, dst, msg) / cnt.clamp(min=1).double()[:, None]
    _exact("segment_mean64", agg, want)


def test_past_the_grid_cap_segment_mean_bwd64():
    o = _ops()
    n = ROWS // 2
    dst, ptr, cnt = _segments(n, [0, 1, 2, 4, 3])
    E = dst.numel()
    assert E == ROWS
    dagg = R.in_slice(_ints(n, COLS, seed=2, mult=12), COLS, 3)[0]         # multiples of 12: every quotient exact
    res = _ints(E, COLS, seed=3)
    out = _twice(lambda: o.segment_mean_bwd64(dagg, _i32(dst), _i32(ptr), res, E))
    _exact("segment_mean_bwd64", out, res + dagg[dst] / cnt.clamp(min=1).double()[dst][:, None])


def test_past_the_grid_cap_gather_bwd64():
    o = _ops()
    dst, ptr_dst, _ = _segments(ROWS, [0, 1, 2, 4, 3])
    E = dst.numel()
    src = torch.randint(0, ROWS, (E,), generator=torch.Generator().manual_seed(4))
    perm = torch.argsort(src, stable=True)
    ptr_src = torch.cat([torch.zeros(1, dtype=torch.int64), torch.bincount(src, minlength=ROWS).cumsum(0)])
    m = types.SimpleNamespace(rowptr_src=_i32(ptr_src), perm_src=_i32(perm), rowptr_dst=_i32(ptr_dst))
    dcat = _ints(E, 3 * COLS, seed=5)
    b0, b1 = R.in_slice(_ints(ROWS, COLS, seed=6), 1, 2)[0], R.in_slice(_ints(ROWS, COLS, seed=7), COLS, 0)[0]
    dx = _twice(lambda: o.gather_bwd64(dcat, m, b0, b1, ROWS, COLS))
    want = (b0 + b1).index_add(0, src.to(DEV), dcat[:, :COLS]).index_add(0, dst, dcat[:, COLS:2 * COLS])
    _exact("gather_bwd64", dx, want)


def test_past_the_grid_cap_graph_pool64():
    o = _ops()
    node_graph, ptr, _ = _segments(ROWS, [1, 2, 3, 4, 0])
    x = _ints(node_graph.numel(), COLS, seed=8)
    pool = _twice(lambda: o.graph_pool64(x, _i32(ptr), ROWS))
    _exact("graph_pool64", pool, torch.zeros(ROWS, COLS, dtype=torch.float64, device=DEV).index_add(0, node_graph, x))


def test_past_the_grid_cap_rows_add64():
    o = _ops()
    a, b = R.in_slice(_ints(500, COLS, seed=9), 2, 1)[0], R.in_slice(_ints(300, COLS, seed=10), 0, 5)[0]
    g = torch.Generator().manual_seed(11)
    ia, ib = torch.randint(0, 500, (ROWS,), generator=g), torch.randint(0, 300, (ROWS,), generator=g)
    out = _twice(lambda: o.rows_add64(ROWS, a, b, ia=_i32(ia), ib=_i32(ib)))
    _exact("rows_add64", out, a[ia.to(DEV)] + b[ib.to(DEV)])


def test_past_the_grid_cap_reduce_rows64():
    o = _ops()
    src = R.in_slice(_ints(3 * ROWS, COLS, seed=12), 1, 1)[0]
    out = _twice(lambda: o.reduce_rows64(src, ROWS, 3, 3, 1))
    _exact("reduce_rows64", out, src.reshape(ROWS, 3, COLS).sum(1))


def test_past_the_grid_cap_index_sum64():
    o = _ops()
    n_src = 300
    src = R.in_slice(_ints(n_src, COLS, seed=13, lo=1), 2, 2)[0]           # no zero: every row that is hit shows it
    idx = torch.randint(0, ROWS, (n_src,), generator=torch.Generator().manual_seed(14))
    idx[0], idx[1], idx[2] = CAP // COLS, ROWS - 1, ROWS - 1               # the rows of flat element 2^21 and of the last one

    def run():
        out, whole = _out_flat((ROWS, COLS))                               # NaN: an element no pass reaches stays NaN
        o.index_sum64(src, _i32(idx), out)
        torch.cuda.synchronize()
        R.assert_guards("index_sum64 out", out, whole)
        return out
    _exact("index_sum64", _twice(run), torch.zeros(ROWS, COLS, dtype=torch.float64, device=DEV).index_add(0, idx.to(DEV), src))


def test_past_the_grid_cap_wgrad64_reduce():
    """N K = 1500 x 1407 > 2^21 with M = 1024: two splits, so the reduction of the partial slabs runs - past its grid cap."""
    o = _ops()
    M, N, K = 1024, 1500, 1407
    assert N * K > CAP and M // o._WGRAD64_ROWS == 2
    dy, x = _ints(M, N, seed=16, lo=-4, hi=5), _ints(M, K, seed=17, lo=-4, hi=5)

    def run():
        dw, whole = _out_flat((N, K))
        o.wgrad64(M, dy, [o.seg64(x)], dw)
        torch.cuda.synchronize()
        R.assert_guards("wgrad64 dw", dw, whole)
        return dw
    _exact("wgrad64", _twice(run), dy.t() @ x)
