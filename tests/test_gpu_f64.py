"""float64 program on a real MI355X (csrc/f64.hip, dostransformer_amd/functional64.py): the kernels against float64 torch,
and Graphnetwork_phonon in float64 against the reference's fixture and the float64 oracle.  The edges of the elementwise, row
and graph kernels (tails, strides, absent operands, the grid cap) against long double: tests/test_gpu_f64_kernels.py."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.util import batch_from, load, rmse, sub

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ops():
    from dostransformer_amd import ops
    return ops


def _r(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).to(DEV)


def _bound_ok(c, ref, a_abs_w_abs, k=1e-13):
    return bool(((c - ref).abs() <= k * a_abs_w_abs + 1e-300).all())


def test_gemm_f64_fragment_map_exact_integers():
    """Small integers: every product and sum is exact, so any misplaced row / column of the f64 C/D map shows up."""
    ops = _ops()
    g = torch.Generator().manual_seed(3)
    for M, N, K in [(16, 16, 4), (37, 70, 9), (64, 64, 64)]:
        a = torch.randint(-8, 9, (M, K), generator=g).double().to(DEV)
        w = torch.randint(-8, 9, (N, K), generator=g).double().to(DEV)
        out = ops.gemm64(M, N, [ops.seg64(a)], w, torch.empty(M, N, dtype=torch.float64, device=DEV))
        assert torch.equal(out, a @ w.t()), (M, N, K)


@pytest.mark.parametrize("M", [1, 17, 1000])
@pytest.mark.parametrize("K", [4, 118, 384])
@pytest.mark.parametrize("N", [16, 136, 1024])
def test_gemm_f64_layouts_and_epilogues(M, N, K):
    ops = _ops()
    a, w, b, r = _r(M, K, seed=1), _r(N, K, seed=2), _r(N, seed=3), _r(M, N, seed=4)
    scale = a.abs() @ w.abs().t()
    out = lambda: torch.empty(M, N, dtype=torch.float64, device=DEV)
    ref = a @ w.t() + b
    c = ops.gemm64(M, N, [ops.seg64(a)], w, out(), bias=b)
    assert _bound_ok(c, ref, scale + b.abs())
    c = ops.gemm64(M, N, [ops.seg64(a)], w.t().contiguous(), out(), w_layout=1, bias=b)
    assert _bound_ok(c, ref, scale + b.abs())
    alpha = torch.tensor([0.3], dtype=torch.float64, device=DEV)
    for act, f in [(ops.ACT64_RELU, F.relu), (ops.ACT64_LEAKY, lambda t: F.leaky_relu(t, 0.01)),
                   (ops.ACT64_PRELU, lambda t: torch.where(t >= 0, t, 0.3 * t))]:
        pre = out()
        c = ops.gemm64(M, N, [ops.seg64(a)], w, out(), bias=b, act=act, alpha=alpha, pre=pre, res=r)
        assert _bound_ok(pre, ref, scale + b.abs())
        assert _bound_ok(c, f(ref) + r, scale + b.abs() + r.abs())


def test_gemm_f64_gathered_segments():
    """cat[x[src], x[dst], e] of an EdgeModel with a K tail in every segment, and the [S,B] broadcast row maps of the head."""
    ops = _ops()
    N, E, H = 23, 300, 37
    g = torch.Generator().manual_seed(5)
    x, e = _r(N, H, seed=6), _r(E, H, seed=7)
    src = torch.randint(0, N, (E,), generator=g).to(torch.int32).to(DEV)
    dst = torch.randint(0, N, (E,), generator=g).to(torch.int32).to(DEV)
    w, b = _r(2 * H + 3, 3 * H, seed=8), _r(2 * H + 3, seed=9)
    segs = [ops.seg64(x, ops.rowmap(idx=src)), ops.seg64(x, ops.rowmap(idx=dst)), ops.seg64(e)]
    c = ops.gemm64(E, 2 * H + 3, segs, w, torch.empty(E, 2 * H + 3, dtype=torch.float64, device=DEV), bias=b)
    A = torch.cat([x[src.long()], x[dst.long()], e], 1)
    assert _bound_ok(c, A @ w.t() + b, A.abs() @ w.abs().t() + b.abs())
    S, B = 51, 6
    emb, graph, w2 = _r(S, H, seed=10), _r(B, H, seed=11), _r(H, 2 * H, seed=12)
    c = ops.gemm64(S * B, H, [ops.seg64(emb, ops.rowmap(d=B, m=1, c=0)), ops.seg64(graph, ops.rowmap(d=B, m=0, c=1))], w2,
                   torch.empty(S * B, H, dtype=torch.float64, device=DEV))
    A = torch.cat([emb[:, None, :].expand(S, B, H), graph[None].expand(S, B, H)], 2).reshape(S * B, 2 * H)
    assert _bound_ok(c, A @ w2.t(), A.abs() @ w2.abs().t())


def test_gemm_f64_strided_operands():
    """out, res and the segments as column slices of wider buffers (ldo != N, ldr != ldo, ld != width); pre shares ldo."""
    ops = _ops()
    M, N, K = 133, 40, 21
    a_buf, w, r_buf = _r(M, K + 9, seed=1), _r(N, K, seed=2), _r(M, N + 13, seed=3)
    a, r = a_buf[:, 5:5 + K], r_buf[:, 7:7 + N]
    out_buf = torch.full((M, N + 30), 7.0, dtype=torch.float64, device=DEV)
    pre_buf = torch.full((M, N + 30), 7.0, dtype=torch.float64, device=DEV)
    out, pre = out_buf[:, 3:3 + N], pre_buf[:, 3:3 + N]
    ops.gemm64(M, N, [ops.seg64(a)], w, out, act=ops.ACT64_RELU, pre=pre, res=r)
    ref = a @ w.t()
    scale = a.abs() @ w.abs().t()
    assert _bound_ok(pre, ref, scale) and _bound_ok(out, F.relu(ref) + r, scale + r.abs())
    keep = torch.ones_like(out_buf, dtype=torch.bool)
    keep[:, 3:3 + N] = False
    assert bool((out_buf[keep] == 7.0).all()) and bool((pre_buf[keep] == 7.0).all())     # nothing written outside


@pytest.mark.parametrize("M", [3, 700, 5000])
def test_wgrad_f64(M):
    ops = _ops()
    N, H = 70, 29
    g = torch.Generator().manual_seed(M)
    dy, x, e = _r(M, N, seed=1), _r(40, H, seed=2), _r(M, 5, seed=3)
    idx = torch.randint(0, 40, (M,), generator=g).to(torch.int32).to(DEV)
    segs = [ops.seg64(x, ops.rowmap(idx=idx)), ops.seg64(e)]
    X = torch.cat([x[idx.long()], e], 1)
    dw = torch.empty(N, H + 5, dtype=torch.float64, device=DEV)
    ops.wgrad64(M, dy, segs, dw)
    assert _bound_ok(dw, dy.t() @ X, dy.abs().t() @ X.abs())
    dw2 = torch.empty_like(dw)
    ops.wgrad64(M, dy, segs, dw2)
    assert torch.equal(dw, dw2)
    db = torch.empty(N, dtype=torch.float64, device=DEV)
    ops.colsum64(dy, db)
    assert _bound_ok(db, dy.sum(0), dy.abs().sum(0))
    # accumulate: dw += dy^T X, db += colsum (the split-M reduction and the direct store both)
    base_w, base_b = _r(N, H + 5, seed=9), _r(N, seed=10)
    dw3, db3 = base_w.clone(), base_b.clone()
    ops.wgrad64(M, dy, segs, dw3, accumulate=True)
    ops.colsum64(dy, db3, accumulate=True)
    assert _bound_ok(dw3, base_w + dy.t() @ X, base_w.abs() + dy.abs().t() @ X.abs())
    assert _bound_ok(db3, base_b + dy.sum(0), base_b.abs() + dy.abs().sum(0))


def _rel(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


@pytest.mark.parametrize("W", [8, 64, 256, 1024])
def test_layernorm_prelu_f64(W):
    ops = _ops()
    M = 77
    z, gam, bet, dout = _r(M, W, seed=1, scale=3.0) + 0.5, _r(W, seed=2), _r(W, seed=3), _r(M, W, seed=4)
    alpha = torch.tensor([0.25], dtype=torch.float64, device=DEV)
    zc, gc, bc, ac = (t.detach().clone().requires_grad_(True) for t in (z, gam, bet, alpha))
    y = F.layer_norm(zc, (W,), gc, bc, 1e-5)
    ref = torch.where(y >= 0, y, ac * y)
    ref.backward(dout)
    xhat, rstd, out = ops.layernorm64(z, gam, bet, alpha)
    assert _rel(out, ref.detach()) < 1e-14
    dz, part = ops.layernorm_bwd64(dout, xhat, rstd, gam, bet, alpha)
    assert _rel(dz, zc.grad) < 1e-13
    sums = torch.empty(2 * W + 1, dtype=torch.float64, device=DEV)
    ops.colsum64(part, sums)
    assert _rel(sums[:W], gc.grad) < 1e-13 and _rel(sums[W:2 * W], bc.grad) < 1e-13 and _rel(sums[2 * W:], ac.grad) < 1e-13


def test_act_bwd_f64():
    ops = _ops()
    M, W = 300, 45
    z, dy = _r(M, W, seed=1), _r(M, W, seed=2)
    alpha = torch.tensor([0.2], dtype=torch.float64, device=DEV)
    dz, _ = ops.act_bwd64(dy, z, ops.ACT64_RELU)
    assert torch.equal(dz, dy * (z > 0))
    dz, _ = ops.act_bwd64(dy, z, ops.ACT64_LEAKY)
    assert torch.equal(dz, torch.where(z > 0, dy, dy * 0.01))
    dz, part = ops.act_bwd64(dy, z, ops.ACT64_PRELU, alpha)
    assert torch.equal(dz, torch.where(z >= 0, dy, dy * 0.2))
    assert _rel(part[:, 0], (dy * z * (z < 0)).sum(1)) < 1e-14


def _graph_case():
    """3 crystals: a 1-atom crystal (self edge only), one with an isolated node and duplicate edges, one ordinary."""
    from dostransformer_amd.batch import collate
    g = torch.Generator().manual_seed(1)
    cs = []
    for n, ei in [(1, [[0], [0]]), (4, [[0, 0, 0, 1, 2], [1, 1, 1, 0, 2]]), (5, [[i % 5 for i in range(17)], [(3 * i + 1) % 5 for i in range(17)]])]:
        ei = torch.tensor(ei)
        cs.append({"x": torch.rand(n, 118, generator=g, dtype=torch.float64), "edge_index": ei,
                   "edge_vec": (torch.rand(ei.shape[1], 3, generator=g, dtype=torch.float64) * 2 - 1) * 3.0,
                   "system": torch.tensor(1), "phdos": torch.rand(1, 51, generator=g, dtype=torch.float64)})
    cs[0]["edge_vec"][0] = 0.0
    return collate(cs)


def test_graph_kernels_f64():
    from oracle import dos_oracle as O
    from dostransformer_amd.batch import graph_meta
    ops = _ops()
    gb = _graph_case()
    m = graph_meta(gb, DEV)
    N, E, B, H = m.num_nodes, m.num_edges, m.num_graphs, 12
    src, dst = m.src.long(), m.dst.long()
    vec = gb.edge_vec.to(DEV)
    if m.edge_perm is not None:
        vec = vec[m.edge_perm]
    vec = vec.contiguous()
    ef = ops.edge_feat_sh1_64(vec, 4.0)
    ref = O.edge_features_sh1(vec.cpu()).to(DEV)
    assert float((ef - ref).abs().max()) <= 1e-14 * float(ref.abs().max())
    msg = _r(E, H, seed=3)
    agg = ops.segment_mean64(msg, m.rowptr_dst, N)
    assert _rel(agg, O.scatter_mean(msg.cpu(), dst.cpu(), N).to(DEV)) < 1e-14
    dagg, de = _r(N, 2 * H, seed=4), _r(E, H, seed=5)
    cnt = torch.bincount(dst, minlength=N).clamp(min=1).double()
    out = ops.segment_mean_bwd64(dagg[:, H:], m.dst, m.rowptr_dst, de, E)
    assert _rel(out, de + (dagg[:, H:] / cnt[:, None])[dst]) < 1e-14
    dcat, b0 = _r(E, 3 * H, seed=6), _r(N, H, seed=7)
    dx = ops.gather_bwd64(dcat, m, b0, dagg[:, :H], N, H)
    ref = b0 + dagg[:, :H] + torch.zeros(N, H, dtype=torch.float64, device=DEV).index_add(0, src, dcat[:, :H]).index_add(
        0, dst, dcat[:, H:2 * H])
    assert _rel(dx, ref) < 1e-14
    x = _r(N, H, seed=8)
    pool = ops.graph_pool64(x, m.graph_ptr, B)
    assert _rel(pool, O.scatter_sum(x.cpu(), gb.batch, B).to(DEV)) < 1e-14
    back = ops.rows_add64(N, pool, ia=m.node_graph)
    assert torch.equal(back, pool[gb.batch.to(DEV)])
    S = 51
    t = _r(S * B, H, seed=9)
    assert _rel(ops.reduce_rows64(t, S, B, B, 1), t.view(S, B, H).sum(1)) < 1e-14
    assert _rel(ops.reduce_rows64(t, B, S, 1, B), t.view(S, B, H).sum(0)) < 1e-14


# ---- Graphnetwork_phonon in float64 --------------------------------------------------------------------------------------
def _model64(H, L, seed=0):
    from dostransformer_amd.embedder_phDOS.graphnetwork_phonon import Graphnetwork_phonon
    torch.manual_seed(seed)
    model = Graphnetwork_phonon(L, 118, 4, H, 51, DEV).double()
    p = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return model.to(DEV), p


def _oracle(p, g, L, w):
    from oracle import dos_oracle as O
    pr = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in p.items()}
    dos = O.graphnetwork_phonon_forward(pr, g, L)
    (dos * w).sum().backward()
    return dos.detach(), {k: v.grad for k, v in pr.items()}


def _check_grads(model, ref_grads, dead, tol):
    worst = 0.0
    for k, prm in model.named_parameters():
        if k in dead:
            assert prm.grad is None, k
            continue
        assert prm.grad is not None and prm.grad.dtype == torch.float64, k
        r = ref_grads[k]
        e = float((prm.grad.cpu() - r).abs().max() / (r.abs().max() + 1e-300))
        worst = max(worst, e)
        assert e <= tol, (k, e)
    return worst


def test_graphnetwork_phonon_f64_golden():
    """Against the reference's own float64 numbers (tests/golden/g8_graphnetwork_phonon.npz)."""
    from dostransformer_amd.embedder_phDOS.graphnetwork_phonon import Graphnetwork_phonon
    z = load("g8_graphnetwork_phonon.npz")
    model = Graphnetwork_phonon(3, 118, 4, 16, 51, DEV).double()
    model.load_state_dict(sub(z, "p0/"))
    model = model.to(DEV)
    dos = model(batch_from(z).to(DEV))
    assert dos.dtype == torch.float64
    assert rmse(dos.detach().cpu(), z["dos"]) <= 1e-12
    (dos * torch.from_numpy(z["w"]).to(DEV)).sum().backward()
    dead = set(str(s) for s in z["dead_params"])
    refs = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("g/")}
    _check_grads(model, refs, dead, 1e-10)
    assert all(v.dtype == torch.float64 for v in model.state_dict().values() if v.is_floating_point())


@pytest.mark.parametrize("H,prompt", [(64, False), (128, False), (64, True)])
def test_graphnetwork_phonon_f64_oracle_live(H, prompt):
    from dostransformer_amd import synth
    L, B = 3, 8
    model, p = _model64(H, L)
    g = synth.phonon_batch(B, seed=17, dtype=torch.float64)
    if prompt:                  # 118 + H/2 wide nodes take node_encoder_prompt (graphnetwork_phonon.py:150-153)
        g.x = torch.cat([g.x, torch.randn(g.x.shape[0], H // 2, generator=torch.Generator().manual_seed(2), dtype=torch.float64)], 1)
    w = torch.randn(B, 51, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    ref, rg = _oracle(p, g, L, w)
    dos = model(g.clone().to(DEV))
    assert dos.dtype == torch.float64
    assert rmse(dos.detach().cpu(), ref) <= 1e-12
    (dos * w.to(DEV)).sum().backward()
    unused = "GN_encoder.node_encoder" if prompt else "GN_encoder.node_encoder_prompt"
    dead = {k for k in p if k.startswith(unused + ".") or ".node_mlp_1." in k}
    worst = _check_grads(model, rg, dead, 1e-10)
    print(f"H={H} prompt={prompt}: worst per-tensor gradient error {worst:.2e}")
    # two runs bitwise equal; an fp32 batch is promoted once and gives the same numbers
    model.zero_grad(set_to_none=True)
    dos2 = model(g.clone().to(DEV, dtype=torch.float32).to(DEV))
    g32 = g.clone().to(DEV, dtype=torch.float32)
    g64 = g.clone()
    g64.x, g64.edge_vec = g32.x.cpu().double(), g32.edge_vec.cpu().double()
    assert torch.equal(dos2, model(g64.to(DEV)))
    assert torch.equal(model(g.clone().to(DEV)), dos)


def test_graphnetwork_phonon_f64_reference_loop():
    """The reference's loop in float64: default dtype float64, module on the GPU, loss.backward(), torch.optim.AdamW,
    3 steps - against the oracle's autograd + adamw_step."""
    from oracle import dos_oracle as O
    from dostransformer_amd import synth
    from dostransformer_amd.embedder_phDOS.graphnetwork_phonon import Graphnetwork_phonon
    L, H, B = 3, 64, 8
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        torch.manual_seed(0)
        model = Graphnetwork_phonon(L, 118, 4, H, 51, DEV)
        params = {k: v.detach().clone() for k, v in model.state_dict().items()}
        model = model.to(DEV)
        opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-2)
        g = synth.phonon_batch(B, seed=5)
        gd = g.clone().to(DEV)
        state = {}
        for step in range(3):
            opt.zero_grad()
            loss = torch.sqrt(F.mse_loss(model(gd), gd.phdos))
            loss.backward()
            opt.step()
            leaves = {k: v.clone().requires_grad_(True) for k, v in params.items()}
            rl = torch.sqrt(F.mse_loss(O.graphnetwork_phonon_forward(leaves, g, L), g.phdos))
            names = list(leaves)
            gr = torch.autograd.grad(rl, [leaves[k] for k in names], allow_unused=True)
            grads = dict(zip(names, gr))
            lv, rv = float(loss.detach()), float(rl.detach())
            assert abs(lv - rv) <= 1e-10, (step, lv, rv)
            O.adamw_step(params, grads, state, 1e-3)
            sd = model.state_dict()
            for k, v in params.items():
                d = (sd[k].cpu() - v).abs()
                gk = grads[k]
                if gk is not None:          # AdamW's 1/sqrt(v) turns a noise-floor gradient into a full lr step
                    exempt = gk.abs() < 1e-12 * gk.abs().max()
                    for i in (exempt & (d > 1e-9)).nonzero().tolist():
                        print("exempt", step, k, i, float(d[tuple(i)]))
                    d = torch.where(exempt, torch.zeros_like(d), d)
                assert float(d.max()) <= 1e-9, (step, k, float(d.max()))
    finally:
        torch.set_default_dtype(old)


def test_f64_error_paths_and_unchanged_modules():
    """Mixed live dtypes raise.  Modules without a float64 program compute exactly as before: a float64 DOSTransformer_phonon
    and a float64 eDOS DOSTransformer return, bitwise, what an fp32 module with the same weights returns."""
    from dostransformer_amd import synth
    from dostransformer_amd._lib import DosxError
    from dostransformer_amd.embedder_eDOS.DOSTransformer import DOSTransformer
    from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
    g = synth.phonon_batch(3, seed=1).to(DEV)
    model, _ = _model64(16, 2)
    model.out_layer[0].float()
    with pytest.raises(DosxError, match="mix"):
        model(g)
    for make, batch in [(lambda: DOSTransformer_phonon(2, 1, 118, 4, 16, DEV, 0.0), lambda: synth.phonon_batch(3, seed=1)),
                        (lambda: DOSTransformer(2, 1, 200, 41, 2, 16, DEV, 0.0), lambda: synth.edos_batch(3, seed=2))]:
        torch.manual_seed(0)
        m64 = make().double()
        m32 = make()
        m32.load_state_dict({k: v.float() for k, v in m64.state_dict().items()})
        b = batch()
        with torch.no_grad():
            a64 = m64.to(DEV)(b.clone().to(DEV))
            a32 = m32.to(DEV)(b.clone().to(DEV))
        for x, y in zip(a64, a32):
            assert torch.equal(x.float(), y.float())
