"""The query-only form of the fused encoder backward (include/dosx.h: DosxFfnBwd.att_dkvhat == NULL) on a real MI355X: the
launch keeps phases a - e of the attention epilogue and drops the key-gradient share, its ticket and the last arriver's
reduction.  dosx_ffn_bwd is run in the full form and in the query-only form on the same inputs; dh, the layer-input gradient,
every column of the feed-forward partial rows (LayerNorm-1, final LayerNorm / head) and the query-side attention partial rows
must be BITWISE equal.  And the trainer reaches the form exactly where functional.attention_query_only says so."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(51, 3, 3, 5), (51, 4, 2, 17), (20, 2, 2, 64), (51, 6, 3, 16)]          # (Sq, Bq, Bk, Nk)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _layer(H, Sq, Bq, Bk, Nk, ragged, drop, seed):
    """One encoder layer's forward (functional.encoder_fwd, T = 1) -> parameters, its saved tensors, the key operand"""
    from dostransformer_amd import functional as Fn
    gen = torch.Generator().manual_seed(seed)
    P = {}
    lp = "e.layers.0"
    for k, shp, sc in ((".layer_norms.0.weight", (H,), 0.2), (".layer_norms.0.bias", (H,), 0.3), (".layer_norms.1.weight", (H,), 0.2),
                       (".layer_norms.1.bias", (H,), 0.3), (".fc1.weight", (4 * H, H), H ** -0.5), (".fc1.bias", (4 * H,), 0.1),
                       (".fc2.weight", (H, 4 * H), (4 * H) ** -0.5), (".fc2.bias", (H,), 0.1)):
        P[lp + k] = (torch.randn(*shp, generator=gen) * sc + (1.0 if "norms" in k and k.endswith("weight") else 0.0)).to(DEV)
    P["e.layer_norm.weight"], P["e.layer_norm.bias"] = (1 + 0.1 * torch.randn(H, generator=gen)).to(DEV), (0.1 * torch.randn(H, generator=gen)).to(DEV)
    P = Fn.pack_params(P)
    x = torch.randn(Sq * Bq, H, generator=gen).to(DEV)
    kv = torch.randn(Nk * Bk, H, generator=gen)
    kv[::5] = 0.0                                       # padded key slots: exact zero rows
    kvhat = kv.to(DEV)
    key_ptr = None
    if ragged:                                          # per-crystal key counts: all of them, none, about half, ...
        counts = [Nk, 0, max(1, Nk // 2)][:Bk]
        key_ptr = torch.tensor([0] + [sum(counts[:i + 1]) for i in range(Bk)], dtype=torch.int32, device=DEV)
    seed_dev = torch.tensor([4321], dtype=torch.int64, device=DEV)
    y, ctx = Fn.encoder_fwd(P, "e", x, Sq, Bq, Bq, 1, kvhat, Nk, Bk, H, 1, final_ln=False,
                            drop=(0.25, seed_dev, 0) if drop else None, key_ptr=key_ptr)
    torch.cuda.synchronize()
    return P, ctx.layers[0], kvhat, key_ptr, y


def _run(o, P, lay, kvhat, key_ptr, H, Sq, Bq, Bk, Nk, query_only, head, seed):
    """dosx_ffn_bwd with the attention half's backward inside, full form or query-only -> every output the two forms share"""
    lp = "e.layers.0"
    rows = Sq * Bq
    gen = torch.Generator().manual_seed(seed)
    nqt = o.ffn_att_bwd_partial_rows(Sq, Bq) // Bq
    nq = Bq * nqt
    nkv = Bk * ((Nk + 15) // 16)
    nan = float("nan")
    part_a = torch.full((nq + nkv, 2 * H), nan, device=DEV)
    dxin = torch.full((rows, H), nan, device=DEV)
    dh = torch.full((rows, 4 * H), nan, device=DEV)
    dkv = torch.zeros(Nk * Bk, H, device=DEV)
    common = dict(x=lay.x, kvhat=kvhat, gamma0=P[lp + ".layer_norms.0.weight"], beta0=P[lp + ".layer_norms.0.bias"], probs=lay.probs,
                  qstats=lay.qstats, mask=lay.mask, dxin=dxin, partials_q=part_a.data_ptr(), Nk=Nk, Bk=Bk, Bq=Bq, Sq=Sq, qs=lay.qs,
                  qb=lay.qb, key_ptr=key_ptr)
    if query_only:
        att = o.AttBwd(partials_kv=None, dkv_part=None, dkv_cnt=None, dkvhat=None, accumulate=0, **common)
    else:
        kvp = torch.full((nq * Nk, H), nan, device=DEV)
        att = o.AttBwd(partials_kv=part_a.data_ptr() + 4 * nq * 2 * H, dkv_part=kvp, dkv_cnt=o.COUNTERS.take(kvhat.device, Bk),
                       dkvhat=dkv, accumulate=0, **common)
    fin, dy, pld = None, torch.randn(rows, H, generator=gen).to(DEV), 2 * H
    fin_dy = None
    if head:                                            # output layer + final LayerNorm backward in front, in the same launch
        xhat, rstd = torch.randn(rows, H, generator=gen).to(DEV), (0.5 + torch.rand(rows, generator=gen)).to(DEV)
        fin_dy = torch.full((rows, H), nan, device=DEV)
        fin = o.Head(P["e.layer_norm.weight"], P["e.layer_norm.bias"], xhat, rstd, w=torch.randn(H, generator=gen).to(DEV),
                     ddos=torch.randn(Bq, Sq, generator=gen).to(DEV), dy=fin_dy, S=Sq, Bq=Bq)
        dy, pld = None, 5 * H + 4
    part = torch.full((o.ffn_att_bwd_partial_rows(Sq, Bq), pld), nan, device=DEV)
    o.ffn_bwd(rows, H, dy, lay.h, lay.x1, lay.st1, P[lp + ".layer_norms.1.weight"], P[lp + ".fc1.weight"], P[lp + ".fc2.weight"],
              dh, None, part, fin=fin, att=att)
    torch.cuda.synchronize()
    live = 5 * H + 1 if head else 2 * H                 # (the head's partial rows: 5 column groups + the bias column)
    out = {"dh": dh, "dxin": dxin, "partials": part[:, :live], "partials_q": part_a[:nq]}
    if fin_dy is not None:
        out["fin_dy"] = fin_dy
    return out, part_a[nq:], dkv


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("Sq,Bq,Bk,Nk", SHAPES)
@pytest.mark.parametrize("H", [64, 128])
def test_query_only_ffn_bwd_is_bitwise_the_full_form(H, Sq, Bq, Bk, Nk, ragged, drop):
    from dostransformer_amd import ops as o
    assert o.ffn_att_bwd_supported(H, Nk, Sq, Bq)
    P, lay, kvhat, key_ptr, _ = _layer(H, Sq, Bq, Bk, Nk, ragged, drop, seed=Sq * 7 + Nk + H)
    assert (lay.mask is not None) == drop
    full, kv_rows, dkv = _run(o, P, lay, kvhat, key_ptr, H, Sq, Bq, Bk, Nk, False, False, seed=5)
    qo, kv_rows_q, dkv_q = _run(o, P, lay, kvhat, key_ptr, H, Sq, Bq, Bk, Nk, True, False, seed=5)
    for name in full:
        assert not bool(torch.isnan(full[name]).any()), name                     # (every element was written)
        assert torch.equal(_bits(full[name]), _bits(qo[name])), name
    # the full form made a key gradient and its key-side partial rows; the query-only form touched neither
    assert bool(dkv.abs().sum() > 0) and not bool(torch.isnan(kv_rows).any())
    assert not bool(dkv_q.any()) and bool(torch.isnan(kv_rows_q).all())


def test_query_only_ffn_bwd_with_the_fused_head():
    from dostransformer_amd import functional as Fn, ops as o
    H, (Sq, Bq, Bk, Nk) = 128, SHAPES[1]
    assert o.ffn_att_bwd_supported(H, Nk, Sq, Bq) and Fn.head_fused_bwd(H, 1)
    P, lay, kvhat, key_ptr, _ = _layer(H, Sq, Bq, Bk, Nk, True, True, seed=99)
    full, _, _ = _run(o, P, lay, kvhat, key_ptr, H, Sq, Bq, Bk, Nk, False, True, seed=6)
    qo, _, _ = _run(o, P, lay, kvhat, key_ptr, H, Sq, Bq, Bk, Nk, True, True, seed=6)
    assert set(full) == {"dh", "dxin", "partials", "partials_q", "fin_dy"}
    for name in full:
        assert not bool(torch.isnan(full[name]).any()), name
        assert torch.equal(_bits(full[name]), _bits(qo[name])), name


def test_query_only_needs_no_key_side_operands_but_the_full_form_does():
    from dostransformer_amd import ops as o
    from dostransformer_amd._lib import DosxError
    H, (Sq, Bq, Bk, Nk) = 64, SHAPES[0]
    P, lay, kvhat, key_ptr, _ = _layer(H, Sq, Bq, Bk, Nk, False, False, seed=3)
    lp = "e.layers.0"
    rows = Sq * Bq
    nq = o.ffn_att_bwd_partial_rows(Sq, Bq)
    part_a, dxin, dh = torch.zeros(nq, 2 * H, device=DEV), torch.zeros(rows, H, device=DEV), torch.zeros(rows, 4 * H, device=DEV)
    att = o.AttBwd(x=lay.x, kvhat=kvhat, gamma0=P[lp + ".layer_norms.0.weight"], beta0=P[lp + ".layer_norms.0.bias"], probs=lay.probs,
                   qstats=lay.qstats, dxin=dxin, partials_q=part_a.data_ptr(), partials_kv=None, dkv_part=None, dkv_cnt=None,
                   dkvhat=torch.zeros(Nk * Bk, H, device=DEV), accumulate=0, Nk=Nk, Bk=Bk, Bq=Bq, Sq=Sq, qs=lay.qs, qb=lay.qb)
    with pytest.raises((DosxError, AttributeError)):    # a key gradient without its scratch / counters / partial rows: refused
        o.ffn_bwd(rows, H, torch.zeros(rows, H, device=DEV), lay.h, lay.x1, lay.st1, P[lp + ".layer_norms.1.weight"],
                  P[lp + ".fc1.weight"], P[lp + ".fc2.weight"], dh, None, torch.zeros(nq, 2 * H, device=DEV), att=att)


def test_policy_and_the_trainer_reach_the_form_where_they_should(monkeypatch):
    """functional.attention_query_only: both conditions are needed (frozen trunk AND the layer's frozen layer_norms.0), never for
    transformer_self; and Trainer runs exactly those layers' ffn_bwd launches without a key gradient."""
    from dostransformer_amd import functional as Fn, ops as o, synth
    from dostransformer_amd.embedder_phDOS.DOSTransformer_phonon import DOSTransformer_phonon
    from dostransformer_amd.train import Trainer
    torch.manual_seed(0)
    mk = lambda: DOSTransformer_phonon(2, 2, 118, 4, 64, DEV, 0.0).to(DEV)
    g = synth.phonon_batch(4, seed=21, dtype=torch.float32).to(DEV)
    calls = []
    real = o.ffn_bwd

    def spy(*a, **k):
        calls.append(k["att"] is not None and k["att"].dkvhat is None)
        return real(*a, **k)
    monkeypatch.setattr(o, "ffn_bwd", spy)
    trunk = ("GN_encoder", "stacked_processor", "GN_decoder")
    want = {}
    # B: only the prompt path trains - the source encoder's two layers qualify (the first encoder's backward is cut altogether)
    want["B"] = (mk().train_only("prompt_token", "fc_prompt"), [True, True, False, False])
    # A: a frozen trunk under trainable layer_norms.0 - their gradient needs the key-side partial rows: the full form everywhere
    want["A"] = (mk().freeze(*trunk), [False] * 6)
    # frozen layer_norms.0 over a trainable trunk: the key gradient is wanted
    want["ln"] = (mk().freeze("transformer_source.layers.0.layer_norms.0", "transformer_source.layers.1.layer_norms.0"), [False] * 6)
    # frozen trunk + ONE frozen layer_norms.0: that layer alone (the backward runs the layers last to first)
    want["one"] = (mk().freeze(*trunk, "transformer_source.layers.0.layer_norms.0"), [False, True, False, False, False, False])
    for name, (model, expect) in want.items():
        G = model.flat_params().G
        assert Fn.attention_bwd_in_ffn(51, 4, g.meta.n_max, 64, False) and Fn.attention_bwd_in_ffn(51, 8, g.meta.n_max, 64, False)
        for pre in ("transformer", "transformer_self", "transformer_source"):
            for t in range(2):
                ln = f"{pre}.layers.{t}.layer_norms.0."
                should = pre != "transformer_self" and G.cut_trunk and ln + "weight" in G.frozen and ln + "bias" in G.frozen
                assert Fn.attention_query_only(G.keys(), G.frozen, pre, t) == should, (name, pre, t)
        del calls[:]
        Trainer(model, lr=1e-3).step(g)
        assert calls == expect, (name, calls)


# ---- dosx_attention_bwd: DOSX_ATTN_BWD_DQ_HALF with dkvhat == NULL is a complete call ---------------------------------------------
def _attn_case(Sq, Bq, Bk, Nk, H, drop):
    """forward through dosx_attention_fwd -> (descriptor factory, float64 reference gradient of the queries, the tensors kept alive)"""
    from dostransformer_amd import ops as o
    from dostransformer_amd._lib import Attn
    from tests.gpu_util import _attn_ref, rnd
    x = rnd(Sq * Bq, H, seed=1).double().requires_grad_(True)
    kv = rnd(Nk * Bk, H, seed=2)
    kv[-Bk:] = 0
    kv = kv.double().requires_grad_(True)
    gam = rnd(H, seed=3).double().requires_grad_(True)
    bet = (0.3 * rnd(H, seed=4)).double().requires_grad_(True)
    mask = None
    if drop > 0:
        mask = (torch.rand(Bq, Sq, Nk, generator=torch.Generator().manual_seed(9)) >= drop).float().to(DEV) / (1 - drop)
    ref, _ = _attn_ref(x, kv, gam, bet, Sq, Bq, Nk, Bk, H, Bq, 1, None if mask is None else mask.double())
    dout = rnd(Sq * Bq, H, seed=5)
    ref.backward(dout.double())
    f = lambda t: t.detach().float().contiguous()
    keep = dict(x=f(x), kv=f(kv), g=f(gam), b=f(bet), out=torch.empty(Sq * Bq, H, device=DEV), probs=torch.empty(Bq, Sq, Nk, device=DEV),
                qstats=torch.empty(Sq * Bq, 2, device=DEV), dout=dout, mask=mask)

    def desc():
        a = Attn()
        a.Sq, a.Bq, a.Nk, a.Bk, a.H, a.q_stride_s, a.q_stride_b = Sq, Bq, Nk, Bk, H, Bq, 1
        a.x, a.kvhat, a.gamma0, a.beta0 = keep["x"].data_ptr(), keep["kv"].data_ptr(), keep["g"].data_ptr(), keep["b"].data_ptr()
        a.out, a.probs, a.qstats = keep["out"].data_ptr(), keep["probs"].data_ptr(), keep["qstats"].data_ptr()
        a.drop_mask = mask.data_ptr() if mask is not None else None
        return a
    o.attention_fwd(desc())
    torch.cuda.synchronize()
    return desc, x.grad, keep


@pytest.mark.parametrize("drop", [0.0, 0.3])
@pytest.mark.parametrize("Sq,Bq,Bk,Nk,H,route", [(201, 4, 2, 41, 256, "aligned"), (51, 4, 2, 70, 64, "streamed"), (8, 4, 2, 330, 64, "general")])
def test_query_only_attention_bwd_is_bitwise_the_full_backward(Sq, Bq, Bk, Nk, H, route, drop):
    """dx and partials_q of the query-only call against the full backward of the same route: the one-launch form where <= 64 keys
    route to the crystal-aligned kernel, the DQ + DKV halves on the streamed (<= 320 keys) and the general route."""
    from dostransformer_amd import ops as o
    desc, xgrad, keep = _attn_case(Sq, Bq, Bk, Nk, H, drop)
    nqt = (Sq + 31) // 32
    nan = float("nan")
    res = {}
    for form in ("full", "query_only"):
        dx = torch.full((Sq * Bq, H), nan, device=DEV)
        nkt = (Nk + 15) // 16 if route == "aligned" else (Nk + 31) // 32
        part = torch.full((Bq * nqt + Bk * nkt, 2 * H), nan, device=DEV)
        dkv = torch.zeros(Nk * Bk, H, device=DEV)
        dsc = torch.full((Bq, Sq, Nk), nan, device=DEV)
        a = desc()
        a.dout, a.dx, a.partials_q = keep["dout"].data_ptr(), dx.data_ptr(), part.data_ptr()
        if form == "query_only":
            a.flags = o.ATTN_BWD_DQ_HALF                         # dkvhat / partials_kv / dkv_part / dkv_cnt stay NULL
            if route != "aligned":
                a.dscores = dsc.data_ptr()                       # (the streamed / general dq kernels' scratch)
            o.attention_bwd(a)
        else:
            a.dkvhat, a.dkv_accumulate, a.partials_kv = dkv.data_ptr(), 0, part.data_ptr() + 4 * Bq * nqt * 2 * H
            if route == "aligned":
                kvp = torch.empty(Bq * nqt * Nk, H, device=DEV)
                a.dkv_part, a.dkv_cnt = kvp.data_ptr(), o.COUNTERS.take(keep["x"].device, Bk)
                o.attention_bwd(a)
            else:
                a.dscores = dsc.data_ptr()
                a.flags = o.ATTN_BWD_DQ_HALF
                o.attention_bwd(a)
                a.flags = o.ATTN_BWD_DKV_HALF
                o.attention_bwd(a)
        torch.cuda.synchronize()
        res[form] = (dx, part[:Bq * nqt], part[Bq * nqt:], dkv)
    (dx0, pq0, pkv0, dkv0), (dx1, pq1, pkv1, dkv1) = res["full"], res["query_only"]
    assert not bool(torch.isnan(dx0).any()) and not bool(torch.isnan(pq0).any())
    print(f"query-only attention_bwd {route} drop {drop}: dx differs in {int((_bits(dx0) != _bits(dx1)).sum())} of {dx0.numel()} elements "
          f"(max {float((dx0 - dx1).abs().max()):.3e}), partials_q in {int((_bits(pq0) != _bits(pq1)).sum())} of {pq0.numel()} "
          f"(max {float((pq0 - pq1).abs().max()):.3e})")
    assert torch.equal(_bits(dx0), _bits(dx1)) and torch.equal(_bits(pq0), _bits(pq1))
    assert bool(dkv0.abs().sum() > 0) and not bool(torch.isnan(pkv0).any())
    assert not bool(dkv1.any()) and bool(torch.isnan(pkv1).all())             # no key gradient, no key-side partial rows
    if route == "aligned":
        # ... and against the float64 torch reference of tests/test_gpu_attention.py, at that file's bar
        from tests.gpu_util import err
        assert err(dx1, xgrad) < 5e-5


def test_query_only_attention_bwd_refuses_what_it_cannot_be():
    from dostransformer_amd import ops as o
    from dostransformer_amd._lib import DosxError
    desc, _, keep = _attn_case(51, 4, 2, 70, 64, 0.0)
    dx, part = torch.zeros(51 * 4, 64, device=DEV), torch.zeros(4 * 2, 128, device=DEV)
    a = desc()
    a.dout, a.dx, a.partials_q, a.flags = keep["dout"].data_ptr(), dx.data_ptr(), part.data_ptr(), o.ATTN_BWD_DQ_HALF
    with pytest.raises(DosxError, match="dscores"):              # 70 keys: the streamed dq kernel needs its scratch
        o.attention_bwd(a)
    a.flags = 0                                                  # the whole backward without a key gradient: still refused
    with pytest.raises(DosxError, match="null operand"):
        o.attention_bwd(a)
