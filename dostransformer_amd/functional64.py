"""float64 forward / backward programs of ``Graphnetwork_phonon`` (`embedder_phDOS/graphnetwork_phonon.py:48-72`) and
``DOSTransformer_phonon`` (`embedder_phDOS/DOSTransformer_phonon.py:66-119`).

The phonon reference computes in float64 (main_phDOS.py:15-16).  A module whose live parameters are float64 runs this
program instead of the fp32 one in ``functional.py``: the same steps as ``oracle.graphnetwork_phonon_forward`` in order,
each a libdosx fp64 kernel (csrc/f64.hip), with the backward written out step by step in reverse.  Straight-line on the
current stream, no fused-path heuristics; every reduction has a fixed order, so two runs are bitwise equal.

Edges are processed in the destination-sorted order of ``GraphMeta`` (``edge_perm`` maps the caller's order to it).  The
transformer half of DOSTransformer_phonon keeps crystal-major rows: b * S + s for the energy rows, b * nmax + j for the
zero-padded dense key rows.

train64.Trainer64 records this program (ops.RECORDER) and replays it on static buffers: every buffer the program creates goes
through ops.alloc64 / ops.keep_alive, and the torch casts in its body (``_f64``, ``g.system.to(int32)``, ``ddos.to(float64)``)
hand back their argument when it already has the dtype and layout the kernels read - which the slot buffers have.

The DOSTransformer_phonon program and the FACTORED Graphnetwork_phonon program (``factored_head=True``) are padding-safe: they
run on a ghost-padded batch (``batch.pad_batch``, or a bucket filled by ``DeviceDataset.collate_into``).  Forward, no kernel
reduces across rows other than over a node's own edges (CSR row pointers) or a crystal's own atoms (``graph_ptr``), so the real
rows are bitwise those of the unpadded batch; backward, the sum pool's gradient reads a spare zero row B for the ghost nodes
(``_dpool_rows``) and every gradient that reaches a ghost row is an exact zero, so the parameter gradients differ from the
unpadded ones only by how the row sums of ``wgrad64`` / ``colsum64`` are grouped.  (Graphnetwork_phonon's default, unfactored
program is not: its sum-pool backward still indexes [B, H] rows.)

Graphnetwork_phonon has two programs.  The default one is what ``model(batch)`` runs: the head's first Linear as one product
over the S * B rows cat[emb[s] | graph[b]], with a torch transpose at either end - it is the autograd path and not recordable.
``factored_head=True`` (train64.GraphnetworkTrainer64, predict.Predictor64) runs the head on its rank structure, as
``functional.graphnetwork_fwd(factored_head=True)`` does in fp32: E1 = emb . W0[:, :H]^T + b0 and C = graph . W0[:, H:]^T, then
one float64 launch each way (csrc/pair_head_f64.hip) that reads and writes dos / ddos as [B, S].  It holds no tensor of S * B
rows and no torch kernel, so it is recorded and replayed like the DOSTransformer_phonon program.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional

import torch

from ._lib import DosxError
from .batch import GraphMeta
from . import functional as Fn
from . import ops
from .ops import (ACT64_LEAKY, ACT64_PRELU, ACT64_RELU, act_bwd64, alloc64, attention64, attention_bwd64, colsum64,
                  dense_rows64, dense_rows_bwd64, edge_feat_sh1_64, gather_bwd64, gemm64, graph_pool64, index_sum64,
                  layernorm64, layernorm_bwd64, pair_head_bwd64, pair_head_fwd64, pair_head_partial_rows, reduce_rows64, rows_add64,
                  rowmap, seg64, segment_mean64, segment_mean_bwd64, wgrad64)

Params = Dict[str, torch.Tensor]

MAX_HIDDEN = 512          # the LayerNorm rows of the edge / node MLPs are 2H wide, dosx_layernorm_f64 takes up to 1024
SOFTMAX64 = False         # tests only: the attention softmax in fp64 instead of the reference's fp32 (DOSX_ATTN64_SOFTMAX_F64)


def _f64(t: torch.Tensor) -> torch.Tensor:
    """A batch field as the program reads it: float64, contiguous (an fp32 batch is promoted here, once)."""
    return t.to(torch.float64).contiguous()


def require_replayable(g, fields, device, who: str) -> None:
    """A recorded program replays libdosx calls only: the torch casts in the body of this module must hand back the very
    buffers (fields ``fields`` of the slot batch ``g``) they are given."""
    cast = lambda k: g[k].to(device=device, dtype=torch.int32).contiguous() if k == "system" else _f64(g[k])
    if not all(cast(k) is g[k] for k in fields):
        raise DosxError(f"{who}: a slot buffer is not in the dtype / layout the float64 program reads")


def _linear_grads(G: Params, key: str, M: int, dy: torch.Tensor, segs) -> None:
    """Weight and bias gradient of nn.Linear ``key`` whose input is cat(segs) and output gradient dy [M, out]."""
    wgrad64(M, dy, segs, G[key + ".weight"])
    colsum64(dy, G[key + ".bias"])


# ---- Linear -> PReLU -> Linear (the encoders, DOSTransformer_phonon.py:129-130) ------------------------------------------
def _mlp_prelu_fwd(P: Params, key: str, inp: torch.Tensor):
    M, H = inp.shape[0], P[key + ".2.weight"].shape[0]
    dev = inp.device
    z, h = alloc64(dev, M, H), alloc64(dev, M, H)
    gemm64(M, H, [seg64(inp)], P[key + ".0.weight"], h, bias=P[key + ".0.bias"], act=ACT64_PRELU,
           alpha=P[key + ".1.weight"], pre=z)
    out = gemm64(M, H, [seg64(h)], P[key + ".2.weight"], alloc64(dev, M, H), bias=P[key + ".2.bias"])
    return out, (inp, z, h)


def _mlp_prelu_bwd(P: Params, G: Params, key: str, ctx, dout: torch.Tensor) -> None:
    inp, z, h = ctx
    M, H = z.shape
    _linear_grads(G, key + ".2", M, dout, [seg64(h)])
    dh = gemm64(M, H, [seg64(dout)], P[key + ".2.weight"], alloc64(dout.device, M, H), w_layout=1)
    dz, part = act_bwd64(dh, z, ACT64_PRELU, P[key + ".1.weight"])
    colsum64(part, G[key + ".1.weight"])
    _linear_grads(G, key + ".0", M, dz, [seg64(inp)])


# ---- Linear -> LayerNorm -> PReLU -> Linear (Edge / Node MLPs, DOSTransformer_phonon.py:193,203-204) ----------------------
def _mlp_ln_fwd(P: Params, key: str, M: int, segs, res: Optional[torch.Tensor]):
    W, H = P[key + ".0.weight"].shape[0], P[key + ".3.weight"].shape[0]
    dev = P[key + ".0.weight"].device
    z = gemm64(M, W, segs, P[key + ".0.weight"], alloc64(dev, M, W), bias=P[key + ".0.bias"])
    xhat, rstd, h = layernorm64(z, P[key + ".1.weight"], P[key + ".1.bias"], P[key + ".2.weight"])
    out = gemm64(M, H, [seg64(h)], P[key + ".3.weight"], alloc64(dev, M, H), bias=P[key + ".3.bias"], res=res)
    return out, (segs, xhat, rstd, h)


def _mlp_ln_bwd(P: Params, G: Params, key: str, ctx, dout: torch.Tensor) -> torch.Tensor:
    """Parameter gradients; returns the gradient of the (virtual) concatenated input, [M, K]."""
    segs, xhat, rstd, h = ctx
    M, W = xhat.shape
    K = P[key + ".0.weight"].shape[1]
    dev = dout.device
    _linear_grads(G, key + ".3", M, dout, [seg64(h)])
    dh = gemm64(M, W, [seg64(dout)], P[key + ".3.weight"], alloc64(dev, M, W), w_layout=1)
    dz, part = layernorm_bwd64(dh, xhat, rstd, P[key + ".1.weight"], P[key + ".1.bias"], P[key + ".2.weight"])
    colsum64(part[:, :W], G[key + ".1.weight"])
    colsum64(part[:, W:2 * W], G[key + ".1.bias"])
    colsum64(part[:, 2 * W:], G[key + ".2.weight"])
    _linear_grads(G, key + ".0", M, dz, segs)
    return gemm64(M, K, [seg64(dz)], P[key + ".0.weight"], alloc64(dev, M, K), w_layout=1)


# ---- one message-passing layer (DOSTransformer_phonon.py:148-171,190-212; scatter_mean aggregation) ------------------------
def _processor_fwd(P: Params, pre: str, x: torch.Tensor, e: torch.Tensor, m: GraphMeta):
    N, E = m.num_nodes, m.num_edges
    segs1 = [seg64(x, rowmap(idx=m.src)), seg64(x, rowmap(idx=m.dst)), seg64(e)]
    msg, c1 = _mlp_ln_fwd(P, pre + ".edge_model.edge_mlp", E, segs1, None)
    agg = segment_mean64(msg, m.rowptr_dst, N)
    e_out = rows_add64(E, e, msg)
    x_out, c2 = _mlp_ln_fwd(P, pre + ".node_model.node_mlp_2", N, [seg64(x), seg64(agg)], x)
    return x_out, e_out, (x, e, msg, agg, c1, c2)


def _processor_bwd(P: Params, G: Params, pre: str, ctx, dx: torch.Tensor, de: Optional[torch.Tensor], m: GraphMeta):
    """(dx, de) of the layer's inputs from those of its outputs (de None: the output edges are not used downstream)."""
    x, e, msg, agg, c1, c2 = ctx
    N, E, H = m.num_nodes, m.num_edges, x.shape[1]
    dcat2 = _mlp_ln_bwd(P, G, pre + ".node_model.node_mlp_2", c2, dx)                 # [N, 2H]: x | agg
    dmsg = segment_mean_bwd64(dcat2[:, H:], m.dst, m.rowptr_dst, de, E)               # + the edge residual
    dcat1 = _mlp_ln_bwd(P, G, pre + ".edge_model.edge_mlp", c1, dmsg)                  # [E, 3H]: x[src] | x[dst] | e
    dx_in = gather_bwd64(dcat1, m, dx, dcat2[:, :H], N, H)
    de_in = rows_add64(E, dcat1[:, 2 * H:], de)
    return dx_in, de_in


# ---- encoders + message-passing layers, shared by the two models (DOSTransformer_phonon.py:74-84) ---------------------
def _gnn_trunk_fwd(P: Params, cfg, g, m: GraphMeta, enc: str):
    vec = g.edge_vec
    if m.edge_perm is not None:
        vec = vec[m.edge_perm]
    e0 = edge_feat_sh1_64(_f64(vec), 4.0)                                              # r_max = 4
    x, cx = _mlp_prelu_fwd(P, enc, _f64(g.x))
    e, ce = _mlp_prelu_fwd(P, "GN_encoder.edge_encoder", e0)
    layers = []
    for l in range(cfg.L):
        x, e, c = _processor_fwd(P, f"stacked_processor.{l}", x, e, m)
        layers.append(c)
    return x, (enc, cx, ce, layers)


def _gnn_trunk_bwd(P: Params, G: Params, cfg, m: GraphMeta, ctx, dx: torch.Tensor) -> None:
    enc, cx, ce, layers = ctx
    de = None
    for l in reversed(range(cfg.L)):
        dx, de = _processor_bwd(P, G, f"stacked_processor.{l}", layers[l], dx, de, m)
    if de is None:                                                                    # L = 0: nothing reaches the edges
        de = ops.keep_alive(torch.zeros(m.num_edges, cfg.H, device=dx.device, dtype=torch.float64))
    _mlp_prelu_bwd(P, G, "GN_encoder.edge_encoder", ce, de)
    _mlp_prelu_bwd(P, G, enc, cx, dx)


def _is_padded(g) -> bool:
    """A ghost-padded batch (batch.pad_batch) or bucket (slots.Slot.empty): it carries its real node count."""
    return getattr(g, "real_nodes", None) is not None


def _dpool_rows(dev, B: int, H: int, padded: bool) -> torch.Tensor:
    """The sum pool's gradient buffer, [B + 1, H]: the GEMM writes rows [0, B); row B is what a ghost node's ``node_graph``
    entry (= B, batch.pad_batch) gathers.  It is zeroed here by torch - once, when the buffer is made, and so outside a recorded
    launch list, which keeps the buffer alive and never writes that row again.  An unpadded batch never reads it."""
    dpool = alloc64(dev, B + 1, H)
    if padded:
        dpool[B:].zero_()
    return dpool


class _FactoredCtx64(NamedTuple):
    """graphnetwork_phonon_fwd(factored_head=True).  padded: the batch is ghost-padded (_dpool_rows)."""
    trunk: tuple
    xL: torch.Tensor
    pool: torch.Tensor
    graph: torch.Tensor
    E1: torch.Tensor
    C: torch.Tensor
    padded: bool


def _pair_head_fwd(P: Params, cfg, B: int, graph: torch.Tensor):
    """out_layer on cat[emb[s] | graph[b]] over all (s, b), on its rank structure -> (dos [B, S], E1 [S, H], C [B, H]): the first
    Linear is E1[s] + C[b], one small product with each column half of its weight; the rest is one launch."""
    H, S, dev = cfg.H, cfg.S, graph.device
    W0 = P["out_layer.0.weight"]
    E1 = gemm64(S, H, [seg64(P["embeddings.weight"])], W0[:, :H], alloc64(dev, S, H), bias=P["out_layer.0.bias"])
    C = gemm64(B, H, [seg64(graph)], W0[:, H:], alloc64(dev, B, H))
    dos = alloc64(dev, B, S)
    pair_head_fwd64(E1, C, P["out_layer.2.weight"], P["out_layer.2.bias"], dos, 0.01)
    return dos, E1, C


def _pair_head_bwd(P: Params, G: Params, cfg, B: int, graph, E1, C, ddos: torch.Tensor) -> torch.Tensor:
    """Backward of _pair_head_fwd: the gradients of out_layer.* and embeddings.weight; returns dL/dgraph [B, H]."""
    H, S, dev = cfg.H, cfg.S, E1.device
    emb, W0, dW0 = P["embeddings.weight"], P["out_layer.0.weight"], G["out_layer.0.weight"]
    dE1, dC = alloc64(dev, S, H), alloc64(dev, B, H)
    part = alloc64(dev, pair_head_partial_rows(S, B), H + 1)
    pair_head_bwd64(ddos.to(torch.float64).contiguous(), E1, C, P["out_layer.2.weight"], dE1, dC, part, 0.01)
    colsum64(part[:, :H], G["out_layer.2.weight"])
    colsum64(part[:, H:], G["out_layer.2.bias"])
    wgrad64(S, dE1, [seg64(emb)], dW0[:, :H])                                          # the two column halves, written in place
    wgrad64(B, dC, [seg64(graph)], dW0[:, H:])
    colsum64(dE1, G["out_layer.0.bias"])
    gemm64(S, H, [seg64(dE1)], W0[:, :H], G["embeddings.weight"], w_layout=1)
    return gemm64(B, H, [seg64(dC)], W0[:, H:], alloc64(dev, B, H), w_layout=1)


def _factored_fwd(P: Params, cfg, g, m: GraphMeta, enc: str):
    H, B = cfg.H, m.num_graphs
    x, ctrunk = _gnn_trunk_fwd(P, cfg, g, m, enc)
    pool = graph_pool64(x, m.graph_ptr, B)
    graph = gemm64(B, H, [seg64(pool)], P["GN_decoder.mlp.0.weight"], alloc64(x.device, B, H), bias=P["GN_decoder.mlp.0.bias"])
    dos, E1, C = _pair_head_fwd(P, cfg, B, graph)
    return dos, _FactoredCtx64(ctrunk, x, pool, graph, E1, C, _is_padded(g))


def _factored_bwd(P: Params, G: Params, cfg, m: GraphMeta, ctx: _FactoredCtx64, ddos: torch.Tensor) -> None:
    H, B, N = cfg.H, m.num_graphs, m.num_nodes
    dev = ctx.E1.device
    dgraph = _pair_head_bwd(P, G, cfg, B, ctx.graph, ctx.E1, ctx.C, ddos)
    _linear_grads(G, "GN_decoder.mlp.0", B, dgraph, [seg64(ctx.pool)])
    dpool = gemm64(B, H, [seg64(dgraph)], P["GN_decoder.mlp.0.weight"], _dpool_rows(dev, B, H, ctx.padded), w_layout=1)
    _gnn_trunk_bwd(P, G, cfg, m, ctx.trunk, rows_add64(N, dpool, ia=m.node_graph))     # backward of the sum pool


def graphnetwork_phonon_fwd(P: Params, cfg, g, m: GraphMeta, factored_head: bool = False):
    """-> (dos [B, S], saved context).  ``factored_head``: the output head on its rank structure (the module docstring;
    train64.GraphnetworkTrainer64 / predict.Predictor64) - recordable and padding-safe; the default is the module's own path."""
    H, S, B = cfg.H, cfg.S, m.num_graphs
    enc = "GN_encoder.node_encoder" if g.x.shape[1] == 118 else "GN_encoder.node_encoder_prompt"   # :150-153
    if factored_head:
        return _factored_fwd(P, cfg, g, m, enc)
    x, ctrunk = _gnn_trunk_fwd(P, cfg, g, m, enc)
    pool = graph_pool64(x, m.graph_ptr, B)
    graph = gemm64(B, H, [seg64(pool)], P["GN_decoder.mlp.0.weight"], alloc64(x.device, B, H), bias=P["GN_decoder.mlp.0.bias"])
    # head on cat[energies, graph] over the [S, B] rows r = s * B + b (graphnetwork_phonon.py:68-71)
    emb = P["embeddings.weight"]
    head = [seg64(emb, rowmap(d=B, m=1, c=0)), seg64(graph, rowmap(d=B, m=0, c=1))]
    hid_pre, hid = alloc64(x.device, S * B, H), alloc64(x.device, S * B, H)
    gemm64(S * B, H, head, P["out_layer.0.weight"], hid, bias=P["out_layer.0.bias"], act=ACT64_LEAKY, pre=hid_pre)
    out = gemm64(S * B, 1, [seg64(hid)], P["out_layer.2.weight"], alloc64(x.device, S * B, 1), bias=P["out_layer.2.bias"])
    dos = out.view(S, B).t().contiguous()
    return dos, (ctrunk, pool, (head, graph), hid_pre, hid)     # graph: keeps the memory `head` points to


def graphnetwork_phonon_bwd(P: Params, G: Params, cfg, m: GraphMeta, saved, ddos: torch.Tensor,
                            factored_head: bool = False) -> None:
    """Writes the gradient of every live parameter into G from ddos [B, S]."""
    if factored_head != isinstance(saved, _FactoredCtx64):
        raise ValueError("graphnetwork_phonon_bwd: factored_head differs from the forward pass that made this context")
    if factored_head:
        return _factored_bwd(P, G, cfg, m, saved, ddos)
    ctrunk, pool, (head, _), hid_pre, hid = saved
    H, S, B, N = cfg.H, cfg.S, m.num_graphs, m.num_nodes
    dev = ddos.device
    rows = S * B
    dout = ddos.to(torch.float64).t().contiguous().view(rows, 1)
    _linear_grads(G, "out_layer.2", rows, dout, [seg64(hid)])
    dhid = gemm64(rows, H, [seg64(dout)], P["out_layer.2.weight"], alloc64(dev, rows, H), w_layout=1)
    dpre, _ = act_bwd64(dhid, hid_pre, ACT64_LEAKY)
    _linear_grads(G, "out_layer.0", rows, dpre, head)
    # input gradient of the head: the energies are broadcast over the crystals and the graph rows over the bins, so sum
    # those rows first (in order), then one small product with each half of out_layer.0.weight
    W0 = P["out_layer.0.weight"]
    Rs = reduce_rows64(dpre, S, B, B, 1)
    gemm64(S, H, [seg64(Rs)], W0[:, :H], G["embeddings.weight"], w_layout=1)
    Rb = reduce_rows64(dpre, B, S, 1, B)
    dgraph = gemm64(B, H, [seg64(Rb)], W0[:, H:], alloc64(dev, B, H), w_layout=1)
    _linear_grads(G, "GN_decoder.mlp.0", B, dgraph, [seg64(pool)])
    dpool = gemm64(B, H, [seg64(dgraph)], P["GN_decoder.mlp.0.weight"], alloc64(dev, B, H), w_layout=1)
    _gnn_trunk_bwd(P, G, cfg, m, ctrunk, rows_add64(N, dpool, ia=m.node_graph))       # backward of the sum pool


# ---- DOSTransformer_phonon ------------------------------------------------------------------------------------------------
class _EncoderLayer64(NamedTuple):
    """One layer of _encoder_fwd: LayerNorm 0 of the queries (normalised rows, 1 / std, output), the attention dropout mask or
    None, the softmax weights, LayerNorm 1 of the attention half's output (normalised rows, 1 / std, output), relu(fc1)."""
    xhq: torch.Tensor
    rsq: torch.Tensor
    q: torch.Tensor
    mask: Optional[torch.Tensor]
    probs: torch.Tensor
    xh1: torch.Tensor
    rs1: torch.Tensor
    y1: torch.Tensor
    h: torch.Tensor


class _EncoderCtx64(NamedTuple):
    pre: str
    layers: List[_EncoderLayer64]
    xhf: torch.Tensor                  # the final LayerNorm's normalised rows ...
    rsf: torch.Tensor                  # ... and 1 / std
    Sq: int
    Bq: int
    Nk: int
    Bk: int
    kvhat: torch.Tensor
    key_ptr: Optional[torch.Tensor]


class _ModelCtx64(NamedTuple):
    """dostransformer_phonon_fwd.  padded: the batch is ghost-padded (_dpool_rows)."""
    trunk: tuple
    kv_n: torch.Tensor
    rstd_n: torch.Tensor
    c1: _EncoderCtx64
    pool: torch.Tensor
    graph: torch.Tensor
    prow: torch.Tensor
    sysidx: torch.Tensor
    seg_g: list
    seg_s: list
    pre: torch.Tensor
    dosin: torch.Tensor
    ptr_s: torch.Tensor
    kv_s: torch.Tensor
    rstd_s: torch.Tensor
    c2: _EncoderCtx64
    c3: _EncoderCtx64
    hsrc: torch.Tensor
    E1: torch.Tensor
    padded: bool


def _encoder_fwd(P: Params, pre: str, x: torch.Tensor, Sq: int, Bq: int, kvhat: torch.Tensor, Nk: int, Bk: int, T: int, drop,
                 key_ptr: Optional[torch.Tensor] = None):
    """TransformerEncoder (layers/transformer.py:46-79,120-157) on the query rows x [Bq*Sq, H] (row bq * Sq + s) over the
    normalised key rows kvhat [Bk*Nk, H], which stay the same for every layer (:72-73).  drop: None or (p, seed_dev,
    stream_base): attention dropout, one [Bq, Sq, Nk] multiplier mask per layer drawn like the fp32 program's.  key_ptr
    (int32 [Bk + 1]): each key crystal's own row count - the padding rows past it take no part (DosxAttn64.key_ptr)."""
    rows, H = x.shape
    lay = []
    for t in range(T):
        lp = f"{pre}.layers.{t}"
        g0, b0 = P[lp + ".layer_norms.0.weight"], P[lp + ".layer_norms.0.bias"]
        xhq, rsq, q = layernorm64(x, g0, b0)
        mask = None
        if drop is not None:
            mask = ops.keep_alive(torch.empty(Bq, Sq, Nk, device=x.device, dtype=torch.float32))
            ops.dropout_mask(mask, drop[0], drop[1], drop[2] + t)
            if Fn.DROP_MASK_LOG is not None:
                Fn.DROP_MASK_LOG.append((pre, t, mask))
        x1, probs = attention64(q, x, kvhat, g0, b0, Sq, Bq, Nk, Bk, mask, SOFTMAX64, key_ptr)
        xh1, rs1, y1 = layernorm64(x1, P[lp + ".layer_norms.1.weight"], P[lp + ".layer_norms.1.bias"])
        h = gemm64(rows, 4 * H, [seg64(y1)], P[lp + ".fc1.weight"], alloc64(x.device, rows, 4 * H), bias=P[lp + ".fc1.bias"],
                   act=ACT64_RELU)
        x2 = gemm64(rows, H, [seg64(h)], P[lp + ".fc2.weight"], alloc64(x.device, rows, H), bias=P[lp + ".fc2.bias"], res=x1)
        lay.append(_EncoderLayer64(xhq, rsq, q, mask, probs, xh1, rs1, y1, h))
        x = x2
    xhf, rsf, y = layernorm64(x, P[pre + ".layer_norm.weight"], P[pre + ".layer_norm.bias"])
    return y, _EncoderCtx64(pre, lay, xhf, rsf, Sq, Bq, Nk, Bk, kvhat, key_ptr)


def _encoder_bwd(P: Params, G: Params, ctx, dy: torch.Tensor, dkvhat: torch.Tensor, kacc: bool) -> torch.Tensor:
    """Gradient of the query rows; every layer's key + value gradient (times gamma0) goes into dkvhat, the first one written
    unless kacc (accumulate) - the key rows of the dense batch are read by two encoders."""
    pre, Sq, Bq, Nk, Bk, kvhat, key_ptr = ctx.pre, ctx.Sq, ctx.Bq, ctx.Nk, ctx.Bk, ctx.kvhat, ctx.key_ptr
    rows, H = dy.shape
    dev = dy.device

    def ln_grads(key, part, acc=False):
        colsum64(part[:, :H], G[key + ".weight"], acc)
        colsum64(part[:, H:2 * H], G[key + ".bias"], acc)

    dx, part = layernorm_bwd64(dy, ctx.xhf, ctx.rsf, P[pre + ".layer_norm.weight"], P[pre + ".layer_norm.bias"])
    ln_grads(pre + ".layer_norm", part)
    for t in reversed(range(len(ctx.layers))):
        lp = f"{pre}.layers.{t}"
        lay = ctx.layers[t]
        q, mask, probs, y1, h = lay.q, lay.mask, lay.probs, lay.y1, lay.h
        g0, b0 = P[lp + ".layer_norms.0.weight"], P[lp + ".layer_norms.0.bias"]
        # x2 = x1 + fc2(relu(fc1(LN1(x1))))
        _linear_grads(G, lp + ".fc2", rows, dx, [seg64(h)])
        dh = gemm64(rows, 4 * H, [seg64(dx)], P[lp + ".fc2.weight"], alloc64(dev, rows, 4 * H), w_layout=1)
        dhz, _ = act_bwd64(dh, h, ACT64_RELU)                    # relu(z) > 0 exactly where z > 0
        _linear_grads(G, lp + ".fc1", rows, dhz, [seg64(y1)])
        dy1 = gemm64(rows, H, [seg64(dhz)], P[lp + ".fc1.weight"], alloc64(dev, rows, H), w_layout=1)
        dz1, part1 = layernorm_bwd64(dy1, lay.xh1, lay.rs1, P[lp + ".layer_norms.1.weight"], P[lp + ".layer_norms.1.bias"])
        ln_grads(lp + ".layer_norms.1", part1)
        dx1 = rows_add64(rows, dx, dz1)
        # x1 = x + attention(LN0(x), LN0(keys))
        dq, partk, _ = attention_bwd64(dx1, q, kvhat, g0, b0, probs, Sq, Bq, Nk, Bk, dkvhat, mask, SOFTMAX64, kacc, key_ptr)
        kacc = True
        dzq, partq = layernorm_bwd64(dq, lay.xhq, lay.rsq, g0, b0)
        ln_grads(lp + ".layer_norms.0", partq)
        ln_grads(lp + ".layer_norms.0", partk, True)
        dx = rows_add64(rows, dx1, dzq)
    return dx


def dostransformer_phonon_fwd(P: Params, cfg, g, m: GraphMeta, drop=None, per_crystal_keys: bool = False):
    """-> (dos [2B, S] (rows [0,B) global, [B,2B) system), x_L [N, H], saved context).  drop: None or (p, seed_dev).
    per_crystal_keys: the two encoders that attend over atoms see each crystal's own atoms only, not the rows that pad it to
    the batch's largest crystal - every crystal gets what the reference gives it at batch_size = 1 (main_phDOS.py:52-55),
    and the backward is the sum of those per-sample gradients.  The dropout masks keep their [Bq, S, nmax] layout."""
    H, S, T, B = cfg.H, cfg.S, cfg.T, m.num_graphs
    nmax = m.n_max
    kp = m.graph_ptr if per_crystal_keys else None
    dr = (lambda base: None) if drop is None else (lambda base: (drop[0], drop[1], base))
    xL, ctrunk = _gnn_trunk_fwd(P, cfg, g, m, "GN_encoder.node_encoder")                # :74-84
    dev = xL.device
    kv_n, rstd_n = dense_rows64(xL, m.graph_ptr, B, nmax)                               # :86-87, the keys' LN0 without affine
    # energies (:71,143): embedding row s for every crystal, crystal-major
    e_idx = ops.keep_alive((torch.arange(B * S, device=dev, dtype=torch.int32) % S).contiguous())
    E1, c1 = _encoder_fwd(P, "transformer", rows_add64(B * S, P["embeddings.weight"], ia=e_idx), S, B, kv_n, nmax, B, T, dr(0),
                          kp)
    pool = graph_pool64(xL, m.graph_ptr, B)                                              # :90, :180-181
    graph = gemm64(B, H, [seg64(pool)], P["GN_decoder.mlp.0.weight"], alloc64(dev, B, H), bias=P["GN_decoder.mlp.0.bias"])
    sysidx = g.system.to(device=dev, dtype=torch.int32).contiguous()
    prow = rows_add64(B, P["prompt_token.weight"], ia=sysidx)                            # :105
    # heads (:93-117): rows [0, B*S) the global branch, [B*S, 2B*S) the system branch
    perB = rowmap(d=S, m=1, c=0)
    BS = B * S
    dosin, pre = alloc64(dev, 2 * BS, H), alloc64(dev, 2 * BS, H)
    seg_g = [seg64(E1), seg64(graph, perB)]
    seg_s = [seg64(E1), seg64(graph, perB), seg64(prow, perB)]
    gemm64(BS, H, seg_g, P["fc.weight"], dosin[:BS], bias=P["fc.bias"], act=ACT64_LEAKY, pre=pre[:BS])
    gemm64(BS, H, seg_s, P["fc_prompt.weight"], dosin[BS:], bias=P["fc_prompt.bias"], act=ACT64_LEAKY, pre=pre[BS:])
    # both branches through each shared encoder at once: Bq = 2B, global crystals first (the masks' layout)
    ptr_s = ops.keep_alive(torch.arange(0, 2 * BS + 1, S, device=dev, dtype=torch.int32))
    kv_s, rstd_s = dense_rows64(dosin, ptr_s, 2 * B, S)                                  # self attention: its own rows
    hs, c2 = _encoder_fwd(P, "transformer_self", dosin, S, 2 * B, kv_s, S, 2 * B, T, dr(64))
    hsrc, c3 = _encoder_fwd(P, "transformer_source", hs, S, 2 * B, kv_n, nmax, B, T, dr(128), kp)
    dos = gemm64(2 * BS, 1, [seg64(hsrc)], P["out_layer.weight"], alloc64(dev, 2 * BS, 1), bias=P["out_layer.bias"])
    ctx = _ModelCtx64(trunk=ctrunk, kv_n=kv_n, rstd_n=rstd_n, c1=c1, pool=pool, graph=graph, prow=prow, sysidx=sysidx, seg_g=seg_g,
                      seg_s=seg_s, pre=pre, dosin=dosin, ptr_s=ptr_s, kv_s=kv_s, rstd_s=rstd_s, c2=c2, c3=c3, hsrc=hsrc, E1=E1,
                      padded=_is_padded(g))
    return dos.view(2 * B, S), xL, ctx


def dostransformer_phonon_bwd(P: Params, G: Params, cfg, m: GraphMeta, ctx, ddos: torch.Tensor,
                              dx_ext: Optional[torch.Tensor]) -> None:
    """Writes the gradient of every live parameter into G from ddos [2B, S] and the gradient of x_L (or None)."""
    ctrunk, c1, c2, c3, kv_n, rstd_n, kv_s, rstd_s, ptr_s = ctx.trunk, ctx.c1, ctx.c2, ctx.c3, ctx.kv_n, ctx.rstd_n, ctx.kv_s, ctx.rstd_s, ctx.ptr_s
    pool, sysidx, seg_g, seg_s, pre, dosin, hsrc, padded = ctx.pool, ctx.sysidx, ctx.seg_g, ctx.seg_s, ctx.pre, ctx.dosin, ctx.hsrc, ctx.padded
    H, S, B, N = cfg.H, cfg.S, m.num_graphs, m.num_nodes
    nmax = m.n_max
    BS = B * S
    dev = dosin.device
    dout = ddos.to(torch.float64).contiguous().view(2 * BS, 1)
    _linear_grads(G, "out_layer", 2 * BS, dout, [seg64(hsrc)])
    dh = gemm64(2 * BS, H, [seg64(dout)], P["out_layer.weight"], alloc64(dev, 2 * BS, H), w_layout=1)
    dkv_n = alloc64(dev, B * nmax, H)
    dh = _encoder_bwd(P, G, c3, dh, dkv_n, False)
    dkv_s = alloc64(dev, 2 * BS, H)
    ddosin = _encoder_bwd(P, G, c2, dh, dkv_s, False)
    dense_rows_bwd64(dkv_s, kv_s, rstd_s, ptr_s, ddosin, 2 * B, S)                      # keys of the self attention
    dpre, _ = act_bwd64(ddosin, pre, ACT64_LEAKY)
    _linear_grads(G, "fc", BS, dpre[:BS], seg_g)
    _linear_grads(G, "fc_prompt", BS, dpre[BS:], seg_s)
    dcat_g = gemm64(BS, 2 * H, [seg64(dpre[:BS])], P["fc.weight"], alloc64(dev, BS, 2 * H), w_layout=1)
    K = P["fc_prompt.weight"].shape[1]
    dcat_s = gemm64(BS, K, [seg64(dpre[BS:])], P["fc_prompt.weight"], alloc64(dev, BS, K), w_layout=1)
    dE1 = rows_add64(BS, dcat_g[:, :H], dcat_s[:, :H])
    dgraph = reduce_rows64(rows_add64(BS, dcat_g[:, H:], dcat_s[:, H:2 * H]), B, S, S, 1)
    index_sum64(reduce_rows64(dcat_s[:, 2 * H:], B, S, S, 1), sysidx, G["prompt_token.weight"])
    _linear_grads(G, "GN_decoder.mlp.0", B, dgraph, [seg64(pool)])
    dpool = gemm64(B, H, [seg64(dgraph)], P["GN_decoder.mlp.0.weight"], _dpool_rows(dev, B, H, padded), w_layout=1)
    dx0 = _encoder_bwd(P, G, c1, dE1, dkv_n, True)
    reduce_rows64(dx0, S, B, 1, S, out=G["embeddings.weight"])                         # energy s: rows b * S + s
    dx = rows_add64(N, dpool, None if dx_ext is None else dx_ext.to(torch.float64).contiguous(), ia=m.node_graph)
    dense_rows_bwd64(dkv_n, kv_n, rstd_n, m.graph_ptr, dx, B, nmax)
    _gnn_trunk_bwd(P, G, cfg, m, ctrunk, dx)
