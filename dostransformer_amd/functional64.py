"""float64 forward / backward program of ``Graphnetwork_phonon`` (`embedder_phDOS/graphnetwork_phonon.py:48-72`).

The phonon reference computes in float64 (main_phDOS.py:15-16).  A module whose live parameters are float64 runs this
program instead of the fp32 one in ``functional.py``: the same steps as ``oracle.graphnetwork_phonon_forward`` in order,
each a libdosx fp64 kernel (csrc/f64.hip), with the backward written out step by step in reverse.  Straight-line on the
current stream, no fused-path heuristics; every reduction has a fixed order, so two runs are bitwise equal.

Edges are processed in the destination-sorted order of ``GraphMeta`` (``edge_perm`` maps the caller's order to it).
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from .batch import GraphMeta
from .ops import (ACT64_LEAKY, ACT64_PRELU, act_bwd64, alloc64, colsum64, edge_feat_sh1_64, gather_bwd64, gemm64,
                  graph_pool64, layernorm64, layernorm_bwd64, reduce_rows64, rows_add64, rowmap, seg64, segment_mean64,
                  segment_mean_bwd64, wgrad64)

Params = Dict[str, torch.Tensor]

MAX_HIDDEN = 512          # the LayerNorm rows of the edge / node MLPs are 2H wide, dosx_layernorm_f64 takes up to 1024


def _f64(t: torch.Tensor) -> torch.Tensor:
    """A batch field as the program reads it: float64, contiguous (an fp32 batch is promoted here, once)."""
    return t.to(torch.float64).contiguous()


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


def graphnetwork_phonon_fwd(P: Params, cfg, g, m: GraphMeta):
    """-> (dos [B, S], saved context)."""
    H, S, B, L = cfg.H, cfg.S, m.num_graphs, cfg.L
    vec = g.edge_vec
    if m.edge_perm is not None:
        vec = vec[m.edge_perm]
    e0 = edge_feat_sh1_64(_f64(vec), 4.0)                                              # r_max = 4
    xin = _f64(g.x)
    enc = "GN_encoder.node_encoder" if xin.shape[1] == 118 else "GN_encoder.node_encoder_prompt"   # :150-153
    x, cx = _mlp_prelu_fwd(P, enc, xin)
    e, ce = _mlp_prelu_fwd(P, "GN_encoder.edge_encoder", e0)
    layers = []
    for l in range(L):
        x, e, c = _processor_fwd(P, f"stacked_processor.{l}", x, e, m)
        layers.append(c)
    pool = graph_pool64(x, m.graph_ptr, B)
    graph = gemm64(B, H, [seg64(pool)], P["GN_decoder.mlp.0.weight"], alloc64(x.device, B, H), bias=P["GN_decoder.mlp.0.bias"])
    # head on cat[energies, graph] over the [S, B] rows r = s * B + b (graphnetwork_phonon.py:68-71)
    emb = P["embeddings.weight"]
    head = [seg64(emb, rowmap(d=B, m=1, c=0)), seg64(graph, rowmap(d=B, m=0, c=1))]
    hid_pre, hid = alloc64(x.device, S * B, H), alloc64(x.device, S * B, H)
    gemm64(S * B, H, head, P["out_layer.0.weight"], hid, bias=P["out_layer.0.bias"], act=ACT64_LEAKY, pre=hid_pre)
    out = gemm64(S * B, 1, [seg64(hid)], P["out_layer.2.weight"], alloc64(x.device, S * B, 1), bias=P["out_layer.2.bias"])
    dos = out.view(S, B).t().contiguous()
    return dos, (enc, cx, ce, layers, pool, (head, graph), hid_pre, hid)     # graph: keeps the memory `head` points to


def graphnetwork_phonon_bwd(P: Params, G: Params, cfg, m: GraphMeta, saved, ddos: torch.Tensor) -> None:
    """Writes the gradient of every live parameter into G from ddos [B, S]."""
    enc, cx, ce, layers, pool, (head, _), hid_pre, hid = saved
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
    dx = rows_add64(N, dpool, ia=m.node_graph)                                       # backward of the sum pool
    de = None
    for l in reversed(range(cfg.L)):
        dx, de = _processor_bwd(P, G, f"stacked_processor.{l}", layers[l], dx, de, m)
    if de is None:                                                                    # L = 0: nothing reaches the edges
        de = torch.zeros(m.num_edges, H, device=dev, dtype=torch.float64)
    _mlp_prelu_bwd(P, G, "GN_encoder.edge_encoder", ce, de)
    _mlp_prelu_bwd(P, G, enc, cx, dx)
