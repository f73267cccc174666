/* dosx.h — C ABI of libdosx.so: the MI355X (gfx950) hot path of DOSTransformer.
 *
 * The reference (HeewoongNoh/DOSTransformer) is pure Python and has NO FFI / plugin
 * boundary of its own; its hot path is a chain of implicit PyTorch /
 * torch_scatter / PyG kernels.  This header is the boundary the build introduces:
 * every entry point replaces a group of those implicit launches, and the Python
 * modules in dostransformer_amd/ (same class names / ctor signatures / state_dict
 * keys as the reference's embedder_phDOS, embedder_eDOS and layers packages) bind
 * them through ctypes (see INTEGRATION.md for the stub).
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is DEVICE memory unless noted;
 *    all floating point data is fp32 row-major, all index data int32;
 *  - nothing is allocated, freed or retained by the library: the caller passes
 *    outputs and scratch ("partials") buffers;
 *  - every call is asynchronous on the given hipStream_t, re-entrant and
 *    graph-capturable (no hidden synchronisation, no host<->device copies);
 *  - return value 0 on success, negative on error; dosx_last_error() gives a
 *    thread-local message.
 */
#ifndef DOSX_H
#define DOSX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* dosx_stream_t; /* hipStream_t */

/* Row indirection used for gathered operands and remapped outputs:
 *   t = (r / d) * m + (r % d) * c + off ;  row = idx ? idx[t] : t
 * identity: d = 1<<30, m = 0, c = 1, off = 0.  r % B: d=B,m=0,c=1.  r / B: d=B,m=1,c=0. */
typedef struct DosxRowMap {
  int32_t d, m, c, off;
  const int32_t* idx;
} DosxRowMap;

/* One K-segment of a (virtually concatenated, row-gathered) matrix operand.
 * Replaces torch.cat([x[row], x[col], edge_attr], 1) (DOSTransformer_phonon.py:166,194). */
typedef struct DosxSeg {
  const float* p;
  int32_t ld;    /* row stride in floats */
  int32_t width; /* columns taken from this segment */
  DosxRowMap map;
} DosxSeg;

/* Prologue applied to the A operand while it is staged into LDS. */
enum {
  DOSX_PRO_NONE = 0,
  DOSX_PRO_PRELU = 1,    /* a = z >= 0 ? z : alpha*z            (nn.PReLU, DOSTransformer_phonon.py:129) */
  DOSX_PRO_LN_PRELU = 2, /* a = prelu(xhat*gamma + beta)          (LayerNorm+PReLU of Edge/NodeModel, :193,204) */
  DOSX_PRO_ROWLN = 3     /* a = (x-mean[r])*rstd[r]*gamma + beta  (pre-norm LN, layers/transformer.py:141-142) */
};

/* Epilogues of dosx_gemm (all but PLAIN/BIAS_ACT need the whole row in one tile: N <= 512). */
enum {
  DOSX_EPI_BIAS_ACT = 0,     /* out = act(acc + bias) [+ res]; act: 0 none, 1 relu, 2 leaky(slope)   */
  DOSX_EPI_LN = 1,           /* out = xhat = LN_noaffine(acc + bias); aux_out = rstd[M]              */
  DOSX_EPI_PRELU_LN_BWD = 2, /* acc = dL/d prelu(y), y = xhat*g+b  ->  out = dL/dz (pre-LN)          */
  DOSX_EPI_RELU_MASK = 3,    /* out = acc * (aux > 0)                                                 */
  DOSX_EPI_ROWLN_BWD = 4,    /* acc = dL/d LN(x) -> out = res + dL/dx ; x = aux, stats = aux_stats    */
  DOSX_EPI_PRELU_BWD = 5,    /* out = acc * (aux >= 0 ? 1 : alpha); partial dalpha                    */
  DOSX_EPI_SEGSUM = 6,       /* message GEMM of a GNN layer with the aggregation in its epilogue (a5 + a6):
                                msg = acc + bias stays in LDS;  seg_agg[n] = seg_scale[n] * sum_{e in seg(n)} msg[e];
                                out = msg + res (the edge residual e' = e + msg) unless out is NULL.  Row tiles are
                                node-aligned: workgroup t owns rows [seg_tile[t], seg_tile[t+1]) (<= 48) = the whole
                                destination segments of the nodes [seg_tile[T+1+t], seg_tile[T+2+t]), T = seg_ntiles    */
  DOSX_EPI_PRELU_LN_BWD_SEG = 7 /* EPI_PRELU_LN_BWD on the node-aligned row tiles of EPI_SEGSUM (same seg_* fields, w_layout 1,
                                N <= 256): out = dL/dz as before AND seg_agg[n] = seg_scale[n] * sum_{e in seg(n)} out[e] - the
                                destination-node sums of dz that the FACTORED first Linear of the EdgeModel needs for its
                                weight and input gradients (DOSTransformer_phonon.py:190-197: cat[x[row], x[col], e] W1^T =
                                (x Wa^T)[row] + (x Wb^T)[col] + e Wc^T, so dWb = (sum_{e: col(e)=n} dz_e)^T x).  One partial
                                row per TILE (seg_ntiles rows, empty tiles write zeros).                                  */
};

/* C[M,N] = epilogue( prologue(A)[M,K] * B ),  fp32 MFMA (v_mfma_f32_32x32x2_f32).
 * w_layout 0: B = W^T with W[N,K] row-major  (nn.Linear forward,  y = x W^T + b)
 * w_layout 1: B = W   with W[K,N] row-major  (nn.Linear backward, dx = dy W)         */
typedef struct DosxGemm {
  int32_t M, N, K;
  int32_t nseg;
  DosxSeg a[3];
  int32_t pro;
  const float* pro_gamma;
  const float* pro_beta;
  const float* pro_alpha; /* device scalar */
  const float* pro_stats; /* [M,2] mean,rstd (ROWLN) */
  const float* w;
  int32_t ldw;
  int32_t w_layout;
  int32_t epi;
  int32_t act;
  float act_slope;
  const float* bias;
  float* out;
  int32_t ldo;
  DosxRowMap out_map;
  const float* res;
  int32_t ldr;
  DosxRowMap res_map;
  float* stats_out;   /* EPI_BIAS_ACT only (refused behind any other epilogue), optional [M,2], N <= 512: mean, rstd of the final output rows */
  float* aux_out;     /* EPI_LN: rstd [M] */
  const float* aux;   /* backward epilogues: xhat / h / x / z, [M, ldaux] */
  int32_t ldaux;
  const float* aux_stats; /* rstd [M] (PRELU_LN_BWD) or [M,2] mean,rstd (ROWLN_BWD) */
  const float* epi_gamma;
  const float* epi_beta;
  const float* epi_alpha;
  float* partials;    /* per-workgroup partial sums: row wg = [dgamma(N) | dbeta(N) | dalpha] */
  int32_t partial_ld;
  /* EPI_SEGSUM only */
  const int32_t* seg_tile;   /* [3][seg_ntiles + 1]: row (edge) boundaries, node boundaries, chunk info of the node-aligned tiles.
                                chunk info != 0 (= chunk << 16 | chunks): the tile's first node has more than 48 incoming edges
                                and the tile owns that chunk of its rows (all but the last chunk are full tiles without
                                other nodes); the chunk sums of a node are published to seg_part and added in chunk order by
                                the last arriving tile (ticket on seg_cnt) - deterministic, no second launch */
  int32_t seg_ntiles;
  const int32_t* seg_rowptr; /* [nodes + 1] CSR by destination */
  const float* seg_scale;    /* [nodes] 1/max(in-degree,1) for scatter_mean, NULL for scatter_sum */
  float* seg_agg;            /* [nodes, N] */
  float* seg_part;           /* [seg_ntiles, N] scratch for the chunk sums of over-full nodes.  REQUIRED (like seg_cnt): the table lives in
                                device memory, so the host cannot know whether a tile carries chunk info; a call without it is
                                refused (-22) instead of silently dropping an over-full node's aggregate */
  int32_t* seg_cnt;          /* [seg_ntiles] arrival counters, zero before the launch, zero again after it (like DosxWgrad.counters) */
  int32_t res_col0;   /* EPI_BIAS_ACT: the residual is added to the output columns [res_col0, N) only, res column c
                         to output column res_col0 + c (0 = all columns).  The backward of the edge residual
                         e += e' (DOSTransformer_phonon.py:84) rides on the e-block of the [E,3H] concat gradient. */
  float* norm_out;    /* EPI_BIAS_ACT, optional (N <= 512): ALSO the LayerNorm-normalised output rows without affine,
                         (y - mean) * rstd, eps 1e-5, at the same (mapped) rows and leading dimension as `out` - the
                         stale keys of the self-attention encoder are the normalised head outputs (layers/transformer.py:
                         131-134 on DOSTransformer_phonon.py:97's input), so the heads' GEMMs write them and no
                         dosx_rownorm launch follows */
  float* norm_rstd;   /* with norm_out: rstd per OUTPUT row [rows of out] */
  int32_t res_pre;    /* EPI_BIAS_ACT: 1 = the residual rows are added BEFORE the activation, out = act(A W + bias + res[res_map(r)]).
                         The K-segments of an output head that are constant along the energy axis - cat[x, graph(, prompt)]
                         (DOSTransformer_phonon.py:93-95,105-109) repeats the pooled crystal vector for every energy - are
                         multiplied once per crystal and enter the per-energy GEMM as such a row-mapped pre-activation term. */
  /* EPI_LN, optional: two GATHERED row addends in front of the LayerNorm statistics (round 5),
   *     xhat[r] = LN_noaffine( acc[r] + bias + add_p[add_ip[r]] + add_q[add_iq[r]] ),   rows of add_p / add_q: N floats, stride ld_add.
   * The EdgeModel's first Linear on cat[x[row], x[col], e] (DOSTransformer_phonon.py:190-197) FACTORED: the two node products
   * P = x Wa^T, Q = x Wb^T are N-row GEMMs (dosx_gemm_pair), this call multiplies the E edge rows by Wc only (K = H instead of
   * 3H) and gathers P[row(e)] + Q[col(e)] from the L2-resident [nodes, 4H] product in its epilogue. */
  const float* add_p;
  const int32_t* add_ip;
  const float* add_q;
  const int32_t* add_iq;
  int32_t ld_add;
  /* w_layout 1 with nseg > 1, optional: K-segment s of A multiplies its OWN block of W - rows restart at 0 and the block is
   * shifted by s * w_seg_off floats:  B(k, n) = w[(k - k0_s) * ldw + s * w_seg_off + n]  (0 = one [K,N] matrix as usual).
   * The node part of the factored EdgeModel input gradient, dx = [S | D] . [Wa ; Wb] with Wa = W1[:, :H], Wb = W1[:, H:2H] two
   * column blocks of ONE [2H,3H] matrix: segments S, D of width 2H, ldw = 3H, w_seg_off = H.  Needs aligned operands and
   * segment widths that are multiples of 32. */
  int32_t w_seg_off;
} DosxGemm;

/* exact number of workgroup rows dosx_gemm writes into `partials` for this epilogue: ceil(M/32) for
 * the row-wise epilogues, ceil(M/32)*ceil(N/128) for the element-wise PRELU_BWD epilogue. */
/* Experiment switch (round 4, default 0 = off; this setter is the only way to turn it on): plain dgrad GEMMs (w_layout 1, no
 * prologue / bias / activation, one segment, identity out / residual maps) of up to `gf` GFLOP run on a vector-ALU kernel whose
 * workgroups (4 waves, 56 VGPRs, 8.5 KB of LDS) fit next to two resident weight-gradient workgroups. */
int dosx_set_sliver_max_gf(double gf);
int dosx_gemm_partial_rows(int M, int N, int epi);
int dosx_gemm(const DosxGemm* g, dosx_stream_t stream);
/* Two independent GEMMs in ONE launch when they share a tile configuration (same N, W[N,K], no prologue, the plain epilogue,
 * 4-float aligned operands), one after the other otherwise - the two output heads `fc` / `fc_prompt`
 * (DOSTransformer_phonon.py:93-95,105-109; DOSTransformer.py:64-66,76-80) write disjoint rows of one tensor and are each one
 * partial round of workgroups: together still one round.  Tile height chosen for the rows of both.
 * Round 5: also two EPI_PRELU_BWD problems (W[K,N], N = 128) of different heights - the node and the edge encoder's backward at
 * the tail of a step (DOSTransformer_phonon.py:129-130,141-142 differentiated): each at ITS tile height in one grid (16-row tiles
 * for the few hundred node rows, 48-row tiles for the edge rows), partial rows numbered per problem as dosx_gemm would. */
int dosx_gemm_pair(const DosxGemm* a, const DosxGemm* b, dosx_stream_t stream);
/* diagnostic: the device symbol dosx_gemm launches for this descriptor, as a profiler prints it
 * ("gemm_kernel<RT, NTW, WL, PRO, VEC, EPI>"), written to the HOST buffer buf[n]. */
int dosx_gemm_kernel_name(const DosxGemm* g, char* buf, int n);

/* dW of y = A W^T + b (nn.Linear weight gradient), split over the M rows into `nsplit` partial sums
 *   part[s][n][k] = sum_{m in split s} dY[m][n] * prologue(A)[m][k],   bias part[s][n] = sum_m dY[m][n].
 * `nsplit` must come from dosx_wgrad_splits().  Two modes:
 *   dst == NULL (slab mode): the partial sums are left in slab[nsplit][N][K] / slab_bias[nsplit][N] for
 *     dosx_reduce_partials;
 *   dst != NULL (finished mode): the kernel itself finishes dW: every workgroup publishes its 64x64 partial tile
 *     (write-through stores), draws a ticket on its tile's counter, and the LAST arriver of a tile adds the nsplit partial
 *     tiles in split order (a fixed order whoever arrives last: bitwise reproducible, no float atomics) and writes
 *     dst[N][K] (row stride K; `accumulate`: dst +=) and dst_bias[N].  No second launch, no slab re-read through HBM.
 *     slab is then private scratch of dosx_wgrad_scratch_floats(N, K, nsplit) floats (tile-major; may be NULL when
 *     nsplit == 1), slab_bias of nsplit * 64*ceil(N/64) floats, `counters` one int32 per 64x64 tile
 *     (dosx_wgrad_tiles(N, K)), ZERO before the first launch that uses them and zero again when the launch is done
 *     (the last arriver resets its counter), so a caller allocates them zeroed once. */
typedef struct DosxWgrad {
  int32_t M, N, K;
  DosxSeg dy;        /* width = N */
  int32_t nseg;
  DosxSeg a[3];
  int32_t pro;
  const float* pro_gamma;
  const float* pro_beta;
  const float* pro_alpha;
  const float* pro_stats;
  float* slab;       /* slab mode: [nsplit, N, K]; finished mode: scratch (see above) */
  float* slab_bias;  /* slab mode: [nsplit, N] or NULL; finished mode: scratch or NULL */
  int32_t nsplit;
  int32_t accumulate; /* finished mode: dst (+)= */
  float* dst;        /* finished mode: [N, K] */
  float* dst_bias;   /* finished mode: [N] or NULL (needs slab_bias) */
  int32_t* counters; /* finished mode: [dosx_wgrad_tiles(N, K)] */
  int32_t ldd;       /* finished mode: row stride of dst in floats (0 = K: contiguous).  A column block of a wider gradient -
                        the three K-segments of the EdgeModel's first Linear are separate jobs (round 4, see
                        dosx_segment_reduce_perm) - is written in place. */
} DosxWgrad;
int dosx_wgrad_splits(int M, int N, int K);
int dosx_wgrad_tiles(int N, int K);
int64_t dosx_wgrad_scratch_floats(int N, int K, int nsplit);
int dosx_wgrad(const DosxWgrad* g, dosx_stream_t stream);
/* The same for `n_jobs` independent jobs in as few launches as possible (one grid over up to 8 jobs at a time; jobs
 * with non-affine operands get their own launch).  Results are identical to n_jobs dosx_wgrad calls. */
int dosx_wgrad_grouped(const DosxWgrad* jobs, int n_jobs, dosx_stream_t stream);

/* Batched deterministic reduction of partial slabs: dst[i] (+)= sum_s src[s*stride + i]. */
typedef struct DosxReduceJob {
  const float* src;
  float* dst;
  int32_t nsplit;
  int32_t stride;
  int32_t count;
  int32_t accumulate; /* 0: overwrite dst, 1: add to dst */
} DosxReduceJob;
/* jobs: HOST array of n_jobs entries (copied into kernel arguments, <= 64 jobs per launch: no device
 * table, no host->device copy, safe under graph capture).  Jobs of one call must have distinct dst. */
int dosx_reduce_partials(const DosxReduceJob* jobs_host, int n_jobs, dosx_stream_t stream);
/* One flush point of a backward pass in ONE launch: the weight-gradient jobs (dosx_wgrad_grouped) and the row-partial
 * reductions of the fused LayerNorm / PReLU / bias epilogues (dosx_reduce_partials; they depend on earlier kernels only,
 * not on the weight-gradient jobs) share a grid: the reduction blocks are appended behind the weight-gradient tiles.
 * Up to 8 weight-gradient + 40 reduction jobs per launch (kernel-argument table); more jobs -> more launches. */
int dosx_grad_flush(const DosxWgrad* jobs, int n_jobs, const DosxReduceJob* rjobs_host, int n_rjobs, dosx_stream_t stream);

/* a1: edge_attr[E,4] = smooth_cutoff(|v|/r_max) * [1, sqrt3 * v/max(|v|,1e-12)]
 * (DOSTransformer_phonon.py:74-77; e3nn semantics restated in oracle/dos_oracle.py). */
int dosx_edge_feat_sh1(const float* edge_vec, float* edge_attr, int E, float r_max, dosx_stream_t stream);
/* the same + the first Linear of GN_encoder.edge_encoder on it (DOSTransformer_phonon.py:129,142; K = 4) in one launch:
 *   edge_attr[E,4] as above ;  z[E,H] = edge_attr . w0^T + b0     (w0 [H,4] row-major, b0 [H]) */
int dosx_edge_embed_sh1(const float* edge_vec, const float* w0, const float* b0, float* edge_attr, float* z, int E, int H,
                        float r_max, dosx_stream_t stream);

/* a5 + a6: CSR segment reduction over destination-sorted edges (replaces torch_scatter
 * scatter_mean / scatter_sum by `col`, DOSTransformer_phonon.py:209 / DOSTransformer.py:187)
 *   agg[n]   = scale[n] * sum_{e in [rowptr[n], rowptr[n+1])} msg[e]       (scale NULL -> 1)
 *   e_out[e] = e_in[e] + msg[e]   (edge residual, DOSTransformer_phonon.py:84; skipped if e_out NULL) */
int dosx_segment_reduce(const float* msg, const int32_t* rowptr, const float* scale, float* agg,
                        const float* e_in, float* e_out, int N, int E, int H, dosx_stream_t stream);
/* The same segment sums over a PERMUTED row order: agg[n] = sum_{j in [rowptr[n], rowptr[n+1])} msg[perm[j]]  (no scale, no
 * residual).  With rowptr_src / perm_src: the sum of a per-edge tensor over the edges that LEAVE node n.  Round 4 uses the pair
 * (this, dosx_segment_reduce) to factor the weight gradient of `Linear(cat[x[row], x[col], e])` (DOSTransformer_phonon.py:
 * 190-197): sum_e dz_e (x) x[row(e)] = sum_n (sum_{e: row(e) = n} dz_e) (x) x_n - the node blocks of that gradient become
 * N-row jobs instead of E-row ones (20 x fewer rows at 20 edges per node). */
int dosx_segment_reduce_perm(const float* msg, const int32_t* rowptr, const int32_t* perm, float* agg, int N, int E, int H,
                             dosx_stream_t stream);

/* The LAST message-passing layer's second Linear on aggregated rows (round 4).  Its per-edge output feeds only the aggregation
 * (`edge_attr += out` of the last layer is dead, DOSTransformer_phonon.py:84,209 / DOSTransformer.py:59,187), and the Linear
 * commutes with the segment sum:  scale_n * sum_{e -> n} (act_e W^T + b) = S[n] W^T + R[n]  with
 *   S[n] = scale[n] * sum_{e in [rowptr[n], rowptr[n+1])} PReLU(xhat[e] * gamma + beta)     [N, W]   (W = 2 * hidden)
 *   R[n] = c_n * bias, c_n = segment length (scale == NULL: scatter_sum) or [segment not empty] (scatter_mean)   [N, Hout]
 * so an N-row dosx_gemm (res = R) replaces the E-row one; backward: dosx_gemm on N rows, dosx_ln_prelu_bwd_gather for the
 * LayerNorm -> PReLU backward of the edge rows, an N-row weight-gradient job on (dagg, S), and the bias gradient as the column
 * sum of dosx_seg_count_scale's rows  out[n] = c_n * in[n]. */
int dosx_act_segment_sum(const float* xhat, const int32_t* rowptr, const float* scale, const float* gamma, const float* beta,
                         const float* alpha, const float* bias, float* S, float* R, int N, int W, int Hout, dosx_stream_t stream);
int dosx_seg_count_scale(const float* in, int ld_in, const int32_t* rowptr, int mean, float* out, int N, int H,
                         dosx_stream_t stream);

/* backward of the aggregation + residual:  dmsg[e] = (de_new ? de_new[e] : 0) + scale[dst[e]] * dagg[dst[e]]
 * dagg has row stride ld_dagg (it is a column block of the node-MLP input gradient), de_new row stride ld_de_new
 * (it is the e-block of the next layer's [E,3H] concat gradient, or a plain [E,H] tensor). */
int dosx_edge_grad_combine(const float* de_new, int ld_de_new, const float* dagg, int ld_dagg, const int32_t* dst,
                           const float* scale, float* dmsg, int E, int H, dosx_stream_t stream);

/* backward of the two gathers x[row], x[col] (the scatter-adds of SURVEY.md §2.2) fused with
 * the node / edge residual gradients, atomic-free:
 *   dx[n]      = dx_res[n] + dnode[n, 0:H]
 *              + sum_{e in dst-seg(n)} dcat[e, H:2H] + sum_{j in src-seg(n)} dcat[perm_src[j], 0:H]
 *   de_out[e]  = (de_new ? de_new[e] : 0) + dcat[e, 2H:3H]          (skipped if de_out NULL) */
int dosx_gather_bwd(const float* dcat, const float* dnode, int ld_dnode, const float* dx_res,
                    const int32_t* rowptr_dst, const int32_t* rowptr_src, const int32_t* perm_src,
                    const float* de_new, float* dx, float* de_out, int N, int E, int H,
                    dosx_stream_t stream);

/* a7: node->graph sum pooling over contiguous node ranges (scatter_sum(x, batch),
 * DOSTransformer_phonon.py:180) and its backward (broadcast add). */
int dosx_graph_pool(const float* x, const int32_t* graph_ptr, float* out, int ld_out, int B, int H,
                    dosx_stream_t stream);
/* num_graphs > 0: nodes with node_graph[n] >= num_graphs (ghost / padding nodes) receive a zero pooled gradient and no
 * row of dpool is read for them (otherwise dpool needs a zero row at index num_graphs). */
int dosx_graph_pool_bwd(const float* dpool, int ld_dpool, const int32_t* node_graph, float* dx, int N, int H,
                        int accumulate, int num_graphs, dosx_stream_t stream);

/* a8 (+ the LN statistics of layer_norms[0] on keys): to_dense_batch + row normalisation.
 *   kvhat[dense_row[n]] = (x[n]-mean)*rstd ; rstd_nodes[n] ; all other rows of kvhat = 0
 * (to_dense_batch DOSTransformer_phonon.py:86-87; padded rows stay exact zeros so that
 *  LayerNorm gives beta on them).  kvhat must be zero-filled by the caller
 *  (dosx_fill) or pass zero_rows = total dense rows to let the kernel do it. */
int dosx_dense_normalize(const float* x, const int32_t* dense_row, float* kvhat, float* rstd_nodes,
                         int N, int H, int dense_rows, dosx_stream_t stream);
/* The same in ONE launch, driven by the dense slots instead of the nodes (no separate zero fill): slot (pos, b) holds
 * node graph_ptr[b] + pos if pos < atoms(b), else zeros; kvhat has n_max*B + 1 rows (the last one = the zero row ghost /
 * padding nodes point at).  rstd_nodes is written for the nodes of the B graphs only. */
int dosx_dense_normalize_slots(const float* x, const int32_t* graph_ptr, float* kvhat, float* rstd_nodes, int B,
                               int n_max, int H, dosx_stream_t stream);
/* backward: dx[n] (+)= rstd[n] * (g - mean(g) - xhat*mean(g*xhat)),  g = dkvhat[dense_row[n]];
 * nodes whose dense_row equals `ghost_row` (>= 0) get dx (+)= 0 without reading rstd_nodes (ghost / padding nodes). */
int dosx_dense_normalize_bwd(const float* dkvhat, const float* kvhat, const float* rstd_nodes,
                             const int32_t* dense_row, float* dx, int N, int H, int accumulate, int ghost_row,
                             dosx_stream_t stream);
/* ... with the backward of the decoder's sum pooling (scatter_sum(x, batch), DOSTransformer_phonon.py:178-181) in the same
 * launch: dx[n] (+)= [the above] + dpool[node_graph[n]]  (dpool [B, >= H] with row stride ld_dpool; nodes whose graph id is
 * >= num_graphs - ghost nodes - get no pooled term).  What dosx_dense_normalize_bwd followed by dosx_graph_pool_bwd do. */
int dosx_dense_normalize_pool_bwd(const float* dkvhat, const float* kvhat, const float* rstd_nodes,
                                  const int32_t* dense_row, const float* dpool, int ld_dpool, const int32_t* node_graph,
                                  int num_graphs, float* dx, int N, int H, int accumulate, int ghost_row,
                                  dosx_stream_t stream);

/* to_dense_batch alone (DOSTransformer_phonon.py:86-87; torch_geometric.utils.to_dense_batch with the mask dropped): dense
 * [n_max*B, H], slot (pos, b) at row pos*B + b = node graph_ptr[b] + pos, or zeros.  The keys of the UNFUSED attention
 * path (hidden > 256), which applies layer_norms[0] to them itself; and its backward: dx[n] (+)= ddense[dense_row[n]],
 * nothing for nodes whose dense_row is ghost_row (padding nodes). */
int dosx_dense_slots(const float* x, const int32_t* graph_ptr, float* dense, int B, int n_max, int H, dosx_stream_t stream);
int dosx_dense_slots_bwd(const float* ddense, const int32_t* dense_row, float* dx, int N, int H, int accumulate,
                         int ghost_row, dosx_stream_t stream);

/* xhat[e] = (v - mean(v)) * rstd(v),  v = z[e] + p[src[e]] + q[dst[e]]   (rows of W <= 1024 floats; rstd [E] saved):
 * the LayerNorm input of the EdgeModel (DOSTransformer_phonon.py:193-195) when its first Linear is FACTORED -
 * Linear(cat[x[row], x[col], e]) = (x Wa^T)[row] + (x Wb^T)[col] + e Wc^T + b: p and q are N-row products (row strides
 * ldp / ldq), z the E-row product on a third of the columns.  Used for large edge sets (functional._factor_edge). */
int dosx_gather_add_rownorm(const float* z, const float* p, int ldp, const float* q, int ldq, const int32_t* src,
                            const int32_t* dst, float* xhat, float* rstd, int E, int W, dosx_stream_t stream);

/* Row LayerNorm without affine (key/value side of self attention) and with affine. */
int dosx_rownorm(const float* x, float* xhat, float* rstd, int M, int H, dosx_stream_t stream);
int dosx_rownorm_bwd(const float* dxhat, const float* xhat, const float* rstd, float* dx, int M, int H,
                     int accumulate, dosx_stream_t stream);
/* out[r] = (res ? res[r] : 0) + a[r] o (mask ? mask[r] : 1)  (+ the LayerNorm statistics [M,2] = (mean, rstd) of the out rows
 * when `stats` is given): the "dropout -> add residual" steps of the encoder layer (layers/transformer.py:137-138,145-148)
 * for relu / res dropout > 0, with the Bernoulli draw as an explicit multiplier (dosx_dropout_mask); mask is [M,H] dense. */
int dosx_mask_residual(const float* a, int lda, const float* mask, const float* res, int ldr, float* out, int ldo,
                       float* stats, int M, int H, dosx_stream_t stream);
/* The same followed by the backward of the (Leaky)ReLU that produced the normalised rows' input y
 * (DOSTransformer_phonon.py:103,106 `F.leaky_relu(self.fc(...))` feeding the self-attention keys):
 *     out = (dx_in + rownorm_bwd(dxhat, xhat, rstd)) * (y > 0 ? 1 : slope)         one launch instead of two */
int dosx_rownorm_bwd_act(const float* dxhat, const float* xhat, const float* rstd, const float* dx_in, const float* y,
                         float slope, float* out, int M, int H, dosx_stream_t stream);
/* y = LN(x)*gamma+beta (layers/transformer.py:76-77); saves xhat, rstd. */
int dosx_layernorm(const float* x, const float* gamma, const float* beta, float* y, float* xhat, float* rstd,
                   int M, int H, dosx_stream_t stream);
/* Backward of `LayerNorm -> PReLU` on rows of W <= 1024 floats (the Edge / Node MLPs, DOSTransformer_phonon.py:193,204, when
 * 2 * hidden > 512 - narrower rows run this in the EPI_PRELU_LN_BWD epilogue of dosx_gemm): dy [M,W] is the gradient behind
 * the PReLU, xhat / rstd what the forward saved; dz [M,W] = gradient in front of the LayerNorm; partials: ceil(M/32) rows
 * of [dgamma(W) | dbeta(W) | pad(3) | dalpha]  (row stride 2W + 4). */
int dosx_ln_prelu_bwd(const float* dy, const float* xhat, const float* rstd, const float* gamma, const float* beta,
                      const float* alpha, float* dz, float* partials, int M, int W, dosx_stream_t stream);
/* The same with the gradient rows gathered and scaled: row r reads dy[idx[r]] * (scale ? scale[idx[r]] : 1) - dy holds one row per
 * destination node (see dosx_act_segment_sum). */
int dosx_ln_prelu_bwd_gather(const float* dy, const int32_t* idx, const float* scale, const float* xhat, const float* rstd,
                             const float* gamma, const float* beta, const float* alpha, float* dz, float* partials, int M, int W,
                             dosx_stream_t stream);
/* dx = LNbwd(dy); partials: ceil(M/32) rows of [dgamma(H) | dbeta(H)]   (H <= 1024) */
int dosx_layernorm_bwd(const float* dy, const float* xhat, const float* rstd, const float* gamma, float* dx,
                       float* partials, int M, int H, dosx_stream_t stream);

/* a9 + the attention half of a10: one pre-norm attention block
 *   x1 = x + softmax_fp32( LN0(x) K^T * H^-1/2 ) K ,  K = kvhat*gamma0 + beta0   (K == V)
 * (layers/transformer.py:131-138, layers/multihead_attention.py:68-74: no projections, no
 *  mask, no heads).  Query row (s, bq) is at x + (s*q_stride_s + bq*q_stride_b)*H; output
 *  row (s,bq) at s*Bq + bq; key row (j, bk) at j*Bk + bk with bk = bq % Bk.
 *  H <= 256, H % 4 == 0; ANY number of keys: up to 320 per crystal the MFMA kernels (score row of a query in LDS), more
 *  through one-wave-per-row kernels with the same results contract (csrc/attention_general.hip; they need `dscores`). */
/* BWD_*_HALF: the two-kernel form of dosx_attention_bwd (dq half: needs dout,P -> dx,dS ; dkv half: needs dS -> dkvhat) issued
 * as TWO calls - one with DOSX_ATTN_BWD_DQ_HALF, one with DOSX_ATTN_BWD_DKV_HALF, e.g. the dkv half on a second stream (only the
 * final key-gradient consumers need it).  A caller that sets one flag owes the other call: together they are the whole backward.
 * The exception: DOSX_ATTN_BWD_DQ_HALF with dkvhat == NULL is a COMPLETE call, the query-only backward for keys that come from
 * frozen parameters - dx and partials_q are the whole backward's, bit for bit, no key gradient exists and no DKV half follows;
 * dkv_part / dkv_cnt / partials_kv may be NULL, dscores too where Nk <= 64 routes to the crystal-aligned kernel. */
enum { DOSX_ATTN_RAW_Q = 1, DOSX_ATTN_NO_RESIDUAL = 2, DOSX_ATTN_BWD_DKV_HALF = 4, DOSX_ATTN_BWD_DQ_HALF = 8 };
typedef struct DosxAttn {
  int32_t Sq, Bq, Nk, Bk, H;
  int32_t q_stride_s, q_stride_b;
  int32_t flags;       /* DOSX_ATTN_RAW_Q: queries are used as given (no LN0, gamma0/beta0 still applied to
                          kvhat); DOSX_ATTN_NO_RESIDUAL: out = softmax(..)K without "+ x".  Both set =
                          the bare MultiheadAttention.forward (layers/multihead_attention.py:49-76). */
  const float* x;      /* queries / residual */
  const float* kvhat;  /* [Nk*Bk, H] normalised keys (no affine) */
  const float* gamma0;
  const float* beta0;
  float* out;          /* [Sq*Bq, H] */
  float* probs;        /* [Bq, Sq, Nk] saved softmax */
  float* qstats;       /* [Sq*Bq, 2] mean, rstd of LN0 on the query rows */
  float* out_stats;    /* optional [Sq*Bq, 2] mean, rstd of the OUTPUT rows (for the following LN1) */
  /* backward only */
  const float* dout;   /* [Sq*Bq, H] */
  float* dx;           /* [Sq*Bq, H] = dout + LN0bwd(dq) */
  float* dscores;      /* [Bq, Sq, Nk] scratch: dS */
  float* dkvhat;       /* [Nk*Bk, H] (+)= */
  int32_t dkv_accumulate;
  float* partials_q;   /* [Bq * ceil(Sq/32)] rows of [dgamma(H) | dbeta(H)] */
  float* partials_kv;  /* [Bk * ceil(Nk/32)] rows of [dgamma(H) | dbeta(H)]; [Bk * ceil(Nk/16)] rows on the dkv_part path */
  const float* drop_mask; /* optional [Bq, Sq, Nk]: attention dropout (F.dropout on the softmax output,
                          layers/multihead_attention.py:70) as an explicit multiplier M in {0, 1/(1-p)} (dosx_dropout_mask);
                          `probs` stays the un-dropped softmax.  NULL = no dropout (eval mode / p = 0) */
  float* dkv_part;     /* optional scratch [Bq * ceil(Sq/32), Nk, H]: with it (and Nk <= 64) the dq kernel also leaves each
                          query tile's share of dK + dV there and the dkv half is a small reduction over those partials
                          (no dscores round trip: dscores may then be NULL); without it the streamed dkv kernel runs */
  int32_t* dkv_cnt;    /* optional, with dkv_part: [Bk] arrival counters, zero before the launch and zero again after it.  The
                          backward is then ONE launch: the last query-tile workgroup of a key crystal to arrive (ticket)
                          sums the partial key gradients of that crystal and writes dkvhat / partials_kv itself, in the
                          reduction kernel's order (bitwise the two-launch result).  Excludes the DKV_HALF / DQ_HALF flags */
  /* forward only, optional (round 5; needs out_stats, <= 320 keys): the layer's NEXT LayerNorm applied to the output rows while
   * they are in registers - ln1_out[r] = (out[r] - mean) * rstd * ln1_gamma + ln1_beta (layers/transformer.py:141: the input of
   * fc1) - so that the fc1 GEMM of a layer whose feed-forward half is not fused reads a plain A operand instead of normalising
   * it in its prologue for every one of its column tiles (hidden 256, M = 25728: 163 -> 139 us) */
  const float* ln1_gamma;
  const float* ln1_beta;
  float* ln1_out;      /* [Sq*Bq, H] */
  /* Per-crystal key counts, forward and backward, every kernel form, any Nk.  key_ptr [Bk + 1] (NULL: every crystal attends
   * over all Nk key rows - padded rows included, like the reference's unmasked to_dense_batch): key crystal bk = bq % Bk has
   * n = clamp(key_ptr[bk + 1] - key_ptr[bk], 0, Nk) keys (the batch's graph_ptr: its own atoms); the rows j >= n do not exist.
   * A batch of B crystals then computes what B batch-size-1 passes compute - the reference trains and evaluates the phonon
   * model and evaluates the Electron-DOS model at batch_size = 1 (main_phDOS.py:52-55, main_eDOS.py:55-56).  The float64
   * contract (DosxAttn64.key_ptr) in fp32:
   *   - nothing at key index >= n is read from kvhat, probs, drop_mask or dscores;
   *   - probs and dscores (when given) are written 0.0 at key index >= n;
   *   - the key-side partial rows (partials_kv) of key tiles past n are written 0.0: column sums need no mask;
   *   - dkvhat rows >= n are written 0.0 without dkv_accumulate and left alone with it;
   *   - n = 0: out = x (forward), dx = dout (backward, with the residual), zero key gradients, no division by zero;
   *   - key_ptr = [0, Nk, 2 Nk, ...] gives bitwise what NULL gives. */
  const int32_t* key_ptr;
} DosxAttn;
/* 1 if dosx_attention_bwd takes the partial-dKV path for this key count / width when dkv_part is given (else it needs
 * dscores and runs the streamed dkv kernel) */
int dosx_attention_pkv_supported(int Nk, int H);
/* Which shapes dosx_attention_fwd / dosx_attention_bwd (one-launch form: dkv_part + dkv_cnt) route to the crystal-aligned
 * kernels (csrc/attention_aligned.hip: flags 0, Nk <= 64, H in {64, 128, 256}): 0 = none (attention.hip's kernels), 1 = H > 128
 * only, 2 = all of them (the default).  Sets the mode unless `mode` < 0;
 * returns the previous one. */
int dosx_attention_aligned_mode(int mode);
int dosx_attention_fwd(const DosxAttn* a, dosx_stream_t stream);
int dosx_attention_bwd(const DosxAttn* a, dosx_stream_t stream);

/* Attention with K != V (`multihead_attention.py:49-76` takes any key / value pair; embed dropout, `transformer.py:61-68`,
 * draws different masks for keys and values).  No reference call site does that, so the MFMA kernels above are built for
 * K = V; the general case is composed from them and these building blocks (csrc/attention_kv.hip: one wave per output row,
 * deterministic, not a hot path).  A / mask / dP: [Bq, Sq, Nk]; X, out rows (s, bq) at s*Bq + bq; V rows (j, bk) at j*Bk + bk:
 *   dosx_attn_pv:     out[(s,bq)] = sum_j (A o mask)[bq,s,j] V[(j, bq % Bk)]                 (P.V, and dQ = dS.K)
 *   dosx_attn_tv:     out[(j,bk)] (+)= sum_{bq = bk mod Bk} sum_s (A o mask)[bq,s,j] X[(s,bq)]   (dV = P^T dOut, dK = dS^T Q)
 *   dosx_attn_dp:     dP[bq,s,j] = X[(s,bq)] . V[(j, bq % Bk)]
 *   dosx_softmax_bwd: dS = scale * P o (dPd o mask - rowsum(dPd o mask o P))                   (rows = Bq*Sq)
 *   dosx_softmax_fwd: P = softmax_fp32(scale * S) row by row - with S from dosx_attn_dp(Q, K) the attention weights for ANY
 *                     number of keys and any H % 4 == 0 (dosx_attention_fwd: H <= 256) */
int dosx_attn_pv(const float* A, const float* mask, const float* V, float* out, int Sq, int Bq, int Nk, int Bk, int H,
                 dosx_stream_t stream);
int dosx_attn_tv(const float* A, const float* mask, const float* X, float* out, int Sq, int Bq, int Nk, int Bk, int H,
                 int accumulate, dosx_stream_t stream);
int dosx_attn_dp(const float* X, const float* V, float* dP, int Sq, int Bq, int Nk, int Bk, int H, dosx_stream_t stream);
int dosx_softmax_bwd(const float* P, const float* mask, const float* dPd, float* dS, long long rows, int Nk, float scale,
                     dosx_stream_t stream);
int dosx_softmax_fwd(const float* S, float* P, long long rows, int Nk, float scale, dosx_stream_t stream);

/* out_layer (nn.Linear(H,1), DOSTransformer_phonon.py:101,115) fused with the encoder's final
 * LayerNorm (layers/transformer.py:76-77) and the squeeze/transposed store:
 *   y[r] = (xhat[r]*gamma+beta) . w + b ;  dos[(r % Bq) , r / Bq] = y[r]   (dos is [Bq, S]) */
int dosx_ln_rowdot(const float* x, const float* gamma, const float* beta, const float* w, const float* b,
                   float* xhat, float* rstd, float* dos, int S, int Bq, int H, dosx_stream_t stream);
/* ddos [Bq,S] -> dx [S*Bq,H]; partials: ceil(M/32) rows of [dgamma(H) | dbeta(H) | dw(H) | db] */
int dosx_ln_rowdot_bwd(const float* ddos, const float* xhat, const float* rstd, const float* gamma,
                       const float* beta, const float* w, float* dx, float* partials, int S, int Bq, int H,
                       dosx_stream_t stream);
/* plain y[r] = act(x[r]) . w + b for the GNN-only variants' last layer (graphnetwork_phonon.py:26,70) */
int dosx_rowdot(const float* x, const float* w, const float* b, float* dos, int S, int Bq, int H,
                dosx_stream_t stream);
int dosx_rowdot_bwd(const float* ddos, const float* x, const float* w, float* dx, float* partials, int S,
                    int Bq, int H, dosx_stream_t stream);

/* a14: losses of the callers, forward + gradient in one pass.
 * phonon (main_phDOS.py:109-114): loss = sqrt(mean_all (pg-y)^2) + beta*sqrt(mean_all (ps-y)^2)
 *   two-phase so that data-parallel ranks can all-reduce the two SSE scalars in between:
 *   dosx_sse2 writes sse[0..1]; dosx_loss_phonon_bwd consumes (possibly all-reduced) sse and
 *   `count` = global number of elements.
 * eDOS (main_eDOS.py:111-123): loss = mean_b rmse_b(global) + beta * mean_b rmse_b(system),
 *   target clamped at 0; `B_global` = number of crystals in the un-sharded batch.
 * ONE-OUTPUT callers (the GNN-only baselines: main_phDOS.py:109-111 / main_eDOS.py:111-118 with their single DOS output) use the
 *   same entries: ps = pg (inputs may alias: they are only read), beta = 0, dps = scratch of the same size (distinct from dpg).
 *   Then loss = rmse(pg) + 0 * rmse(pg) = the one-output loss EXACTLY (every rmse is finite), dpg is its gradient, and dps
 *   receives 0 (or NaN where the rmse is 0: 0/0 - scratch, never read).  That is within the contract above; nothing here
 *   depends on beta != 0 or on pg != ps. */
int dosx_sse2(const float* pg, const float* ps, const float* y, float* sse, int count, dosx_stream_t stream);
int dosx_loss_phonon_bwd(const float* pg, const float* ps, const float* y, const float* sse, float beta,
                         double count_global, float* dpg, float* dps, float* loss, int count,
                         dosx_stream_t stream);
/* single-process form: dosx_sse2 + dosx_loss_phonon_bwd in one launch (count = all B*S elements; sse may be NULL) */
int dosx_loss_phonon(const float* pg, const float* ps, const float* y, float* sse, float beta, float* dpg, float* dps,
                     float* loss, int count, dosx_stream_t stream);
int dosx_loss_edos(const float* pg, const float* ps, const float* y_ft, float beta, int B, int S, int B_global,
                   float* dpg, float* dps, float* loss_partial, dosx_stream_t stream);

/* dst[0] = sum_i src[i]: the mean over crystals of the eDOS loss (main_eDOS.py:117,121) from the
 * per-crystal shares written by dosx_loss_edos. */
int dosx_sum(const float* src, int n, float* dst, dosx_stream_t stream);

/* torch.optim.AdamW step on a flat buffer (main_eDOS.py:93,127): decoupled weight decay (csrc/adamw.hip).
 * `step` is the 1-based step count. */
int dosx_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
               float eps, float weight_decay, int step, float grad_scale, dosx_stream_t stream);

/* Fused feed-forward half of the encoder layer (layers/transformer.py:141-148), forward:
 *     h   = relu( LN1(x) . W1^T + b1 )      [M,4H]   (written out: the backward needs it)
 *     out = x + h . W2^T + b2               [M,H]
 * LN1(x) = (x - mean)*rstd*gamma + beta with the per-row (mean, rstd) pairs in `stats` (produced by the attention
 * kernel's epilogue).  One launch instead of two GEMMs; dosx_ffn_supported(H) says whether this H has the fused kernel
 * (H % 32 == 0, H <= 128), otherwise the caller issues the two dosx_gemm calls. */
typedef struct DosxFfn {
  int32_t M, H;
  const float* x; int32_t ldx;
  const float* stats;
  const float* gamma; const float* beta;
  const float* w1; const float* b1;       /* fc1.weight [4H,H], fc1.bias [4H] */
  const float* w2; const float* b2;       /* fc2.weight [H,4H], fc2.bias [H]  */
  float* h; int32_t ldh;
  float* out; int32_t ldo;
  /* optional: the encoder's final LayerNorm (layers/transformer.py:76-77) applied to the result of the LAST layer in
   * the same launch: with fin_gamma != NULL, `out` receives LN(x + ffn)*gamma + beta, fin_xhat [M,H] (row stride H) the
   * normalised rows and fin_rstd [M] their 1/sigma (what dosx_layernorm would have produced from the un-normalised sum) */
  const float* fin_gamma; const float* fin_beta;
  float* fin_xhat; float* fin_rstd;
  /* optional, with the final LayerNorm: the H -> 1 output layer of the model head on the normalised rows
   * (DOSTransformer_phonon.py:116-117), dos[r % Bq][r / Bq] = LN(..)[r] . fin_w + fin_b[0] for the [S, Bq] row space
   * (fin_dos [Bq, S]; what dosx_ln_rowdot computes as a launch of its own); `out` may then be NULL */
  const float* fin_w; const float* fin_b; float* fin_dos;
  int32_t fin_S, fin_Bq;
  /* optional (round 4): the ATTENTION half of the layer in front of the feed-forward half, for key sets of at most 16 rows
   * per crystal (the prompt-guided cross attention over the atoms of a crystal, layers/transformer.py:131-138 +
   * multihead_attention.py:68-74) - one launch per encoder layer instead of dosx_attention_fwd + dosx_ffn_fwd.  With
   * att_kvhat != NULL:  `x` is the layer INPUT (the query rows: row r = s*att_Bq + bq at x + (s*att_qs + bq*att_qb)*ldx),
   * `stats` is ignored, and per row   q = LN0(x)*g0+b0,  P = softmax_fp32(q . (khat_j*g0+b0) / sqrt(H)) over the att_Nk keys
   * khat_j = att_kvhat[j*att_Bk + bq % att_Bk] (pre-normalised keys, dosx_dense_normalize_slots),  x1 = x + (P o mask) . K
   * is what the feed-forward half then reads.  Outputs, in the formats dosx_attention_fwd writes (its backward reads them):
   * att_probs [Bq,Sq,Nk] (un-dropped P), att_qstats [M,2] (mean, rstd of the query rows), att_x1 [M,H] (row stride
   * att_ldx1), att_st1 [M,2] (LayerNorm-1 statistics of x1).  att_mask: NULL or the dropout multipliers [Bq,Sq,Nk]. */
  const float* att_kvhat; const float* att_gamma0; const float* att_beta0; const float* att_mask;
  float* att_probs; float* att_qstats; float* att_x1; float* att_st1;
  int32_t att_Nk, att_Bk, att_Bq, att_Sq, att_qs, att_qb, att_ldx1;
  /* att_aligned != 0: CRYSTAL-ALIGNED tiles - a workgroup owns consecutive query rows s of ONE query batch entry (grid =
   * att_Bq x ceil(att_Sq / rows per workgroup)), the crystal's key rows are staged in LDS once per workgroup: up to 64 keys
   * (dosx_ffn_att_aligned_supported), e.g. the 51-key self attention over the energy bins; same outputs.  The caller chooses
   * it while that grid is about one round of workgroups: Sq is padded to the tile height per crystal. */
  int32_t att_aligned;
  const int32_t* att_key_ptr;   /* as DosxAttn.key_ptr: per-crystal key counts of the fused attention half */
} DosxFfn;
int dosx_ffn_supported(int H);
int dosx_ffn_att_supported(int H, int Nk);   /* whether dosx_ffn_fwd takes the att_* fields for this shape (H, Nk <= 16) */
int dosx_ffn_att_aligned_supported(int H, int Nk);   /* ... with att_aligned (Nk <= 64 and the key rows fit the stage buffers) */
int dosx_ffn_fwd(const DosxFfn* a, dosx_stream_t stream);
/* n <= 2 consecutive layers of ONE encoder stack (layers/transformer.py:70-79) in one launch (round 6): with the attention half inside the
 * launch a layer is row-local per tile - every layer attends over the ORIGINAL keys (transformer.py:72-73) - so a workgroup runs the
 * layers back to back on its own rows.  descs[l + 1].x must be descs[l].out (dense query rows), every descriptor carries att_*, all
 * share one launch plan (same M, H, tile form); same outputs as n dosx_ffn_fwd calls, bitwise. */
int dosx_ffn_fwd_multi(const DosxFfn* descs, int n, dosx_stream_t stream);

/* Backward of the same half layer in one launch (what autograd derives from layers/transformer.py:141-148):
 *     dh = (dy . W2) o [h > 0]            [M,4H]  (written out: the fc1 weight gradient reads it)
 *     dx = dy + LN1_bwd(dh . W1)          [M,H]   (dy also flows through the residual connection)
 *     partials[r] = [ dgamma | dbeta ] of LN1 summed over the rows of workgroup r (dosx_ffn_bwd_partial_rows(M) rows,
 *                   reduced by dosx_reduce_partials like every other slab)
 * Same H support as the forward (dosx_ffn_supported).  The weight / bias gradients of fc1 and fc2 stay dosx_wgrad calls. */
typedef struct DosxFfnBwd {
  int32_t M, H;
  const float* dy; int32_t lddy;
  const float* h; int32_t ldh;            /* relu(fc1(LN1 x)) saved by the forward */
  const float* x; int32_t ldx;            /* input of the half layer (pre-LN1) */
  const float* stats;                     /* (mean, rstd) per row of x */
  const float* gamma;                     /* LN1 weight */
  const float* w1; const float* w2;       /* fc1.weight [4H,H], fc2.weight [H,4H] */
  float* dh; int32_t lddh;
  float* dx; int32_t lddx;
  float* partials; int32_t partial_ld;
  /* optional: the backward of the encoder's final LayerNorm (layers/transformer.py:76-77) in front of the LAST layer's
   * half, same launch.  With fin_gamma != NULL, `dy` is the gradient w.r.t. that LayerNorm's OUTPUT; the kernel computes
   * dy' = LN_bwd(dy) from fin_xhat [M,H] (row stride H) / fin_rstd [M] (what the forward's fin_* outputs hold), writes
   * it to fin_dy [M,H] (row stride lddy: the fc2 weight gradient reads it), continues with dy', and appends
   * [ dgamma | dbeta ] of that LayerNorm to every partial row (columns [2H,4H): partial_ld >= 4H). */
  const float* fin_gamma; const float* fin_xhat; const float* fin_rstd;
  float* fin_dy;
  /* ... and, in front of that LayerNorm, the H -> 1 output layer of the model head (DOSTransformer_phonon.py:116-117
   * `out_layer(LN(h))`): with fin_ddos != NULL (then `dy` may be NULL) the rows are  dy[r] = ddos[r % Bq][r / Bq] * w  for
   * the [S, Bq] row space of the encoder and ddos [Bq, S]; the partial rows get [ dw (H) | db ] behind the LayerNorm's two
   * groups (columns [4H, 5H] : partial_ld >= 5H + 1).  What dosx_ln_rowdot_bwd computes as a launch of its own. */
  const float* fin_ddos; const float* fin_w; const float* fin_beta;
  int32_t fin_S, fin_Bq;
  /* optional (round 5; att_kvhat != NULL): the ATTENTION half's backward of the same encoder layer behind the feed-forward
   * half's, same launch (layers/transformer.py:131-138 + layers/multihead_attention.py:68-74 differentiated) - what
   * dosx_attention_bwd's one-launch form computes from `dx` as its `dout`, which then never reaches HBM (`dx` may be NULL).
   * Crystal-aligned tiles: a workgroup owns consecutive query rows s of ONE query batch entry (row r = s * att_Bq + bq; grid =
   * att_Bq x ceil(att_Sq / rows per workgroup) = dosx_ffn_att_bwd_partial_rows workgroups and partial rows).
   *   att_x [rows, att_ldxin]: the LAYER input (row (s, bq) at s * att_qs + bq * att_qb); att_qstats / att_probs / att_mask: saved
   *   by the forward; att_kvhat [Nk * Bk, H]: the pre-normalised keys; att_dxin [M, att_lddxin]: gradient w.r.t. the layer input;
   *   att_partials_q [Bq * tiles, 2H], att_partials_kv [Bk * ceil(Nk / 16), 2H], att_dkv_part [Bq * tiles * Nk, H] scratch,
   *   att_dkv_cnt [Bk] arrival counters (zero before and after), att_dkvhat (+)= the key gradient (att_dkv_accumulate)
   * - the fields of DosxAttn with the same names, same layouts (32-query tiles), same summation orders.
   *   att_dkvhat == NULL selects the QUERY-ONLY form, for keys that come from frozen parameters: no key gradient is computed,
   *   att_dkv_part / att_dkv_cnt / att_partials_kv are not touched and may be NULL too; dh, att_dxin, every column of `partials`
   *   and att_partials_q are bitwise the full form's. */
  const float* att_x; int32_t att_ldxin;
  const float* att_kvhat; const float* att_gamma0; const float* att_beta0;
  const float* att_probs; const float* att_qstats; const float* att_mask;
  float* att_dxin; int32_t att_lddxin;
  float* att_partials_q; float* att_partials_kv; float* att_dkv_part; int32_t* att_dkv_cnt;
  float* att_dkvhat; int32_t att_dkv_accumulate;
  int32_t att_Nk, att_Bk, att_Bq, att_Sq, att_qs, att_qb;
  const int32_t* att_key_ptr;   /* as DosxAttn.key_ptr: per-crystal key counts of the fused attention half's backward, or NULL */
} DosxFfnBwd;
int dosx_ffn_bwd_partial_rows(int M);
int dosx_ffn_att_bwd_supported(int H, int Nk, int Sq, int Bq);   /* whether dosx_ffn_bwd takes the att_* fields for this shape */
int dosx_ffn_att_bwd_partial_rows(int Sq, int Bq);               /* workgroups = partial rows of such a launch */
int dosx_ffn_att_aligned_rows(int Sq, int Bq);                   /* rows per workgroup (16 / 32) of a crystal-aligned launch, fwd and bwd */
int dosx_ffn_bwd(const DosxFfnBwd* a, dosx_stream_t stream);

/* The phonon EDGE ENCODER in one launch (round 6; csrc/heads.hip): attr = SH(l <= 1)(vec) * smooth_cutoff(|vec| / r_max)
 * (DOSTransformer_phonon.py:74-77; [E,4]), z = attr . w0^T + b0 ([E,H]: the saved pre-activation), out = prelu(z) . w2^T + b2
 * (GN_encoder.edge_encoder, :129,142).  What dosx_edge_embed_sh1 + dosx_gemm (PReLU prologue) compute; hidden 64 / 128. */
typedef struct DosxEdgeEnc {
  int32_t E, H;
  const float* vec;                         /* [E,3] */
  float inv_rmax;
  const float* w0; const float* b0;         /* [H,4], [H] */
  const float* alpha;
  const float* w2; const float* b2;         /* [H,H], [H] */
  float* attr; float* z;                    /* [E,4], [E,H] OUT */
  float* out; int32_t ldo;                  /* [E,H] OUT */
} DosxEdgeEnc;
int dosx_edge_enc_supported(int H);
int dosx_edge_enc_fwd(const DosxEdgeEnc* a, dosx_stream_t stream);

/* The backward of the two output heads (DOSTransformer_phonon.py:93-109, DOSTransformer.py:67-83: `fc`, `fc_prompt`, F.leaky_relu)
 * between the self encoder's and the first encoder's backward, in ONE launch (round 6; csrc/heads.hip):
 *     dpre[(s, bq)] = ( ddosin + rownorm_bwd(dkvs, kvs, rstd) )[(s, bq)] * leaky_relu'(dosin[(s, bq)])       rows (s, bq) at s * 2B + bq
 *     de1[(s, b)]   = dpre[(s, b)] . wg[:, :H] + dpre[(s, B + b)] . ws[:, :H]                                rows (s, b) at s * B + b
 * wg = fc.weight [H, ldwg], ws = fc_prompt.weight [H, ldws] (nn.Linear layout: only their first H columns - the E1 inputs - are
 * read).  What dosx_rownorm_bwd_act followed by two dosx_gemm calls (w_layout 1, row-mapped A) compute; hidden 64 / 128 / 256. */
typedef struct DosxHeadsBwd {
  int32_t S, B, H;
  const float* dkvs; const float* kvs; const float* rstd;     /* [S*2B, H], [S*2B, H], [S*2B] */
  const float* ddosin; const float* dosin;                    /* [S*2B, H] */
  float slope;                                                /* leaky_relu negative slope (0.01) */
  float* dpre;                                                /* [S*2B, H] OUT */
  const float* wg; int32_t ldwg; const float* ws; int32_t ldws;
  float* de1; int32_t ldde1;                                  /* [S*B, H] OUT */
} DosxHeadsBwd;
int dosx_heads_bwd_supported(int H);
int dosx_heads_bwd(const DosxHeadsBwd* a, dosx_stream_t stream);

/* The output head of the GNN-only baselines (graphnetwork_phonon.py:26,66-70, graphnetwork.py:22,38-42, mlp.py:20,30-34) on its rank
 * structure (csrc/pair_head.hip).  The head's input row (s, b) is cat[emb[s] | graph[b]], so its first Linear is e1[s] + c[b] with
 * e1 = emb . W0[:, :H]^T + b0 and c = graph . W0[:, H:]^T (two small dosx_gemm calls); then, one launch each:
 *   dosx_pair_head_fwd:  dos[b, s] = b2[0] + sum_h w2[h] * leaky(e1[s, h] + c[b, h])              leaky(p) = p > 0 ? p : slope * p
 *   dosx_pair_head_bwd:  gate = e1[s, h] + c[b, h] > 0 ? 1 : slope                                (torch's rule: 0 takes slope)
 *                        de1[s, h] = w2[h] * sum_b ddos[b, s] * gate      dc[b, h] = w2[h] * sum_s ddos[b, s] * gate
 *                        partials[s] = [ sum_b ddos[b, s] * leaky(e1[s, :] + c[b, :])  (H)  |  sum_b ddos[b, s] ]
 *     - dosx_pair_head_partial_rows(S, B) (= S) rows of H + 1 floats whose column sums are dw2 and db2 (dosx_reduce_partials).
 * No tensor of S * B * H elements is read or written.  Every sum is one thread's sequential chain (dc: four of them added in a
 * fixed order): no float atomics, two launches on the same operands give the same bits.  e1, c, de1, dc are contiguous rows of H
 * floats, 16-byte aligned like w2; dos and ddos are [B, S] row-major.  H % 8 == 0, H <= 512, any S, B >= 1 with S * B * H < 2^31;
 * anything else is refused with -22.  The forward reads e1, c, w2, b2 and writes dos; the backward reads e1, c, w2, ddos and
 * writes de1, dc, partials; the other side's fields may be NULL. */
typedef struct DosxPairHead {
  int32_t S, B, H;
  float slope;                                                /* leaky_relu negative slope (0.01) */
  const float* e1; const float* c;                            /* [S, H], [B, H] */
  const float* w2; const float* b2;                           /* [H], [1] */
  float* dos;                                                 /* [B, S] OUT (forward) */
  const float* ddos;                                          /* [B, S] (backward) */
  float* de1; float* dc;                                      /* [S, H], [B, H] OUT (backward) */
  float* partials;                                            /* [S, H + 1] OUT (backward) */
} DosxPairHead;
int dosx_pair_head_partial_rows(int S, int B);
int dosx_pair_head_fwd(const DosxPairHead* a, dosx_stream_t stream);
int dosx_pair_head_bwd(const DosxPairHead* a, dosx_stream_t stream);

/* The float64 twin (csrc/pair_head_f64.hip), for the float64 program of Graphnetwork_phonon (functional64, factored_head): the
 * contract above in double, e1 and c from two dosx_gemm_f64 calls, partials [dosx_pair_head_partial_rows(S, B), H + 1] doubles
 * whose column sums (dosx_colsum_f64, ld = H + 1) are dw2 and db2.  Every sum is one thread's sequential chain, plus a fixed
 * 16-lane tree in the forward and the fixed four-term sum of dc: no atomics, the same bits on every run.  e1, c, w2, de1, dc are
 * 16-byte aligned rows of H doubles; H % 8 == 0, H <= 512, S, B >= 1, S * B * H < 2^31; anything else is refused with -22. */
typedef struct DosxPairHead64 {
  int32_t S, B, H;
  double slope;                                               /* leaky_relu negative slope (0.01) */
  const double* e1; const double* c;                          /* [S, H], [B, H] */
  const double* w2; const double* b2;                         /* [H], [1] */
  double* dos;                                                /* [B, S] OUT (forward) */
  const double* ddos;                                         /* [B, S] (backward) */
  double* de1; double* dc;                                    /* [S, H], [B, H] OUT (backward) */
  double* partials;                                           /* [S, H + 1] OUT (backward) */
} DosxPairHead64;
int dosx_pair_head_fwd_f64(const DosxPairHead64* a, dosx_stream_t stream);
int dosx_pair_head_bwd_f64(const DosxPairHead64* a, dosx_stream_t stream);

/* Split-bf16 GEMM (round 6, csrc/gemm_bf16x3.hip) - OPT-IN: with DOSX_FFN_BF16X3=1 functional.encoder_fwd / encoder_bwd run the
 * plain feed-forward GEMMs through it; by default every program runs dosx_gemm's exact-fp32 kernels:
 *     C[M,N] = epi( A[M,K] . op(W) + bias[N] )      w_layout 0: W is [N][K] (nn.Linear), 1: W is [K][N]
 *     epi: relu (act = 1), then + res[M,N] (optional), then zero where mask[M,N] <= 0 (optional: dosx_gemm's EPI_RELU_MASK)
 * fp32 operands and result; every element is split into three bf16 terms on the fly and the six leading products run on the
 * bf16 matrix pipe with fp32 accumulation (error of the size of one fp32 rounding per product; tests hold it to dosx_gemm's
 * tolerance against float64).  N % 128 == 0, K % 32 == 0, 16-byte aligned operands, leading dimensions multiples of 4.
 * bench.py reports it as `secondary.split_bf16` for the two largest Electron-DOS GEMM shapes (no reference counterpart: the
 * reference computes in fp32 / fp64, main_phDOS.py:15-16). */
int dosx_gemm_bf16x3_supported(int M, int N, int K);
int dosx_gemm_bf16x3(const float* A, int lda, const float* W, int ldw, int w_layout, const float* bias, float* C, int ldc,
                     int M, int N, int K, int act, const float* res, int ldres, const float* mask, int ldmask,
                     dosx_stream_t stream);

/* Linear -> LayerNorm -> PReLU -> Linear (+ residual) in ONE launch for small row counts: the NodeModel MLP of a GNN layer
 * (DOSTransformer_phonon.py:200-212 `node_mlp_2(cat[x, agg])`, DOSTransformer.py:178-190).
 *     z    = [a0 | a1] . W1^T + b1                  [M,NH]     (a0: k0 columns, a1: K - k0 columns, plain row-major)
 *     xhat = (z - mean) * rstd   (eps 1e-5)         written out with rstd: the backward and dosx_wgrad read them
 *     out  = prelu(xhat*gamma + beta) . W2^T + b2 (+ res)      [M,NO]
 * What two dosx_gemm calls (EPI_LN, then PRO_LN_PRELU) compute, for the shapes dosx_mlp_ln_supported accepts
 * (K, NH multiples of 128 up to 512; NO a multiple of 64 up to 256, NO <= K); 16 rows per workgroup, so meant for
 * M of a few thousand rows at most - the caller keeps the two-GEMM path for long inputs. */
typedef struct DosxMlpLn {
  int32_t M, K, NH, NO, k0;
  const float* a0; int32_t lda0;
  const float* a1; int32_t lda1;          /* may be NULL when k0 == K */
  const float* w1; const float* b1;       /* [NH,K], [NH]  (nn.Linear layout) */
  const float* gamma; const float* beta;  /* LayerNorm(NH) */
  const float* alpha;                     /* PReLU (1 parameter) */
  const float* w2; const float* b2;       /* [NO,NH], [NO] */
  const float* res; int32_t ldres;        /* optional residual added to the output (NULL: none) */
  float* xhat; float* rstd;               /* [M,NH] (row stride NH), [M] */
  float* out; int32_t ldo;
  /* optional third product on the finished output rows (round 5: the NEXT message-passing layer's node products of the
   * factored EdgeModel Linear, DosxGemm.add_p / add_q - the dosx_gemm_pair launch between two layers):
   *     pq[r, b * n3 + n] = sum_k out[r, k] * w3[n * ldw3 + b * NO + k]      b < nb3, n < n3 (a multiple of 256)
   * NULL w3: none */
  const float* w3; int32_t ldw3, n3, nb3;
  float* pq; int32_t ldpq;
  /* round 6 - COLUMN-SPLIT form (cs_buf != NULL; shapes of dosx_mlp_ln_cs_supported: the NodeModel (K, NH, NO) = (2, 2, 1) x
   * hidden, hidden 64 / 128): a 16-row tile is shared by hidden / 16 workgroups of 4 waves, each owning 32 columns of the first
   * product and 16 of the second (1 / 8 of the weights and of the MFMAs at hidden 128) - 232 workgroups instead of 29 for the 450
   * node rows of the benchmark batch; the siblings exchange the pre-LayerNorm tile (and, with w3, the output tile) IN the launch:
   * publish with write-through stores, one ticket each on the tile's counter, every sibling waits for all tickets and reads the
   * tile back (csrc/mlp2.hip).  cs_buf: dosx_mlp_ln_cs_scratch_floats(M, NH) floats of scratch; cs_cnt: dosx_mlp_ln_cs_tiles(M)
   * arrival counters, zero before and after the launch.  Same outputs as the one-workgroup-per-tile form to fp32 rounding
   * (k-split sums added in wave order: bitwise reproducible run to run). */
  float* cs_buf; int32_t* cs_cnt;
} DosxMlpLn;
int dosx_mlp_ln_supported(int K, int NH, int NO);
int dosx_mlp_ln_cs_supported(int K, int NH, int NO);      /* whether the column-split form exists for this block shape */
int dosx_mlp_ln_cs_tiles(int M);                          /* counters it needs (= 16-row tiles) */
int64_t dosx_mlp_ln_cs_scratch_floats(int M, int NH);     /* floats of cs_buf */
int dosx_mlp_ln_fwd(const DosxMlpLn* a, dosx_stream_t stream);

/* The node ENCODER + the first message-passing layer's node products in ONE column-split launch (round 6; csrc/mlp2.hip):
 *     z   = x . W0^T + b0            [M,H]  written (the saved pre-activation: the backward reads it)        x [M,Fa], W0 [H,Fa]
 *     out = prelu(z) . W2^T + b2     [M,H]  (DOSTransformer_phonon.py:129,141: Linear -> PReLU -> Linear)
 *     pq[r, b * n3 + n] = sum_k out[r, k] * w3[n * ldw3 + b * H + k]      b < nb3, nb3 * n3 == 4H (DosxMlpLn.w3)
 * What two dosx_gemm calls and dosx_gemm_pair compute; hidden 64 / 128, even Fa <= 256; cs_cnt: dosx_mlp_ln_cs_tiles(M) counters. */
typedef struct DosxEncCs {
  int32_t M, Fa, H;
  const float* x; int32_t ldx;
  const float* w0; int32_t ldw0; const float* b0;
  const float* alpha;
  const float* w2; const float* b2;
  float* z; float* out; int32_t ldo;
  const float* w3; int32_t ldw3, n3, nb3;
  float* pq; int32_t ldpq;
  int32_t* cs_cnt;
} DosxEncCs;
int dosx_enc_cs_supported(int Fa, int H);
int dosx_enc_cs_fwd(const DosxEncCs* a, dosx_stream_t stream);

/* Backward of the same block in one launch:
 *     da = dy . W2 ; dy' = da o prelu'(xhat*gamma+beta) ; dz = LayerNorm_bwd(dy' o gamma)  [M,NH] (written: the W1 weight
 *     gradient reads it) ; dcat = dz . W1  [M,K]
 *     partials[r] = [ dgamma (NH) | dbeta (NH) | pad | dalpha ] summed over the rows of workgroup r — the layout of
 *     DOSX_EPI_PRELU_LN_BWD (dalpha in column partial_ld - 1), dosx_mlp_ln_bwd_partial_rows(M) rows.
 * The weight / bias gradients of the two Linear layers stay dosx_wgrad calls. */
typedef struct DosxMlpLnBwd {
  int32_t M, K, NH, NO;
  const float* dy; int32_t lddy;
  const float* xhat; const float* rstd;   /* saved by the forward */
  const float* w1; const float* w2;
  const float* gamma; const float* beta; const float* alpha;
  float* dz;                              /* [M,NH], row stride NH */
  float* dcat; int32_t lddcat;            /* [M,K] */
  float* partials; int32_t partial_ld;
  int32_t add_dy;                         /* 1: dcat[:, :NO] += dy - the block's residual connection out = res + MLP(cat[res, .])
                                             (NodeModel, DOSTransformer_phonon.py:204-212 + :83) differentiated in the same launch */
  float* cs_buf; int32_t* cs_cnt;         /* column-split form (see DosxMlpLn): the siblings exchange the `da` tile; same sizes */
  /* round 6, column-split form only: what PRODUCES dy, in the same launch - the N-row launch that used to run in front of it.
   *   pre = 1: the node side of the LATER message-passing layer's factored input gradient (DosxNodeGrad: pre_dz [E,2H] that
   *            layer's dz, pre_rowptr_src / pre_perm_src the CSR by source, pre_aggd [M,2H], pre_w [2H, >= 2H] row stride pre_ldw,
   *            pre_res / pre_res2 optional [M,H] addends, pre_aggs [M,2H] OUT): dy = pre_res + pre_res2 + aggs Wa + aggd Wb;
   *   pre = 2: dosx_dense_normalize_pool_bwd (pre_dkv / pre_kvhat dense [*,H], pre_rstd_nodes [M], pre_dense_row [M], pre_dpool
   *            [graphs, pre_ld_dpool], pre_node_graph [M], pre_num_graphs, pre_ghost_row; no accumulation): dy = its dx.
   * dy is then an OUTPUT (pre_dy = the same pointer, writable; [M,H], row stride lddy): the weight-gradient jobs read it. */
  int32_t pre;
  float* pre_dy;
  const float* pre_dz; const int32_t* pre_rowptr_src; const int32_t* pre_perm_src; const float* pre_aggd;
  const float* pre_w; int32_t pre_ldw;
  const float* pre_res; int32_t pre_ldres; const float* pre_res2; int32_t pre_ldres2;
  float* pre_aggs;
  const float* pre_dkv; const float* pre_kvhat; const float* pre_rstd_nodes; const int32_t* pre_dense_row;
  const float* pre_dpool; int32_t pre_ld_dpool; const int32_t* pre_node_graph; int32_t pre_num_graphs, pre_ghost_row;
} DosxMlpLnBwd;
int dosx_mlp_ln_bwd_partial_rows(int M);
int dosx_mlp_ln_bwd(const DosxMlpLnBwd* a, dosx_stream_t stream);

/* STALL REPORT of the column-split exchanges above.  Their poll for the siblings' tickets is bounded; a poll that ends on its
 * bound instead of on the target used to fall through in silence.  Now thread 0 of that workgroup reports into a sticky device
 * status {code, kernel id, tile, stalls}: code = DOSX_EXCHANGE_STALLED from the first report on, kernel id / tile those of the FIRST
 * report, stalls the number of reports.  Outputs are NOT poisoned: between a stall and the host's next look at the status every
 * number the device produces is untrustworthy, and the stalled launch leaves tickets on its counters.
 *   dosx_exchange_status: a one-thread kernel copies the four words to out4 (caller-owned device memory) and, with clear != 0,
 *     zeroes the status behind the copy.  Stream-ordered, no sync.
 *   dosx_exchange_selftest: TEST ONLY - a one-thread kernel that files one report for (kernel_id, tile) and does nothing else.  It
 *     is how the report path is exercised: no test or tool may make a real exchange stall. */
enum { DOSX_EXCHANGE_OK = 0, DOSX_EXCHANGE_STALLED = 1 };
enum { DOSX_EXCHANGE_KERNEL_MLP_LN_CS_FWD = 1, DOSX_EXCHANGE_KERNEL_ENC_CS_FWD = 2, DOSX_EXCHANGE_KERNEL_MLP_LN_CS_BWD = 3 };
int dosx_exchange_status(int32_t* out4, int clear, dosx_stream_t stream);
int dosx_exchange_selftest(int kernel_id, int tile, dosx_stream_t stream);

/* The EdgeModel of one message-passing layer + the aggregation behind it in ONE launch (round 5; SURVEY.md §7 step 4;
 * DOSTransformer_phonon.py:186-197,209 and the edge residual :84), first Linear FACTORED (see DosxGemm.add_p):
 *     z    = e . Wc^T + b1 + pq[src[r], 0:2H] + pq[dst[r], 2H:4H]          Wc = first Linear's weight block [2H, H], row stride ldw1
 *     xhat = (z - mean) * rstd  (eps 1e-5; written with rstd: the backward and dosx_wgrad read them)
 *     msg  = prelu(xhat * gamma + beta) . W3^T + b3                        W3 [H, 2H]
 *     e_out = e + msg (skipped when NULL) ;  seg_agg[n] = seg_scale[n] * sum_{r in seg(n)} msg[r]
 * What dosx_gemm (EPI_LN + add_p / add_q) followed by dosx_gemm (PRO_LN_PRELU, EPI_SEGSUM) compute, for hidden 64 / 128: one
 * workgroup per node-aligned row tile of the batch's tile table (seg_* exactly as in DosxGemm), the [48, 2H] intermediate in LDS.
 * pq [nodes, >= 4H] holds the two node products P | Q (dosx_gemm_pair on the N node rows). */
typedef struct DosxEdgeMlp {
  int32_t E, H;
  const float* e; int32_t lde;
  const float* pq; int32_t ldpq;
  const int32_t* src; const int32_t* dst;
  const float* w1; int32_t ldw1; const float* b1;
  const float* gamma; const float* beta; const float* alpha;
  const float* w3; const float* b3;
  float* xhat; float* rstd;
  float* e_out; int32_t ldeo;
  const int32_t* seg_tile; int32_t seg_ntiles;
  const int32_t* seg_rowptr; const float* seg_scale; float* seg_agg; float* seg_part; int32_t* seg_cnt;
} DosxEdgeMlp;
/* Backward of the same block in one launch (what dosx_edge_grad_combine + dosx_gemm EPI_PRELU_LN_BWD_SEG + the E-row input-
 * gradient GEMM compute):
 *     dmsg[r] = de_next[r] + seg_scale[dst[r]] * dagg[dst[r]]     (written: W3's weight gradient reads it; de_next NULL: the last layer)
 *     dz = LayerNorm_bwd(PReLU_bwd(dmsg . W3))  [E,2H] written ;  seg_agg[n] = sum_{r in seg(n)} dz[r]  [nodes, 2H]  (unscaled)
 *     de[r] = dz[r] . Wc + de_next[r]                              (gradient of the layer's edge state)
 *     partials[tile] = [ dgamma (2H) | dbeta (2H) | pad | dalpha ]  - seg_ntiles rows, the layout of DOSX_EPI_PRELU_LN_BWD. */
typedef struct DosxEdgeMlpBwd {
  int32_t E, H;
  const float* dagg; int32_t lddagg;
  const float* de_next; int32_t ldden;
  const int32_t* dst;
  const float* xhat; const float* rstd;
  const float* w3;
  const float* w1; int32_t ldw1;
  const float* gamma; const float* beta; const float* alpha;
  float* dmsg;
  float* dz;
  float* de; int32_t ldde;
  float* partials; int32_t partial_ld;
  const int32_t* seg_tile; int32_t seg_ntiles;
  const int32_t* seg_rowptr; const float* seg_scale; float* seg_agg; float* seg_part; int32_t* seg_cnt;
} DosxEdgeMlpBwd;
int dosx_edge_mlp_bwd(const DosxEdgeMlpBwd* a, dosx_stream_t stream);
/* The NODE side of the factored EdgeModel input gradient in one launch (what dosx_segment_reduce_perm + a two-segment dosx_gemm
 * with w_seg_off compute; hidden 64 / 128 / 256):
 *     aggs[n] = sum_{e: src(e) = n} dz[e]   (rows perm_src[rowptr_src[n] .. rowptr_src[n+1]) of dz [E,2H]; written: the weight
 *                                            gradient of the source block reads it)
 *     dx[n]   = res[n] + res2[n] + aggs[n] . w[:, :H] + aggd[n] . w[:, H:2H]        w: the first Linear's weight [2H, 3H], row stride ldw
 * (DOSTransformer_phonon.py:166,190-197 differentiated w.r.t. x[row] / x[col]; res / res2 optional [N,H] addends). */
typedef struct DosxNodeGrad {
  int32_t N, H;
  const float* dz;
  const int32_t* rowptr_src; const int32_t* perm_src;
  const float* aggd;
  const float* w; int32_t ldw;
  const float* res; int32_t ldres;
  const float* res2; int32_t ldres2;
  float* aggs;
  float* dx; int32_t lddx;
} DosxNodeGrad;
int dosx_node_grad(const DosxNodeGrad* a, dosx_stream_t stream);
int dosx_edge_mlp_supported(int H);
int dosx_edge_mlp_fwd(const DosxEdgeMlp* a, dosx_stream_t stream);

/* Graph metadata ("CSR build") on the device, stream-ordered, no host round trip — counterpart of what PyG's
 * collate / to_dense_batch / torch_scatter derive per call from `edge_index` and `batch`
 * (DOSTransformer_phonon.py:48-56,86,209).
 *   edge_index [2,E] int64 (any order), batch [N] int64 non-decreasing, B graphs.
 *   dst/src [E]      : the edges STABLY sorted by destination (aggregation = contiguous segment sum);
 *   edge_perm [E]    : int64, position of sorted edge e in the caller's edge arrays (may be NULL);
 *   rowptr_dst/src [N+1], perm_src [E] : CSR by destination / by source (ids in the sorted numbering);
 *   graph_ptr [B+1], node_graph [N], dense_row [N] = pos*B + graph, inv_deg [N] = 1/max(in-degree,1);
 *   n_max [1]        : device scalar, atoms of the largest crystal (may be NULL).
 * workspace: dosx_csr_workspace_bytes(E) bytes of device scratch owned by the caller. */
int dosx_csr_workspace_bytes(int E, size_t* bytes);
int dosx_csr_build(const long long* edge_index, const long long* batch, int N, int E, int B, int32_t* src, int32_t* dst,
                   long long* edge_perm, int32_t* rowptr_dst, int32_t* perm_src, int32_t* rowptr_src,
                   int32_t* graph_ptr, int32_t* node_graph, int32_t* dense_row, float* inv_deg, int32_t* n_max,
                   void* workspace, size_t ws_bytes, dosx_stream_t stream);

/* BATCH VALIDATION (csrc/validate.hip; dostransformer_amd/validate.py) - the fail-loudly path in front of dosx_csr_build and of
 * every kernel that dereferences a batch: the caller's OWN arrays in the reference schema are checked before any metadata is
 * derived from them.  Lengths come from the caller's tensor shapes alone, every value is classified from the value itself, and
 * batch[src] is read only after src passed its range test, so the checker reads nothing outside the arrays whatever they hold.
 *   R1  an edge endpoint outside [0, N)                                             offender: edge
 *   R2  both endpoints in range, batch[src] != batch[dst] (an edge between crystals) offender: edge
 *   R3  batch[i] outside [0, B), or batch[i] < batch[i-1], or batch[0] != 0          offender: node
 *   R4  a crystal of [0, B) that owns no node                                        offender: crystal
 *   R5  system[b] outside [0, prompts)  (system != NULL)                             offender: crystal
 *   R6  n_max > 0 and a crystal owns more than n_max nodes                           offender: crystal
 *   R7  require_sorted != 0 and dst[e] < dst[e-1]                                    offender: edge
 * (R4 / R6 count the nodes whose batch value is the crystal's, wherever they stand.)
 * report: DOSX_CHECK_RULES pairs {count, first}, rule r at report[2(r-1)], caller-owned device memory that the caller
 * initialises to {0, INT32_MAX}; count = violations of the rule (saturating at INT32_MAX), first = the smallest offending index.
 * A sum and a minimum: the pair does not depend on the order of the (vector) atomics that form it.
 * crystal_count: B int32 words of caller-owned device scratch (zeroed here, stream-ordered).  No sync, no allocation.
 * The grid: DOSX_CHECK_THREADS threads, at most DOSX_CHECK_MAX_BLOCKS workgroups that stride over edges and nodes. */
#define DOSX_CHECK_RULES 7
#define DOSX_CHECK_THREADS 256
#define DOSX_CHECK_MAX_BLOCKS 1024
typedef struct DosxBatchCheck {
  const long long* edge_index;     /* [2,E] int64: sources, then destinations */
  const long long* batch;          /* [N] int64 */
  const long long* system;         /* [B] int64, may be NULL (no R5) */
  int32_t N, E, B;
  int32_t n_max;                   /* 0: not given (no R6) */
  int32_t prompts;                 /* rows of the prompt table: 7 for both models */
  int32_t require_sorted;          /* != 0: R7 */
  int32_t* crystal_count;          /* [B] scratch */
} DosxBatchCheck;
int dosx_batch_check(const DosxBatchCheck* d, int32_t* report, dosx_stream_t stream);
/* Non-finite elements (NaN, +-inf) of one contiguous tensor of n elements: report_slot = one {count, first} pair with the
 * conventions above (an index past INT32_MAX - 1 is reported as INT32_MAX - 1).  16-byte loads with scalar head / tail;
 * memory-bound: meant for a whole resident dataset table as much as for a batch. */
int dosx_finite_check_f32(const float* p, int64_t n, int32_t* report_slot, dosx_stream_t stream);
int dosx_finite_check_f64(const double* p, int64_t n, int32_t* report_slot, dosx_stream_t stream);

/* Collate on the device: the dataset is resident with per-crystal destination-sorted edges and cached
 * local CSR (`*_all` arrays, crystal c owns nodes [node_ptr_all[c], node_ptr_all[c+1]) and edges likewise; its cached
 * row pointers have n_c + 1 entries starting at node_ptr_all[c] + c).  `sel [B]` picks the crystals of the batch,
 * `out_node_ptr / out_edge_ptr [B+1]` are the batch's prefix sums (N, E = their last entries).  Outputs: everything
 * dosx_csr_build would give for the concatenated batch (already destination-sorted), plus `batch` / `edge_index` in
 * the reference's int64 schema and `node_row [N]`, `edge_row [E]` = source rows for gathering the feature tensors. */
int dosx_collate(const int32_t* sel, const int32_t* node_ptr_all, const int32_t* edge_ptr_all, const int32_t* out_node_ptr,
                 const int32_t* out_edge_ptr, int B, int N, int E, const int32_t* src_all, const int32_t* dst_all,
                 const int32_t* perm_src_all, const int32_t* rowptr_dst_all, const int32_t* rowptr_src_all,
                 const float* inv_deg_all, long long* batch, long long* edge_index, int32_t* src, int32_t* dst,
                 int32_t* perm_src, int32_t* rowptr_dst, int32_t* rowptr_src, int32_t* node_graph, int32_t* dense_row,
                 float* inv_deg, int32_t* node_row, int32_t* edge_row, dosx_stream_t stream);

/* Collate straight into the STATIC buffers of a shape bucket, ghost padding included (train.Trainer.step_dataset): the
 * selected crystals' segments + feature rows as dosx_collate / the row gathers would give them, followed by the ghost tail
 * batch.pad_batch appends (ghost nodes: zero features, node_graph = B, dense slot n_max*B; ghost edges: self loops on the
 * first ghost node, zero features; rowptr[N] = E, rowptr[N+1..N_pad] = E_pad).  All pointers device memory; feature data
 * fp32.  target: [B,S] rows (phdos / y_ft), glob: [B,n_glob] (n_glob = 0: none), system: int32 [B].
 * node_row / edge_row: scratch [N_pad] / [E_pad].  Needs N_pad > N (at least one ghost node). */
typedef struct DosxCollate {
  int32_t B, N, E, N_pad, E_pad, n_max, Fa, Fe, S, n_glob;
  const int32_t* sel;
  const int32_t* out_node_ptr;
  const int32_t* out_edge_ptr;
  const int32_t* node_ptr_all;
  const int32_t* edge_ptr_all;
  const int32_t* src_all;
  const int32_t* dst_all;
  const int32_t* perm_src_all;
  const int32_t* rowptr_dst_all;
  const int32_t* rowptr_src_all;
  const float* inv_deg_all;
  const float* x_all;
  const float* edge_feat_all;
  const float* target_all;
  const float* glob_all;
  const int32_t* system_all;
  float* x;
  float* edge_feat;
  float* target;
  float* glob;
  int32_t* system;
  int32_t* src;
  int32_t* dst;
  int32_t* perm_src;
  int32_t* rowptr_dst;
  int32_t* rowptr_src;
  int32_t* graph_ptr;
  int32_t* node_graph;
  int32_t* dense_row;
  float* inv_deg;
  int32_t* node_row;
  int32_t* edge_row;
  /* optional: node-aligned row tiles of the message GEMM (DosxGemm EPI_SEGSUM), seg_tile [3][T+1] (NULL = skip).  Crystal c
   * owns the tiles [tile_off_all[c], tile_off_all[c+1]) of tile_e_all / tile_n_all / tile_p_all (crystal-local START edge /
   * node and the chunk info of each tile); out_tile_ptr [B+1] = prefix sums of the selected crystals' tile counts; ghost
   * edges follow in tile_rows-row tiles, the first of which owns every ghost node; the remaining slots are empty. */
  int32_t T, tile_rows;
  const int32_t* out_tile_ptr;
  const int32_t* tile_off_all;
  const int32_t* tile_e_all;
  const int32_t* tile_n_all;
  int32_t* seg_tile;
  const int32_t* tile_p_all;
} DosxCollate;
int dosx_collate_padded(const DosxCollate* d, dosx_stream_t stream);

/* The same collate into the bucket of the float64 program (train64.Trainer64.step_dataset): same descriptor, same index
 * outputs, but x_all / edge_feat_all / target_all and x / edge_feat / target point at `double` tables and buffers (the `float*`
 * fields carry their addresses; all 8-byte aligned); system stays int32, inv_deg stays float.  n_glob must be 0 and seg_tile
 * NULL (the float64 program is the phonon one and has no tiled message GEMM).  Rows of x / target move as 16-byte vectors
 * when the tables are 16-byte aligned and the row width is even. */
int dosx_collate_padded_f64(const DosxCollate* d, dosx_stream_t stream);

/* Periodic neighbour list of C crystals at once (replaces ASE's `neighbor_list("ijS", a, cutoff=r_max,
 * self_interaction=True)` + the edge_vec arithmetic of `utils.py:267-273` in build_data).  `pos [N][3]` Cartesian,
 * `cell [C][3][3]` lattice vectors as rows, crystal c owns atoms [atom_ptr[c], atom_ptr[c+1]) and the ordered atom
 * pairs [pair_ptr[c], pair_ptr[c+1]) (pair_ptr = prefix sums of n_c^2, n_pairs = its last entry).  An edge is a triple
 * (i, j, S) with |pos[j]-pos[i]+S·cell| < cutoff; (i, i, 0) only if `self_interaction`; bit k of `pbc_mask` = axis k is
 * periodic.  Two passes: `_count` writes the number of edges of every pair, the caller turns it into exclusive offsets
 * `pair_off` (E = their total), `_fill` writes per edge: crystal, src = i and dst = j (crystal-local), shift [E][3],
 * edge_vec [E][3] = pos[dst]-pos[src]+shift·cell.  Order: crystal, i, j, shift (lexicographic) — deterministic. */
int dosx_neighbor_count(const double* pos, const double* cell, const int32_t* atom_ptr, const long long* pair_ptr, int C,
                        long long n_pairs, double cutoff, int self_interaction, int pbc_mask, int32_t* pair_count,
                        dosx_stream_t stream);
int dosx_neighbor_fill(const double* pos, const double* cell, const int32_t* atom_ptr, const long long* pair_ptr, int C,
                       long long n_pairs, double cutoff, int self_interaction, int pbc_mask, const long long* pair_off,
                       int32_t* crystal, int32_t* src, int32_t* dst, int32_t* shift, double* edge_vec,
                       dosx_stream_t stream);

/* The Electron-DOS crystal graph of C crystals at once (`data/mat2graph.py:120-243`: pymatgen's `get_all_neighbors(radius)`,
 * sorted by distance, cut at max_num_nbr, Gaussian-expanded; pymatgen is neither in the reference tree nor pinned, so this
 * comment is the contract - PARITY UNPINNED at that boundary, like ASE's for dosx_neighbor_*).  One launch, N*K edges out.
 *   neighbour set  for atom i of a crystal: every periodic image (j, S) of an atom j of the same crystal, S an integer shift,
 *                  with  tol*tol < r2 <= radius*radius ,  d = (pos[j]-pos[i]) + ((S0*a0 + S1*a1) + S2*a2) ,
 *                  r2 = (dx*dx + dy*dy) + dz*dz  in float64 without fused multiply-adds (dosx_neighbor_*'s arithmetic, bit for
 *                  bit).  The atom itself and a coincident atom are out (r2 <= tol*tol); images (i, i, S != 0) are in.  Bit k
 *                  of `pbc_mask` = axis k is periodic (otherwise S_k = 0).
 *   selection      the K smallest by the key (r2 compared as a number, then j, then S0, S1, S2), ascending.  The reference
 *                  leaves the order inside a distance tie to pymatgen; this key fixes it.  Ranking is on r2, never on a root.
 *   outputs        rank r of atom i is row i*K + r:  nbr_idx = j (crystal-local), nbr_shift = S, nbr_dist = sqrt(r2);
 *                  nbr_count[i] = neighbours kept (<= K).  Ranks from nbr_count[i] on are the reference's padding
 *                  (`:222-227`): nbr_idx 0, nbr_shift 0, nbr_dist = pad_dist (the reference's radius + 1).
 *   edge_attr      (optional) row i*K + r, column g:  t = nbr_dist - centers[g];  (float) exp(-(t*t) / (var*var)) , float64
 *                  without fused multiply-adds, rounded to float32 once (`:162-179,237`); padded ranks included.
 * Atoms per crystal and box sizes are free, but a shift digit is held in 11 bits: a pair whose shift box passes |S_k| = 1023 on
 * an axis (a cell below radius/1000, a position a thousand cells away, a singular cell) contributes no neighbour.  The result is
 * a pure function of the crystal (no atomics, no dependence on scheduling).  Required: 1 <= K <= 16 and N*K < 2^31; refused
 * with rc -22 before any launch: null descriptor, C <= 0, N < 0, K out of range, radius <= 0, tol < 0, a null
 * pos / cell / atom_ptr / nbr_idx / nbr_shift / nbr_dist / nbr_count, and with edge_attr set G < 1, null centers, var <= 0.
 * N == 0 returns 0 without a launch. */
typedef struct DosxKnn {
  int32_t C, N, K, G, pbc_mask, reserved;
  double radius, tol, pad_dist, var;
  const double* pos;        /* [N][3] Cartesian */
  const double* cell;       /* [C][3][3], rows = lattice vectors */
  const int32_t* atom_ptr;  /* [C+1] */
  const double* centers;    /* [G] Gaussian centres, made by the host with numpy.arange so they are bitwise the reference's */
  int32_t* nbr_idx;         /* [N][K] crystal-local neighbour index, 0 in the padding */
  int32_t* nbr_shift;       /* [N][K][3], 0 in the padding */
  double*  nbr_dist;        /* [N][K], pad_dist in the padding */
  int32_t* nbr_count;       /* [N] real neighbours kept (<= K) */
  float*   edge_attr;       /* [N*K][G], may be NULL (then G, centers, var are ignored) */
} DosxKnn;
int dosx_knn_graph(const DosxKnn* d, dosx_stream_t stream);

/* The crystal system of C crystals from their structures (the prompt label `entry.crystal_system` of `utils.py:277-290`, which
 * the reference takes from Materials-Project metadata, i.e. pymatgen / spglib; neither is in the reference tree nor pinned, so
 * this comment is the contract - PARITY UNPINNED at that boundary: spglib's angle tolerance and refinement are not restated, and a
 * structure within symprec of a symmetry change may be labelled differently there).  All arithmetic is float64 without fused
 * multiply-adds.  `cell [C][3][3]` = a basis A, rows = lattice vectors; `frac [N][3]` = fractional rows x with r = x A;
 * `species [N]` >= 0; crystal c owns atoms [atom_ptr[c], atom_ptr[c+1]); symprec in Angstrom (0.1 is Materials Project's).
 *   distance       of a moved atom y to atom k:  d = y - x_k ,  d -= rint(d) ,  c_a = (d0*A[0][a] + d1*A[1][a]) + d2*A[2][a] ,
 *                  r2 = (c0*c0 + c1*c1) + c2*c2 ;  y "lands on" k when r2 < symprec*symprec and species[k] is y's species.
 *   reference atom the first atom of the rarest species, ties to the smallest species number.
 *   (a) the caller Delaunay-reduces every cell (dostransformer_amd/symmetry.py: delaunay_reduce) before either call.
 *   (b) dosx_sym_translations: flag[j] = 1 iff j is another atom of the reference atom's species and, with t = x_j - x_ref,
 *       y = x_i + t lands on some k for EVERY atom i; 0 otherwise (other species and the reference atom included).  The caller
 *       takes the lattice generated by A and the n_t flagged t (volume V / (n_t + 1)), Delaunay-reduces it and re-expresses all
 *       atoms in it; coincident copies stay.
 *   (c) dosx_sym_point_group, lattice operations: integer W with entries in {-1, 0, 1} and |det W| = 1 whose images
 *       a_i' = (W[i][0]*A[0] + W[i][1]*A[1]) + W[i][2]*A[2] keep the six lengths |a_0|, |a_1|, |a_2|, |a_0+a_1|, |a_0+a_2|,
 *       |a_1+a_2| : | |v'| - |v| | < symprec , |v| = sqrt((v0*v0 + v1*v1) + v2*v2).  n_lattice_ops counts them; more than 48
 *       is no lattice's holohedry: code 7, n_ops 0, nothing kept.
 *   (d) structure operations: W is kept iff for some atom j of the reference species, with
 *       t = x_j - ((xr0*W[0] + xr1*W[1]) + xr2*W[2])  (xr = x_ref),  y = ((xi0*W[0] + xi1*W[1]) + xi2*W[2]) + t lands on some k
 *       for every atom i.  ops [C][48][9] int8: the n_ops kept matrices, row-major, in the lexicographic order of their nine
 *       entries; zeros after them.
 *   (e) hist [C][5]: the DISTINCT proper parts det(W) * W counted by trace -1, 0, 1, 2, 3 (2-, 3-, 4-, 6-fold rotations,
 *       identity).  code [C]: the histogram must be one of the eleven proper point groups (N2 N3 N4 N6 | order | code)
 *         1: 0 0 0 0 | 1 | 6     2: 1 0 0 0 | 2 | 5     222: 3 0 0 0 | 4 | 4    4: 1 0 2 0 | 4 | 2    422: 5 0 2 0 | 8 | 2
 *         3: 0 2 0 0 | 3 | 3    32: 3 2 0 0 | 6 | 3       6: 1 2 0 2 | 6 | 1  622: 7 2 0 2 | 12 | 1   23: 3 8 0 0 | 12 | 0
 *         432: 9 8 6 0 | 24 | 0
 *       with one identity, as many distinct proper parts as the order, and n_ops once or twice the order; the codes are the
 *       reference's (0 Cubic, 1 Hexagonal, 2 Tetragonal, 3 Trigonal, 4 Orthorhombic, 5 Monoclinic, 6 triclinic).  Anything
 *       else is INCONSISTENT: code 7, never a silent 6.
 * One workgroup per crystal; coordinates and species are staged in LDS up to 1024 atoms and read from global memory beyond.
 * Every "some" / "every" search may stop early, which cannot change the answer; there are no atomics and the outputs are a pure
 * function of the crystal.  n_min / n_max: the smallest / largest number of atoms of a crystal, stated by the caller (atom_ptr
 * lives on the device); the kernels leave a crystal they find outside [1, n_max] untouched.  Refused with rc -22 before any
 * launch: null descriptor, C <= 0, N <= 0, n_min <= 0 (an empty crystal), n_max < n_min or >= 2^21, symprec <= 0 or NaN, a
 * null buffer. */
typedef struct DosxSymTranslations {
  int32_t C, N, n_min, n_max;
  double symprec;
  const double* cell;       /* [C][3][3] Delaunay-reduced, rows = lattice vectors */
  const double* frac;       /* [N][3] fractional rows in that basis */
  const int32_t* species;   /* [N] */
  const int32_t* atom_ptr;  /* [C+1] */
  void* flag;               /* [N] one byte per atom */
} DosxSymTranslations;
int dosx_sym_translations(const DosxSymTranslations* d, dosx_stream_t stream);

typedef struct DosxSymPointGroup {
  int32_t C, N, n_min, n_max;
  double symprec;
  const double* cell;       /* [C][3][3] reduced primitive cells */
  const double* frac;       /* [N][3] */
  const int32_t* species;   /* [N] */
  const int32_t* atom_ptr;  /* [C+1] */
  int32_t* n_lattice_ops;   /* [C] */
  int32_t* n_ops;           /* [C] */
  void* ops;                /* [C][48][9] int8 */
  int32_t* hist;            /* [C][5] */
  int32_t* code;            /* [C] */
} DosxSymPointGroup;
int dosx_sym_point_group(const DosxSymPointGroup* d, dosx_stream_t stream);

/* DOS targets of C crystals from their raw spectra (csrc/spectra.hip): Gaussian broadening onto a grid (dosx_spectra_broaden) and
 * linear resampling onto it (dosx_spectra_interp).  The reference reads finished targets (`data/mat2graph.py:81-92`:
 * `densities_total_1_ft`, `densities_total_1`) and never shows how they are made, so this comment is the contract; the numpy twin
 * is dostransformer_amd/spectra.py.  Every input and every operation is float64, one rounding per operation as written, no fused
 * multiply-adds.  Crystal c owns the samples [ptr[c], ptr[c+1]) of `e` (energies) and `v` (values), n = their number.
 *   grid      E_s = e0 + de * (double)s ,  s = 0..S-1.
 *   samples   ec_i = e_i - shift[c]  (shift = the Fermi level; 0 for phonons).
 *   weights   DOSX_SPECTRA_POINTS: w_i = v_i (delta peaks: mode frequencies with q-point weights; any order, n = 0 allowed).
 *             DOSX_SPECTRA_CURVE: v is a density tabulated on strictly ascending e, n >= 2; trapezoid weights of the raw e:
 *             w_0 = v_0 * (0.5 * (e_1 - e_0)) ,  w_i = v_i * (0.5 * (e_{i+1} - e_{i-1})) ,  w_{n-1} = v_{n-1} * (0.5 * (e_{n-1} - e_{n-2})).
 *   broaden   g = 1 / (sigma[c] * 2.5066282746310002)  (the double nearest sqrt(2 pi)) ;  per bin s and sample i:
 *             x = (E_s - ec_i) / sigma[c]  (a true division) ;  the term is kept iff fabs(x) <= cutoff ;
 *             t_i = (w_i * g) * exp(-0.5 * (x * x)) ;  y[c][s] starts at 0.0 and the kept t_i are added to it in ascending i.
 *             A dropped term adds nothing, not even a +0.0.  Only exp may differ from another implementation, by its last
 *             place.  The order of summation depends on (n, S) alone: no atomics, bitwise the same from run to run.
 *   interp    (curves) outside [ec_0, ec_{n-1}] (or when a comparison with E_s is unordered) y = 0 ; otherwise j = the last index
 *             with ec_j <= E_s ;  j = n-1 gives v_{n-1} ;  else  y = v_j + (v_{j+1} - v_j) * ((E_s - ec_j) / (ec_{j+1} - ec_j)).
 *   y_max [C] the row maximum (S >= 1: never -inf).   area [C] = de * (((y_0 + y_1) + y_2) + ...), ascending s.
 *   y_norm    (optional, NULL = skip) y / y_max, zeros where y_max <= 0.
 *   report    [C][4] int32: n_inside = samples with lo <= ec_i <= hi, lo = E_0 - (cutoff * sigma[c]), hi = E_{S-1} + (cutoff *
 *             sigma[c]) (interp: lo = E_0, hi = E_{S-1}) ;  covered = (ec_0 <= E_0 && ec_{n-1} >= E_{S-1}) for a curve, 1 for
 *             points ;  bad = samples with a non-finite e_i or v_i, plus 1 for a shift[c] that is not finite, plus 1 for a
 *             sigma[c] that is not a finite number above 0 ;  unsorted = for a curve the number of i with e_{i+1} <= e_i.
 * A crystal with bad > 0, or a curve with unsorted > 0, gets NaN in its row of y and y_norm and in y_max and area, and its counts;
 * no other crystal's row is touched.  n_min / n_max: the smallest / largest n, stated by the caller (ptr lives on the device); a
 * crystal the kernel finds outside [n_min, n_max] or outside [0, T] gets the NaN row and the report (0, 0, -1, 0), and none of its
 * samples is read.  One 256-lane workgroup per crystal, one launch per call.  Refused with rc -22 before any launch: null
 * descriptor, C <= 0, T < 0, S outside [1, 1024], e0 or de not finite, de <= 0 with S > 1, cutoff <= 0 or NaN, an unknown kind,
 * n_min < 0, a curve with n_min < 2, n_max < n_min or n_max >= 2^20, a null ptr / shift / sigma / y / y_max / area / report, and
 * with T > 0 a null e / v. */
enum { DOSX_SPECTRA_POINTS = 0, DOSX_SPECTRA_CURVE = 1 };
typedef struct DosxSpectra {
  int32_t C, T, S, kind, n_min, n_max;
  double e0, de, cutoff;
  const int32_t* ptr;       /* [C+1] */
  const double* e;          /* [T] */
  const double* v;          /* [T] */
  const double* shift;      /* [C] */
  const double* sigma;      /* [C] */
  double* y;                /* [C][S] */
  double* y_max;            /* [C] */
  double* area;             /* [C] */
  double* y_norm;           /* [C][S], may be NULL */
  int32_t* report;          /* [C][4]: n_inside, covered, bad, unsorted */
} DosxSpectra;
int dosx_spectra_broaden(const DosxSpectra* d, dosx_stream_t stream);

typedef struct DosxSpectraInterp {
  int32_t C, T, S, reserved, n_min, n_max;
  double e0, de;
  const int32_t* ptr;       /* [C+1] */
  const double* e;          /* [T] strictly ascending inside a crystal */
  const double* v;          /* [T] */
  const double* shift;      /* [C] */
  double* y;                /* [C][S] */
  double* y_max;            /* [C] */
  double* area;             /* [C] */
  double* y_norm;           /* [C][S], may be NULL */
  int32_t* report;          /* [C][4] */
} DosxSpectraInterp;
int dosx_spectra_interp(const DosxSpectraInterp* d, dosx_stream_t stream);

/* Replay of a recorded launch list (the host side of train.Trainer(replay=True), see csrc/replay.cpp): `n` calls are
 * issued in order.  A call names its callee by `op` (from dosx_replay_op: every `int dosx_*` entry point of this header,
 * plus "hipEventRecord" / "hipStreamWaitEvent" for stream fork/join) and carries the callee's integer-class arguments in
 * declaration order (pointers, integers, by-pointer descriptors; at most 19) and its float/double arguments in
 * declaration order (at most 6).  Each op is dispatched through a typed thunk generated from this header, i.e. an
 * ordinary C call.  Returns the first non-zero return code (its index in *failed_index) or 0. */
enum { DOSX_OP_HIP_BASE = 1000 };
typedef struct DosxCall {
  int32_t op;
  int32_t nint;
  int32_t nflt;
  int32_t reserved;
  int64_t iarg[19];
  double farg[6];
} DosxCall;
/* op index of an entry point by name (-1 if unknown); optionally its integer-class / floating-point argument counts */
int dosx_replay_op(const char* name, int* n_int, int* n_float);
int dosx_replay(const DosxCall* calls, int n, int* failed_index);
/* Measurement twin: replays the list with a HIP event pair around every library entry, recorded on the stream that entry
 * launches on; ms_out[n] (HOST array) receives the elapsed milliseconds of every entry.  Ends with a device
 * synchronisation - diagnostic use only (bench.py's per-kernel roofline figures). */
int dosx_replay_timed(const DosxCall* calls, int n, float* ms_out, int* failed_index);

/* misc */
/* Dropout multiplier: mask[i] = u_i >= p ? 1/(1-p) : 0 with u_i uniform in [0,1) from Philox4x32-10 (counter = (i/4, stream_id),
 * key = *seed_dev, word i%4 of the block; the top 24 bits make u).  The seed is read FROM DEVICE MEMORY so a recorded /
 * graph-captured program draws fresh masks on every replay: the caller bumps *seed_dev between steps.  stream_id
 * separates the masks of different layers / sites drawn under one seed. */
int dosx_dropout_mask(float* mask, int64_t n, float p, const unsigned long long* seed_dev, long long stream_id,
                      dosx_stream_t stream);
/* Batched device-to-device copy in ONE launch: dst[0:dwords] = src[0:dwords] (32-bit words, 4-byte aligned, any mix of
 * fp32 / int32 buffers).  jobs: HOST array, copied into kernel arguments (no device table, graph-capturable).
 * train._Slot.load moves a batch's fields and CSR arrays into the static buffers of its shape bucket with it. */
typedef struct DosxCopyJob {
  const void* src;
  void* dst;
  int64_t dwords;
} DosxCopyJob;
int dosx_copy_many(const DosxCopyJob* jobs_host, int n_jobs, dosx_stream_t stream);
int dosx_fill(float* p, float value, int64_t n, dosx_stream_t stream);
/* out[r] = table[idx[r]] rows (prompt_token[g.system], DOSTransformer_phonon.py:105) and its backward
 * (deterministic: one workgroup per table row scans idx). */
int dosx_embed_rows(const float* table, const int32_t* idx, float* out, int rows, int width, dosx_stream_t stream);
int dosx_embed_rows_bwd(const float* dout, int ld_dout, const int32_t* idx, float* dtable, int rows,
                        int table_rows, int width, dosx_stream_t stream);
/* dst[i, 0:width] (+)= sum_{j < n_red} src[(i*stride_out + j*stride_red), 0:width]
 * Row reductions of the [S,B,H] layout: over the batch (gradient of the energy-embedding broadcast,
 * DOSTransformer_phonon.py:143: n_out=S, n_red=B, stride_out=B, stride_red=1) or over the energy bins
 * (gradient of graph.expand(51,...), :91: n_out=B, n_red=S, stride_out=1, stride_red=B). */
int dosx_reduce_rows(const float* src, int ld_src, float* dst, int ld_dst, int n_out, int n_red, int stride_out,
                     int stride_red, int width, int accumulate, dosx_stream_t stream);
/* out = dy * (y > 0 ? 1 : slope): backward of F.leaky_relu (DOSTransformer_phonon.py:95) from its output. */
int dosx_act_bwd(const float* dy, const float* y, float slope, float* out, int64_t n, dosx_stream_t stream);

/* ---- float64 program (csrc/f64.hip) -------------------------------------------------------------------------------------
 * The phonon reference computes in float64 (main_phDOS.py:15-16).  A Graphnetwork_phonon whose live parameters are float64
 * runs these entry points instead of the fp32 ones above.  Everything here is fp64 row-major (index data int32) and
 * deterministic: no atomics on data, every reduction in a fixed order.  Matrix products use v_mfma_f64_16x16x4_f64. */

/* One K-segment of an fp64 operand: columns [0, width) of rows map(r) of p (row stride ld doubles). */
typedef struct DosxSeg64 {
  const double* p;
  int32_t ld;
  int32_t width;
  DosxRowMap map;
} DosxSeg64;

/* act of dosx_gemm_f64 */
enum { DOSX_ACT64_NONE = 0, DOSX_ACT64_RELU = 1, DOSX_ACT64_LEAKY = 2 /* slope 0.01 */, DOSX_ACT64_PRELU = 3 /* *alpha */ };

/* out[M,N] = act(cat_k(A segments)[M,K] * op(W) + bias) + res
 *   w_layout 0: W[N,K] (y = x W^T, nn.Linear forward); 1: W[K,N] (dx = dy W, input gradients).
 *   pre (optional): the pre-activation acc + bias, [M, ldo]; res (optional): [M, ldr] added after the activation.
 * K = sum of the segment widths (any value >= 1: the k tail of every segment is zero-padded). */
typedef struct DosxGemm64 {
  int32_t M, N, K;
  int32_t nseg;
  DosxSeg64 a[3];
  const double* w;
  int32_t ldw;
  int32_t w_layout;
  int32_t act;
  const double* alpha; /* device scalar, ACT64_PRELU */
  const double* bias;  /* [N] or NULL */
  double* out;
  int32_t ldo;
  double* pre;
  const double* res;
  int32_t ldr;
} DosxGemm64;

/* dw[N,K] (+)= dy[M,N]^T * cat_k(X segments)[M,K]  (weight gradient of y = x W^T).  M is cut into nsplit row ranges; with
 * nsplit > 1 each range writes its own slice of partials [nsplit, N, K] and a second launch adds the slices in order. */
typedef struct DosxWgrad64 {
  int32_t M, N, K;
  const double* dy;
  int32_t lddy;
  int32_t nseg;
  DosxSeg64 x[3];
  double* dw;
  int32_t ldd;
  int32_t accumulate;
  int32_t nsplit;
  double* partials; /* [nsplit, N, K], needed when nsplit > 1 */
} DosxWgrad64;

int dosx_gemm_f64(const DosxGemm64* desc_host, dosx_stream_t stream);
int dosx_wgrad_f64(const DosxWgrad64* desc_host, dosx_stream_t stream);
/* out[0:N] (+)= column sums of src[M,N] (row stride ld), rows added in order.  partials: [ceil(M/DOSX_COLSUM64_ROWS), N]
 * scratch, needed when M > DOSX_COLSUM64_ROWS. */
#define DOSX_COLSUM64_ROWS 256
int dosx_colsum_f64(const double* src, int M, int N, int ld, double* partials, double* out, int accumulate,
                    dosx_stream_t stream);
/* LayerNorm (eps 1e-5) of z[M,W] with affine gamma / beta, then PReLU(*alpha) when alpha != NULL:
 * out = prelu(xhat * gamma + beta); saves xhat [M,W] and rstd [M].  W <= 1024. */
int dosx_layernorm_f64(const double* z, const double* gamma, const double* beta, const double* alpha, double* xhat,
                       double* rstd, double* out, int M, int W, dosx_stream_t stream);
/* Backward of dosx_layernorm_f64: dz [M,W] from dout; part [M, 2W+1] = per row dout_y*xhat | dout_y | dalpha term
 * (dosx_colsum_f64 of part gives dgamma | dbeta | dalpha). */
int dosx_layernorm_bwd_f64(const double* dout, const double* xhat, const double* rstd, const double* gamma,
                           const double* beta, const double* alpha, double* dz, double* part, int M, int W,
                           dosx_stream_t stream);
/* Activation backward from the pre-activation z [M,W] (rows of stride ld): dz = dy * act'(z).  act: ACT64_*; for PRELU,
 * part [M] gets the per-row dalpha term sum_c dy*z*(z<0) (NULL otherwise). */
int dosx_act_bwd_f64(const double* dy, const double* z, int ld, int act, const double* alpha, double* dz, double* part,
                     int M, int W, dosx_stream_t stream);
/* out[e] = smooth_cutoff(|v|/r_max) * [1, sqrt3 v/max(|v|,1e-12)]  (DOSTransformer_phonon.py:74-77), out [E,4] */
int dosx_edge_feat_sh1_f64(const double* edge_vec, double* out, int E, double r_max, dosx_stream_t stream);
/* out[n] = sum_{e in [rowptr[n], rowptr[n+1])} src[e] / max(in-degree, 1)  (scatter_mean over destinations) */
int dosx_segment_mean_f64(const double* src, const int32_t* rowptr, double* out, int N, int H, dosx_stream_t stream);
/* Backward of the mean aggregation plus the edge residual: out[e] = res[e] + dagg[dst[e]] / max(in-degree(dst[e]), 1)
 * (res may be NULL; dagg rows of stride ld_dagg). */
int dosx_segment_mean_bwd_f64(const double* dagg, int ld_dagg, const int32_t* dst, const int32_t* rowptr,
                              const double* res, double* out, int E, int H, dosx_stream_t stream);
/* Gradient of the node operands of cat[x[src], x[dst], .] as CSR sums in a fixed order:
 * dx[n] = base0[n] + base1[n] + sum_{k in [rowptr_src[n], rowptr_src[n+1])} dcat[perm_src[k], 0:H]
 *                             + sum_{e in [rowptr_dst[n], rowptr_dst[n+1])} dcat[e, H:2H]
 * (base0 / base1 optional, rows of stride ld0 / ld1; dcat rows of stride ldc). */
int dosx_gather_bwd_f64(const double* dcat, int ldc, const int32_t* rowptr_src, const int32_t* perm_src,
                        const int32_t* rowptr_dst, const double* base0, int ld0, const double* base1, int ld1,
                        double* dx, int N, int H, dosx_stream_t stream);
/* out[b] = sum_{n in [graph_ptr[b], graph_ptr[b+1])} x[n]  (scatter_sum over crystals, nodes in crystal order) */
int dosx_graph_pool_f64(const double* x, const int32_t* graph_ptr, double* out, int B, int H, dosx_stream_t stream);
/* out[r] = a[ia ? ia[r] : r] + b[ib ? ib[r] : r]  (rows of width W; b optional): residual adds and the backward of a
 * row broadcast (dx += dpool[node_graph]) */
int dosx_rows_add_f64(const double* a, int lda, const int32_t* ia, const double* b, int ldb, const int32_t* ib,
                      double* out, int ldo, int M, int W, dosx_stream_t stream);
/* dst[i, 0:width] (+)= sum_{j < n_red} src[(i*stride_out + j*stride_red), 0:width]  (fp64 dosx_reduce_rows) */
int dosx_reduce_rows_f64(const double* src, int ld_src, double* dst, int ld_dst, int n_out, int n_red, int stride_out,
                         int stride_red, int width, int accumulate, dosx_stream_t stream);

/* ---- float64 attention of DOSTransformer_phonon (csrc/f64_attention.hip) -----------------------------------------------
 * One encoder layer's attention half (layers/multihead_attention.py:49-76, transformer.py:131-137), single head, no
 * projections: out = x + (softmax(q k^T * H^-1/2) o drop_mask) v with k = v = kvhat * gamma0 + beta0.  Query rows are
 * crystal-major, row bq * Sq + s of q / x / out / dout / dq; key rows row bk * Nk + j of kvhat / dkvhat, with
 * bk = bq % Bk (Bq a multiple of Bk); probabilities, masks and ds are [Bq, Sq, Nk].  The scores and both products are
 * fp64; the softmax follows the reference: scores rounded to fp32, softmax in fp32 (accurate expf), promoted - and its
 * backward the autograd mirror (dP o mask rounded to fp32, p (dP - sum p dP) in fp32, promoted, times H^-1/2).
 * DOSX_ATTN64_SOFTMAX_F64 computes the softmax and its backward in fp64 instead (a test hook, not the reference).
 * key_ptr (device, [Bk + 1], or NULL: every key row takes part, the reference's unmasked padding): key crystal bk has
 * n = key_ptr[bk+1] - key_ptr[bk] keys (clamped to [0, Nk]), the rows j >= n do not exist for any query crystal that reads
 * it - what the reference computes for that crystal alone in a batch of one.  Nothing of kvhat, probs, ds or drop_mask
 * past n is read; probs, ds and part are written as 0.0 there, dkvhat as 0.0 unless accumulate (then left alone); n = 0
 * gives out = x. */
#define DOSX_ATTN64_MAX_H 512
#define DOSX_ATTN64_SOFTMAX_F64 1
typedef struct DosxAttn64 {
  int32_t Sq, Bq, Nk, Bk, H;
  int32_t flags;            /* DOSX_ATTN64_* */
  const double* q;          /* [Bq*Sq, H] LayerNorm 0 of the query rows */
  const double* x;          /* [Bq*Sq, H] the residual (forward) */
  const double* kvhat;      /* [Bk*Nk, H] normalised key rows (zero rows: padding keys, k = v = beta0) */
  const double* gamma0;     /* [H] */
  const double* beta0;      /* [H] */
  const float* drop_mask;   /* [Bq, Sq, Nk] dropout multipliers applied after the softmax, or NULL */
  double* out;              /* [Bq*Sq, H] x + attn (forward) */
  double* probs;            /* [Bq, Sq, Nk] the un-dropped probabilities (written by the forward, read by the backward) */
  const double* dout;       /* [Bq*Sq, H] gradient of the attention output (backward) */
  double* dq;               /* [Bq*Sq, H] gradient of q (backward) */
  double* ds;               /* [Bq, Sq, Nk] scratch: gradient of the scores (backward) */
  double* dkvhat;           /* [Bk*Nk, H] (+)= dkv * gamma0, dkv the summed key + value gradient (backward) */
  double* part;             /* [Bk*Nk, 2H] per key row dkv * kvhat | dkv: column sums are dgamma0 | dbeta0 (backward) */
  int32_t accumulate;       /* dkvhat += instead of = */
  const int32_t* key_ptr;   /* [Bk + 1] device: per-crystal key counts (the batch's graph_ptr), or NULL */
} DosxAttn64;
/* forward: writes out and probs */
int dosx_attention_f64(const DosxAttn64* desc_host, dosx_stream_t stream);
/* backward: dq and ds per query tile, then a second launch reduces each key tile's dkv over every query row that reads it,
 * in a fixed order (crystals bk, bk + Bk, ..., rows in order) */
int dosx_attention_bwd_f64(const DosxAttn64* desc_host, dosx_stream_t stream);
/* to_dense_batch + parameter-free LayerNorm (eps 1e-5): out[b*nmax + j] = normalised x[graph_ptr[b] + j] for
 * j < graph_ptr[b+1] - graph_ptr[b], else a zero row; rstd [N] per node.  H <= 1024. */
int dosx_dense_rows_f64(const double* x, const int32_t* graph_ptr, double* out, double* rstd, int B, int nmax, int H,
                        dosx_stream_t stream);
/* its backward: dx[n] (+)= rstd (g - mean(g) - xhat mean(g xhat)) of the dense row of node n (ghost rows are dropped) */
int dosx_dense_rows_bwd_f64(const double* dout, const double* xhat, const double* rstd, const int32_t* graph_ptr, double* dx,
                            int B, int nmax, int H, int accumulate, dosx_stream_t stream);
/* dst[i, 0:W] (+)= sum over r < n_src with idx[r] == i, in order of r, of src[r, 0:W]  (embedding gradient) */
int dosx_index_sum_f64(const double* src, int ld_src, const int32_t* idx, int n_src, double* dst, int ld_dst, int n_dst,
                       int W, int accumulate, dosx_stream_t stream);

/* ---- float64 training step (csrc/f64_train.hip; the AdamW entry: csrc/adamw.hip) -------------------------------------------
 * The tail of train64.Trainer64's step: phonon loss + gradient and the flat AdamW update on double operands.
 *
 * dosx_loss_phonon_f64: the float64 twin of dosx_loss_phonon (main_phDOS.py:109-114), one launch, one workgroup:
 *     loss[0] = sqrt(mean (pg-y)^2) + beta sqrt(mean (ps-y)^2)           mean over the `count` = B*S elements
 *     dpg = (pg-y) / (count rmse_g),   dps = beta (ps-y) / (count rmse_s)
 *   sse (may be NULL) receives the two sums of squares.  Fixed-order reduction: two runs are bitwise equal.  IEEE sqrt and /.
 *   An RMSE of exactly 0 has no gradient direction: that branch's gradient is written as zeros, never NaN (torch's autograd
 *   gives 0/0 there; dosx_loss_phonon documents no convention for the case).  Single process only: no count_global.
 * dosx_adamw_f64: torch.optim.AdamW's single-tensor update on flat double buffers, in torch's operation order:
 *     p *= 1 - lr wd;  m += (g - m)(1 - beta1);  v = v beta2 + (1 - beta2) g g;
 *     denom = sqrt(v) / sqrt(bc2) + eps;  p -= (lr / bc1) m / denom;         bc_k = 1 - beta_k^step, in double on the host
 *   `step` is the 1-based step count (>= 1); p, g, m, v 16-byte aligned (16-byte accesses); n = 0 is a no-op.
 * Both refuse NULL operands (sse excepted), count <= 0, n < 0, step < 1 and misaligned buffers with -22 and a message. */
int dosx_loss_phonon_f64(const double* pg, const double* ps, const double* y, double beta, double* dpg, double* dps,
                         double* loss, double* sse, int count, dosx_stream_t stream);
int dosx_adamw_f64(double* p, const double* g, double* m, double* v, int64_t n, double lr, double beta1, double beta2,
                   double eps, double weight_decay, int step, dosx_stream_t stream);

/* ---- per-crystal losses (csrc/loss_rows.hip) -------------------------------------------------------------------------------
 * The objective a fused trainer is asked for with `loss=`: every crystal's own term, averaged over the crystals - what the
 * reference's drivers optimise at batch_size = 1, where the phonon model is trained (main_phDOS.py:52-55, 109-114: the RMSE of
 * ONE crystal per step) and what main_eDOS.py:111-123 spells out per crystal; MSE, MAE and Huber are the other metrics
 * utils.test / utils.test_phonon report and torch.nn.HuberLoss.  pg, ps, y, dpg, dps: [B,S] row-major; forward + gradient.
 *
 *   t = clamp_target ? max(y, 0) : y  (main_eDOS.py:113 `torch.where(y < 0, 0, y)`; phonon: clamp_target = 0),  r = p - t
 *   f(p_b):  DOSX_LOSS_RMSE  sqrt(mean_s r^2)      DOSX_LOSS_MSE  mean_s r^2      DOSX_LOSS_MAE  mean_s |r|
 *            DOSX_LOSS_HUBER mean_s h(r),  h(r) = r^2 / 2 where |r| <= delta, else delta (|r| - delta / 2)   (torch.nn.HuberLoss;
 *            |r| == delta is the quadratic branch); delta is read by this kind alone, which requires it finite and > 0
 *   l_b = f(pg_b) + beta f(ps_b);   per_crystal[b] = l_b (per_crystal may be NULL);   loss[0] = (1 / B_global) sum_b l_b
 *   dpg, dps = d loss[0] / d pg, d ps.  `B_global`: crystals in the un-sharded batch (as dosx_loss_edos).
 * One-output models: ps == NULL with dps == NULL; then l_b = f(pg_b) and beta is not read (no `ps = pg, beta = 0` scratch here).
 * A crystal whose RMSE is exactly 0 gets a zero gradient for that output, never 0 / 0 (the rule of dosx_loss_phonon_f64).  The MAE
 * subgradient at r == 0 is 0 (torch.sign).  A NaN / inf prediction - or target - reaches that crystal's l_b, loss[0] and the
 * crystal's gradient rows, and no other crystal's rows: the step guard sees it.  ONE exception, the one dosx_loss_edos has:
 * under clamp_target the clamp is fmax(y, 0), which turns a NaN TARGET into 0.
 * Deterministic: lane l of a crystal's wavefront adds the elements l, l + 64, ... in order, one wave reduction; loss[0] adds
 * the rounded shares l_b / B_global in dosx_sum's order; no atomics - two runs are bitwise equal.  kind = RMSE with clamp_target
 * and two outputs is dosx_loss_edos + dosx_sum bit for bit: dpg, dps, per_crystal[b] / B_global = its loss_partial[b], loss[0].
 * Launches: with per_crystal two (rows, then the total in one workgroup); without, one workgroup does both (same bits).
 * Both refuse with -22 and a message: a NULL pg, y, dpg or loss; ps / dps not both set or both NULL; B, S or B_global <= 0; a
 * kind outside the enumerators; DOSX_LOSS_HUBER with delta <= 0 or not finite; B * S >= 2^31. */
enum { DOSX_LOSS_RMSE = 0, DOSX_LOSS_MSE = 1, DOSX_LOSS_MAE = 2, DOSX_LOSS_HUBER = 3 };
int dosx_loss_rows(const float* pg, const float* ps, const float* y, int B, int S, int B_global, int kind, int clamp_target,
                   float beta, float delta, float* dpg, float* dps, float* per_crystal, float* loss, dosx_stream_t stream);
int dosx_loss_rows_f64(const double* pg, const double* ps, const double* y, int B, int S, int B_global, int kind,
                       int clamp_target, double beta, double delta, double* dpg, double* dps, double* per_crystal, double* loss,
                       dosx_stream_t stream);

/* ---- weighted per-crystal losses (csrc/loss_rows.hip, the same kernels under two further template flags) --------------------
 * dosx_loss_rows / _f64 with per-crystal sample weights and energy-bin weights - torch's `(w * per_sample_loss).mean()`:
 *   w        sample weights, or NULL for all ones
 *   w_index  NULL: w_b = w[b], w has B entries.  Otherwise w_b = w[w_index[b]]: w is a whole dataset's table, w_index the batch's
 *            selection (every entry inside the table: the caller's contract, nothing here knows its length) - gathered inside
 *            the loss launch, no extra launch and no [B] staging tensor.  w_index without w is refused.
 *   bin_w    [S] energy-bin weights v_s, or NULL for unweighted
 * With t and r = p - t as above:
 *   V = sum_s v_s, computed by every wavefront with the lane-strided loop and the wave reduction of the crystal sums: fixed
 *       order, bitwise run to run, no host read of bin_w.  Without bin_w: v_s = 1, V = S.
 *   f(p_b):  RMSE sqrt(sum_s v_s r^2 / V)    MSE sum_s v_s r^2 / V    MAE sum_s v_s |r| / V    HUBER sum_s v_s h(r) / V
 *   l_b = f(pg_b) + beta f(ps_b);   per_crystal[b] = l_b - NOT multiplied by w_b: it stays the crystal's own loss
 *   loss[0] = (1 / B_global) sum_b w_b l_b - divided by the crystal count, not by the sum of the weights: weights that average
 *       to 1 keep the loss scale, and B_global keeps its meaning inside an accumulation window
 *   dpg, dps = d loss[0] / d pg, d ps
 * w_b enters the gradient's coefficient as (w_b / B_global) and the share as (l_b w_b) / B_global, each product rounded: all-ones
 * w with bin_w == NULL is dosx_loss_rows bit for bit, and a power-of-two multiple of one w_b scales that crystal's rows exactly.
 * w_b == 0: the crystal's gradient rows are written as +0.0 and its share of loss[0] is exactly 0 whatever its predictions and
 * targets hold, NaN and inf included; per_crystal[b] is still its l_b and may be NaN.  Negative or non-finite weights are
 * undefined here: the owners of a weight table check them once on the host.  v_s == 0 removes bin s from sums and gradients (a
 * NaN in it too); V == 0 is the caller's error (0 / 0 everywhere) - the trainers refuse such a bin_w at construction.
 * Launches as above (two with per_crystal, one without; the same bits).  Refused with -22 and a message: everything
 * dosx_loss_rows refuses; w_index without w; w or bin_w lying inside pg, ps, y, dpg or dps. */
int dosx_loss_rows_w(const float* pg, const float* ps, const float* y, int B, int S, int B_global, int kind, int clamp_target,
                     float beta, float delta, float* dpg, float* dps, float* per_crystal, float* loss, const float* w,
                     const int32_t* w_index, const float* bin_w, dosx_stream_t stream);
int dosx_loss_rows_w_f64(const double* pg, const double* ps, const double* y, int B, int S, int B_global, int kind,
                         int clamp_target, double beta, double delta, double* dpg, double* dps, double* per_crystal, double* loss,
                         const double* w, const int32_t* w_index, const double* bin_w, dosx_stream_t stream);

/* ---- linear functionals in the per-crystal losses (csrc/loss_functional.hip) ------------------------------------------------
 * dosx_loss_rows_w / _w_f64 with a penalty on K linear functionals of the DOS next to the pointwise term: cumulative DOS (the
 * Cramer / Wasserstein-1 distances), moments, windows, heat-capacity kernels - all one table fn_w [K,S], row-major, in the
 * operands' type, F_k(p) = sum_s fn_w[k,s] p_s.  With t, r = p - t, f, beta, w_b, v_s and B_global exactly as above:
 *   u_k(p_b) = sum_s fn_w[k,s] r_s                  (= F_k(p_b) - F_k(t_b); t is the clamped target under clamp_target)
 *   h(p_b)   = (1 / K) sum_k e(u_k),   e(u) = u^2  (DOSX_FN_SQ)   or   |u|  (DOSX_FN_ABS)
 *   l_b      = f(pg_b) + beta f(ps_b) + lam (h(pg_b) + beta h(ps_b))        (one-output models: l_b = f(pg_b) + lam h(pg_b))
 *   per_crystal[b] = l_b      loss[0] = (1 / B_global) sum_b w_b l_b      dpg, dps = d loss[0] / d pg, d ps
 * The gradient of the new term on element s is  coef lam / K sum_k e'(u_k) fn_w[k,s],  coef = w_b / B_global (times beta for ps),
 * e'(u) = 2 u (SQ) or sign(u) (ABS) with sign(0) = 0 as torch.sign gives.  Bin weights v_s act on f only: the table carries its
 * own weighting.  A lower-triangular table of ones times the bin width makes SQ the Cramer distance between the two cumulative
 * DOS curves and ABS their Wasserstein-1 distance.  The rules of the entries above hold:
 *   - w_b == 0: the crystal's rows are +0.0 and its share of loss[0] exactly 0 whatever it holds; per_crystal[b] is still its l_b
 *   - a NaN / inf in crystal b reaches l_b, loss[0] and that crystal's rows, and no other crystal's rows
 *   - an all-zero table row adds nothing; lam / K is ONE number formed on the host in the operands' type, so K -> 2 K with
 *     lam -> 2 lam and K zero rows appended is the same call bit for bit
 *   - every sum runs in a fixed order that depends on (S, K) alone - not on B or on where the crystal stands in the launch
 *     (the order: the header comment of csrc/loss_functional.hip); no atomics, two runs are bitwise equal
 * One wavefront per crystal; the residuals of both outputs, u_k and the gradient sums stay in registers, the table is read from
 * global memory once per crystal, the rows are written once.  Launches as above (two with per_crystal, one without; the same
 * bits).  Limits with a table: 1 <= S <= 512, 1 <= K <= 512.  fn_w == NULL or lam == 0: the dosx_loss_rows_w kernels, bit for
 * bit (K is then not read).  Refused with -22 and a message that starts with the entry's name: everything dosx_loss_rows_w
 * refuses; fn_kind outside the enumerators; lam not finite or < 0; with a table K < 1, K > 512, S > 512, or fn_w lying inside
 * pg, ps, y, dpg or dps. */
enum { DOSX_FN_SQ = 0, DOSX_FN_ABS = 1 };
int dosx_loss_rows_fn(const float* pg, const float* ps, const float* y, int B, int S, int B_global, int kind, int clamp_target,
                      float beta, float delta, float* dpg, float* dps, float* per_crystal, float* loss, const float* w,
                      const int32_t* w_index, const float* bin_w, const float* fn_w, int K, int fn_kind, float lam,
                      dosx_stream_t stream);
int dosx_loss_rows_fn_f64(const double* pg, const double* ps, const double* y, int B, int S, int B_global, int kind,
                          int clamp_target, double beta, double delta, double* dpg, double* dps, double* per_crystal, double* loss,
                          const double* w, const int32_t* w_index, const double* bin_w, const double* fn_w, int K, int fn_kind,
                          double lam, dosx_stream_t stream);

/* ---- normalised functionals in the per-crystal losses (csrc/loss_functional.hip) ------------------------------------------
 * dosx_loss_rows_fn with the LAST K_norm rows of the table divided by one common denominator functional - a band centre or a
 * mean frequency m1 / m0, C_V(T) per mode, the cumulative curve of the DOS as a shape.  t, f, beta, w_b, v_s, B_global, e, lam
 * and K exactly as above; the table fn_w [K,S] is unchanged, its first K - K_norm rows are the plain rows of above.  New
 * operands: fn_den [S] in the operands' type, den_floor > 0 and K_norm.
 *   D(x)   = sum_s fn_den[s] x_s          D+(x) = max(D(x), den_floor)
 *   plain row k:       u_k(p) = F_k(p) - F_k(t)
 *   normalised row k:  u_k(p) = F_k(p) / D+(p)  -  F_k(t) / D+(t)
 *   h(p)   = (1 / K) sum_k e(u_k)         l_b = f(pg_b) + beta f(ps_b) + lam (h(pg_b) + beta h(ps_b))
 * (t is the clamped target under clamp_target.)  For a normalised row, with q_k = F_k(p) / D+(p),
 *   d u_k / d p_s = fn_w[k,s] / D+ - [D(p) > den_floor] q_k fn_den[s] / D+ :
 * a floored denominator is a constant (torch's clamp(min=) subgradient away from equality).  The gradient of the term on
 * element s is  coef lam / K ( sum_k c_k fn_w[k,s] - [D > den_floor] A fn_den[s] ),  c_k = e'(u_k) on plain rows and
 * e'(u_k) / D+ on normalised rows,  A = sum_{k normalised} e'(u_k) q_k / D+.  A purely normalised objective leaves the scale of
 * the prediction free (sum_s p_s d/dp_s of such a term is 0 where D > den_floor): the pointwise term, or a plain row, carries it.
 * The rules of dosx_loss_rows_fn hold: a NaN stays inside its crystal, w_b == 0 writes +0.0 rows, per_crystal[b] = l_b unweighted,
 * fixed summation orders that depend on (S, K, K_norm) alone (the header comment of csrc/loss_functional.hip), no atomics, the
 * same launches and limits (S, K <= 512).  K_norm == 0 (fn_den is then not read), fn_w == NULL or lam == 0: dosx_loss_rows_fn's
 * own launches under this entry's name, bit for bit.  Refused with -22 and a message that starts with the entry's name:
 * everything dosx_loss_rows_fn refuses; K_norm < 0, or K_norm > K with a table; K_norm > 0 with fn_den == NULL; den_floor not
 * finite or <= 0; fn_den lying inside pg, ps, y, dpg or dps.
 *
 * dosx_loss_rows_fn_norm_desc / _desc_f64: the same call - the same checks under their own names, the same kernels - with the
 * table's side in a DosxFnNorm, read on the host when the call is issued.  These are the forms a recorded step holds: a DosxCall
 * carries 19 integer-class arguments, the entries above have 21.  lam and den_floor are converted to the operands' type;
 * reserved is not read.  A NULL descriptor is refused. */
typedef struct DosxFnNorm {
  const void* fn_w;    /* [K,S] in the operands' type, or NULL */
  const void* fn_den;  /* [S] in the operands' type; may be NULL with K_norm == 0 */
  int32_t K, K_norm, fn_kind, reserved;
  double lam, den_floor;
} DosxFnNorm;
int dosx_loss_rows_fn_norm(const float* pg, const float* ps, const float* y, int B, int S, int B_global, int kind,
                           int clamp_target, float beta, float delta, float* dpg, float* dps, float* per_crystal, float* loss,
                           const float* w, const int32_t* w_index, const float* bin_w, const float* fn_w, int K, int fn_kind,
                           float lam, const float* fn_den, int K_norm, float den_floor, dosx_stream_t stream);
int dosx_loss_rows_fn_norm_f64(const double* pg, const double* ps, const double* y, int B, int S, int B_global, int kind,
                               int clamp_target, double beta, double delta, double* dpg, double* dps, double* per_crystal,
                               double* loss, const double* w, const int32_t* w_index, const double* bin_w, const double* fn_w,
                               int K, int fn_kind, double lam, const double* fn_den, int K_norm, double den_floor,
                               dosx_stream_t stream);
int dosx_loss_rows_fn_norm_desc(const float* pg, const float* ps, const float* y, int B, int S, int B_global, int kind,
                                int clamp_target, float beta, float delta, float* dpg, float* dps, float* per_crystal, float* loss,
                                const float* w, const int32_t* w_index, const float* bin_w, const DosxFnNorm* fn,
                                dosx_stream_t stream);
int dosx_loss_rows_fn_norm_desc_f64(const double* pg, const double* ps, const double* y, int B, int S, int B_global, int kind,
                                    int clamp_target, double beta, double delta, double* dpg, double* dps, double* per_crystal,
                                    double* loss, const double* w, const int32_t* w_index, const double* bin_w,
                                    const DosxFnNorm* fn, dosx_stream_t stream);

/* ---- guarded optimizer step (csrc/step_guard.hip; the guarded AdamW entries: csrc/adamw.hip) ------------------------------
 * What a fused trainer has in place of `clip_grad_norm_` and of a GradScaler-style "skip if non-finite": one statistics launch
 * over the flat gradient, behind the recorded program and in front of the AdamW launch, and an AdamW that reads its verdict
 * from device memory.  No host read anywhere in the step.
 *
 * DosxStepGuard: the device-resident record, one per trainer, 16-byte aligned, zero-initialised by its owner.
 *   this step:  sumsq = sum of g[i]^2 over the FINITE elements (accumulated in double for both dtypes), norm = sqrt(sumsq),
 *               clip = max_norm / (norm + 1e-6) where that is < 1, else exactly 1.0 (also without a max_norm) - torch's
 *               clip_grad_norm_ coefficient; n_bad / first_bad = count and lowest flat index of the non-finite elements
 *               (first_bad = -1: none); skip = 0 / 1; reason = DOSX_GUARD_* bits; step_size / bc2_scale = the two
 *               bias-correction scalars the guarded AdamW applies; t = the AdamW time they stand for.
 *   sticky (until the owner zeroes them): applied / skipped = steps counted since then; first_skip_step / first_skip_reason /
 *               first_skip_bad = attempt number, reason and first_bad of the FIRST skipped step.
 * reason: NONFINITE - an element with all exponent bits set (NaN, +-inf); OVERFLOW - sumsq itself is not finite although every
 *   element is (float64 only: an element of magnitude beyond ~1e154 squares to inf) - such a gradient is treated like a
 *   non-finite one; STALLED - exchange_status[0] != 0 (the sticky stall status of the column-split exchanges above: every step
 *   is skipped until the owner has cleared it).
 *
 * dosx_grad_guard_f32 / _f64: one launch over g[0, n).  DOSX_GUARD_THREADS threads; min(ceil(n / (16 / sizeof(T)) /
 *   DOSX_GUARD_THREADS), DOSX_GUARD_MAX_BLOCKS) workgroups (at least 1: dosx_grad_guard_blocks) that stride over the 16-byte
 *   vectors, the < 16-byte tail goes to the first threads of the grid one element each.  Each workgroup publishes {sum of
 *   squares, bad count, first bad} to its slot of the workspace slab and draws a ticket (csrc/common.h: publish / ticket /
 *   last arriver); the workgroup that draws the last ticket reads all slots back - thread t the slots t, t + 256, ... in rising
 *   order, then a fixed tree over the threads - finishes the record and zeroes the counter.  Nobody waits for anybody: no poll,
 *   nothing that can stall.  The grid and every summation order are functions of n alone: the record is bitwise run to run.
 *   max_norm < 0: no clipping (clip = 1.0).  exchange_status: NULL or the device address dosx_exchange_status_address gives.
 *   step: the caller's 1-based ATTEMPT count; lr, beta1, beta2 as the unguarded AdamW entry takes them.  With skipped == 0 the
 *   record receives the bias-correction scalars the unguarded entry computes on the host for `step` (computed by the same
 *   host expressions: a guarded run in which nothing trips is bit for bit the unguarded run); otherwise they are recomputed on
 *   the device in double with pow() for t = step - skipped: a skipped step does not advance AdamW's time.
 *   fp32: step_size = (float)(lr / bc1), bc2_scale = (float)(1 / sqrt(bc2)); float64: step_size = lr / bc1, bc2_scale = sqrt(bc2).
 *   workspace: DOSX_GUARD_WORKSPACE_BYTES of 16-byte aligned device memory, zeroed once by its owner, private to one stream.
 * dosx_adamw_guarded / _f64: dosx_adamw (grad_scale = clip) / dosx_adamw_f64 (on g * clip) with skip, clip and the two scalars read
 *   from the record by every thread (plain uniform loads); skip != 0 returns before any store.  g is never written.
 * All four refuse NULL operands, n < 0, step < 1, a NaN max_norm and buffers off a 16-byte boundary with -22 and a message. */
enum { DOSX_GUARD_NONFINITE = 1, DOSX_GUARD_OVERFLOW = 2, DOSX_GUARD_STALLED = 4 };
#define DOSX_GUARD_THREADS 256
#define DOSX_GUARD_MAX_BLOCKS 256
#define DOSX_GUARD_WORKSPACE_BYTES 6208
typedef struct DosxStepGuard {
  double sumsq, norm, clip;
  double step_size, bc2_scale;
  int64_t n_bad, first_bad;
  int64_t first_skip_bad;
  int32_t skip, reason, t;
  int32_t applied, skipped, first_skip_step, first_skip_reason;
  int32_t reserved;
} DosxStepGuard;
int dosx_grad_guard_blocks(int64_t n, int elem_bytes);
/* the device address of the four status words of dosx_exchange_status on the current device, written to *address_out (HOST memory) */
int dosx_exchange_status_address(unsigned long long* address_out);
int dosx_grad_guard_f32(const float* g, int64_t n, double max_norm, const int32_t* exchange_status, float lr, float beta1,
                        float beta2, int step, void* guard, void* workspace, dosx_stream_t stream);
int dosx_grad_guard_f64(const double* g, int64_t n, double max_norm, const int32_t* exchange_status, double lr, double beta1,
                        double beta2, int step, void* guard, void* workspace, dosx_stream_t stream);
int dosx_adamw_guarded(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                       float weight_decay, const void* guard, dosx_stream_t stream);
int dosx_adamw_guarded_f64(double* p, const double* g, double* m, double* v, int64_t n, double lr, double beta1, double beta2,
                           double eps, double weight_decay, const void* guard, dosx_stream_t stream);

/* ---- AdamW with parameter groups (instantiations of the ungrouped entries' kernel and launcher: csrc/adamw.hip) -------------
 * torch.optim.AdamW's param groups on the flat buffers: every DOSX_ADAMW_GROUP_CHUNK elements of the flat buffer carry one
 * byte that names their group, each group has its own lr and weight_decay; beta1, beta2, eps and the step count are shared.
 *
 * chunk_group: DEVICE memory, n / DOSX_ADAMW_GROUP_CHUNK bytes (uint8); byte c is the group of the elements [64c, 64c + 64).
 *   Built once per layout, only read here.  A byte >= n_groups cannot be seen from the host without a read-back: the kernel
 *   steps such a chunk as group 0.
 * groups: HOST memory, read during the call (nothing of it is referenced afterwards).  lr[k], weight_decay[k] for k < n_groups;
 *   both arrays have DOSX_ADAMW_MAX_GROUPS entries.
 * Element arithmetic: that of dosx_adamw / dosx_adamw_f64, the same expressions in the same order; only decay and step_size are
 *   per group, computed on the host by the ungrouped entries' expressions -
 *   fp32: step_size_k = (float)((double)(float)lr_k / bc1), decay_k = 1.f - (float)lr_k * (float)wd_k; float64: lr_k / bc1,
 *   1.0 - lr_k * wd_k.  A launch over a run of chunks of group k is bit for bit the ungrouped launch over it with (lr_k, wd_k).
 * Guarded forms: as dosx_adamw_guarded / _f64 - skip != 0 returns before any store, clip stands where grad_scale stood (fp32) /
 *   multiplies g (float64), bc2_scale is the record's.  The record holds ONE step size, so the per-group one is the host's
 *   step_size_k when the record's t equals `step` (nothing skipped so far: the caller's 1-based attempt count IS AdamW's time),
 *   else it is recomputed on the device by dosx_grad_guard's expression, bc1 = 1 - pow(beta1, (double)t), lr_k / bc1 (rounded
 *   through float for fp32): what dosx_grad_guard_* writes when called with lr_k.
 * Grid: the ungrouped entry's (16-byte vectors, 256 threads, the same cap, grid-stride); a vector never straddles a chunk.
 * All four refuse with -22 and a message: NULL operands, n < 0, step < 1, n % DOSX_ADAMW_GROUP_CHUNK != 0, n_groups outside
 *   [1, DOSX_ADAMW_MAX_GROUPS], a NaN or negative lr / weight_decay of a used group, p / g / m / v (or the record) off a
 *   16-byte boundary.  n = 0 is a no-op. */
#define DOSX_ADAMW_MAX_GROUPS 16
#define DOSX_ADAMW_GROUP_CHUNK 64
typedef struct DosxAdamWGroups {
  int32_t n_groups, reserved;
  double lr[16], weight_decay[16];
} DosxAdamWGroups;
int dosx_adamw_grouped(float* p, const float* g, float* m, float* v, int64_t n, const void* chunk_group,
                       const DosxAdamWGroups* groups, float beta1, float beta2, float eps, int step, float grad_scale,
                       dosx_stream_t stream);
int dosx_adamw_grouped_f64(double* p, const double* g, double* m, double* v, int64_t n, const void* chunk_group,
                           const DosxAdamWGroups* groups, double beta1, double beta2, double eps, int step,
                           dosx_stream_t stream);
int dosx_adamw_grouped_guarded(float* p, const float* g, float* m, float* v, int64_t n, const void* chunk_group,
                               const DosxAdamWGroups* groups, float beta1, float beta2, float eps, int step, const void* guard,
                               dosx_stream_t stream);
int dosx_adamw_grouped_guarded_f64(double* p, const double* g, double* m, double* v, int64_t n, const void* chunk_group,
                                   const DosxAdamWGroups* groups, double beta1, double beta2, double eps, int step,
                                   const void* guard, dosx_stream_t stream);

/* ---- AdamW that also keeps an exponential moving average of the parameters (the EMA instantiations: csrc/adamw.hip) ---------
 * What torch.optim.swa_utils.AveragedModel with an EMA multi_avg_fn, torch-ema and timm's ModelEma do in a second pass over the
 * parameters: here the thread that holds the new parameter p' in registers also updates the average,
 *     ema' = ema + (p' - ema) (1 - d_t)        fp32: fmaf(fmaf(p', 1.f, -ema), omd, ema); float64: fma(p' - ema, omd, ema)
 * with omd = (T)1 - (T)d_t: the expression of the first-moment update with g := p', m := ema, 1 - beta1 := omd (vector body and
 * scalar tail alike), so the bits of ema' are those the plain entry leaves in m for these operands.  p', m', v' are bit for bit
 * those of the launch without the average; ema is read and written with the same 16-byte accesses, nothing else is.
 * Traffic: 36 B (fp32) / 72 B (float64) per parameter against 28 / 56.
 *
 * DosxAdamWEma (HOST memory, read during the call): ema = DEVICE buffer laid out like p, at least n elements, 16-byte aligned,
 *   not p; decay in [0, 1); warmup != 0: d_t = min(decay, (1 + t) / (10 + t)), else d_t = decay, with t = T_adamw - t0 - AdamW's
 *   time (`step` of the unguarded forms, the record's t of the guarded ones: a skipped step does not advance the warm-up) less
 *   t0, AdamW's time when averaging began.  d_t is evaluated in double and rounded once to the buffers' type, on the host for
 *   `step` and - guarded, when the record's t is not `step` - on the device by the same function (dosx_adamw_ema_decay gives
 *   it: elem_bytes 4 -> rounded through float, else double; t as above).
 * dosx_adamw_ema / _f64: ONE entry per type for the four forms.  chunk_group and groups: both NULL - one (lr, weight_decay), the
 *   arguments - or both given - dosx_adamw_grouped*'s operands, lr and weight_decay are not read.  guard: NULL, or the record of
 *   dosx_grad_guard_* - then the launch is dosx_adamw_guarded* / _grouped_guarded*'s (grad_scale is not read, `step` is the attempt
 *   count the guard was given); skip != 0 returns before any store, the one to ema included.
 * Refused with -22 and a message: what the form in question refuses (n = 0 is a no-op behind the checks), a chunk map without
 *   groups or the reverse, a NULL descriptor or ema, ema off a 16-byte boundary, ema overlapping p, decay NaN or outside [0, 1),
 *   t0 < 0 or t0 >= step.
 *
 * dosx_swap_buffers: a[0, bytes) <-> b[0, bytes) in one launch (16-byte vectors, DOSX_SWAP_THREADS threads, at most
 *   DOSX_SWAP_MAX_BLOCKS workgroups that stride over the vectors) - what puts the average in the parameters' place and back;
 *   blind to the element type.  Refuses NULL, bytes < 0, bytes % 16 != 0, buffers off a 16-byte boundary and buffers that
 *   overlap with -22 and a message; bytes = 0 is a no-op. */
#define DOSX_SWAP_THREADS 256
#define DOSX_SWAP_MAX_BLOCKS 2048
typedef struct DosxAdamWEma {
  void* ema;
  double decay;
  int32_t warmup, t0;
} DosxAdamWEma;
int dosx_adamw_ema(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                   float weight_decay, int step, float grad_scale, const void* chunk_group, const DosxAdamWGroups* groups,
                   const void* guard, const DosxAdamWEma* ema, dosx_stream_t stream);
int dosx_adamw_ema_f64(double* p, const double* g, double* m, double* v, int64_t n, double lr, double beta1, double beta2,
                       double eps, double weight_decay, int step, const void* chunk_group, const DosxAdamWGroups* groups,
                       const void* guard, const DosxAdamWEma* ema, dosx_stream_t stream);
double dosx_adamw_ema_decay(double decay, int warmup, int t, int elem_bytes);
int dosx_swap_buffers(void* a, void* b, int64_t bytes, dosx_stream_t stream);

/* ---- gradient accumulation over the batches of one optimizer step (csrc/grad_accumulate.hip) ---------------------------------
 * What a torch loop gets from calling backward() on several batches before one optimizer.step(): the backward program
 * OVERWRITES the flat gradient, so a fused trainer adds the micro-batches' gradients with one launch behind each program
 * (train.py: step_accumulate).
 *   dst[i] = a[i] + b[i] for i < n;  b == NULL: dst[i] = a[i] - the first batch of a window: dst is never read, so an
 *   accumulator needs no zeroing and a stale NaN in it cannot reach a window.
 *   dst may be exactly a or exactly b; any other overlap of dst with a or b is refused (a and b are only read).
 *   The scalar triple does the same for one element, by one thread: sdst[0] = sa[0] + sb[0], or sdst[0] = sa[0] when sb == NULL
 *   (whatever b is) - the window's loss, without a torch kernel or a host read.  All three NULL: skipped.  sdst may be sa or sb;
 *   no scalar may lie inside dst[0, n), nor sdst inside a[0, n) / b[0, n).
 * One kernel template over the element type: 16-byte loads and stores (float4 / double2), DOSX_ACCUM_THREADS threads, min(ceil(n /
 * (16 / sizeof(T)) / DOSX_ACCUM_THREADS), DOSX_ACCUM_MAX_BLOCKS) workgroups (at least 1) that stride over the vectors; the
 * < 16-byte tail goes to the first threads of the grid, one element each.  Every element is ONE IEEE add: no multiply, so nothing
 * to contract, and no atomics - two runs are bitwise equal, and the result is bit for bit `a + b` of torch on the same device.
 * A NaN or an inf passes through like any other value (the step guard is what judges the sum); the copy form copies bits (-0.0).
 * Both refuse with -22 and a message that starts with the entry's name, before any launch: a NULL dst or a; n < 0; dst, a or b
 * off a 16-byte boundary; a partial overlap; an sdst without sa or an sa without sdst (an sb without them); a scalar off its
 * element's alignment or inside the vectors as above.  n == 0 returns 0 without a launch (the scalar triple is then not
 * carried out either). */
#define DOSX_ACCUM_THREADS 256
#define DOSX_ACCUM_MAX_BLOCKS 2048
int dosx_grad_accumulate(float* dst, const float* a, const float* b, int64_t n, float* sdst, const float* sa, const float* sb,
                         dosx_stream_t stream);
int dosx_grad_accumulate_f64(double* dst, const double* a, const double* b, int64_t n, double* sdst, const double* sa,
                             const double* sb, dosx_stream_t stream);

/* ---- evaluation metrics (csrc/eval.hip) -----------------------------------------------------------------------------------
 * utils.py:76-89 / :127-139 evaluated one crystal at a time (what the reference computes at batch_size = 1).
 * pred, y: [B,S] rows with unit inner stride, rows S apart.  clamp0 != 0: both are clamped at 0 first (utils.py:74-76).
 * metrics [B,4] = rmse, mse, mae, r2 of each row, accumulated in float64:
 *   mse = sum (y-p)^2 / S,  rmse = sqrt(mse),  mae = sum |p-y| / S,
 *   r2 = 1 - sum (y-p)^2 / sum (y - mean(y))^2   (mean first, then the squares: two passes, no E[y^2]-E[y]^2)
 * r2 of a row with a constant target is what IEEE division gives (-inf, or NaN when the error is 0 too), like evaluate.r2 on
 * that row - as far as the row's mean is exact in float64 (sum / S of S equal numbers is, when the partial sums are).
 * pred_out / y_out: NULL, or [B,S] rows that receive the (clamped) values - the preds / y that utils.test concatenates; they may
 * be pred / y themselves, not each other's input.
 * One wavefront per row, every sum in a fixed order that depends on S alone: a row's result does not depend on B or on where
 * the row stands in the launch.  B = 0 is a no-op; S < 1, B < 0 and NULL pred / y / metrics are refused with -22 and a message. */
int dosx_eval_metrics(const float* pred, const float* y, int B, int S, int clamp0, double* metrics, float* pred_out, float* y_out,
                      dosx_stream_t stream);
int dosx_eval_metrics_f64(const double* pred, const double* y, int B, int S, int clamp0, double* metrics, double* pred_out,
                          double* y_out, dosx_stream_t stream);

/* ---- evaluation functionals (csrc/loss_functional.hip) ----------------------------------------------------------------------
 * The integrated quantities a DOS is used through - cumulative DOS, band centre and width, states in a window, C_V(T) - of the
 * predictions and targets evaluate.test_per_crystal leaves on the device: out [B,2,K] float64 holds F_k(pred_b) scale_b in
 * out[b,0,k] and F_k(y_b) scale_b in out[b,1,k], F_k(p) = sum_s fn_w[k,s] p_s with fn_w [K,S] row-major in the operands' type.
 * scale: NULL (1), or [B] float64 - e.g. the eDOS y_max that undoes the target's normalisation.  pred / y are taken as given.
 * Products and sums in float64, one wavefront per row: lane l adds its elements l, l + 64, ... in rising order, one wave
 * reduction per k - a fixed order that depends on (S, K) alone.  Any S, K >= 1; B = 0 is a no-op; S < 1, K < 1, B < 0 and a NULL
 * pred / y / fn_w / out are refused with -22 and a message. */
int dosx_eval_functionals(const float* pred, const float* y, int B, int S, const double* scale, const float* fn_w, int K,
                          double* out, dosx_stream_t stream);
int dosx_eval_functionals_f64(const double* pred, const double* y, int B, int S, const double* scale, const double* fn_w, int K,
                              double* out, dosx_stream_t stream);

const char* dosx_last_error(void);
int dosx_version(void);

#ifdef __cplusplus
}
#endif
#endif /* DOSX_H */
