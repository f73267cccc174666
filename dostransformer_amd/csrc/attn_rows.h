// The ROW phases of the crystal-aligned attention tile (<= 64 keys of one crystal per workgroup), shared by the fused encoder layer
// (ffn.hip: ffn_att_tile / ffn_att_bwd_tile, hidden <= 128) and the stand-alone kernels (attention_aligned.hip, hidden <= 256).
// One QUARTER wave owns a query row: lane q16 holds the float4 columns 4 q16 + 64 k, k < NG (on[k]: the column exists), and key
// j = q16 + 16 jj, jj < 4; reductions over the row are row16_sum / row16_max.  The matrix phases between them (scores, P.K, dP, dq,
// the key-gradient share) differ per kernel and stay there, and so does everything that orders a tile: no phase here holds a
// barrier, a stamp, a prefetch or the key staging.  They take plain pointers - `*_row` is the row's first element, in LDS or in
// global memory - and values; a caller sums its split-K partial score tiles itself, in its own order (forward: into v[4]; backward:
// dp(j), a callable, so that the sums stay where the kernels formed them), and reads dO from where it keeps it (go(k)).
// A phase is here only if it cost no instantiation of either kernel a VGPR, scratch or an occupancy step.  Three loops did and
// stay written out in both kernels, each with a comment at its site: forward A's q store (its statistics are dosx_row16_stats),
// forward E's x1 loop, backward a; and all of ffn.hip's ffn_att_row (the <= 16-key per-row form, at 255 VGPRs).
#pragma once
#include "common.h"
#include "rowstat.h"

// ---- forward C: exact fp32 softmax over the row's nk live scores v (-INFINITY beyond nk); the un-dropped P -> probs (rows of the
// data only: rv), P o mask -> s_row (zeros up to NkP: the padded keys of the second product).  Returns sum(P o mask). ----
template <bool KP>
__device__ __forceinline__ float dosx_att_softmax_row(float (&v)[4], const int nk, const int Nk, const int NkP, const int q16,
                                                      const float* __restrict__ mask, float* __restrict__ probs, const size_t prow,
                                                      const bool rv, float* __restrict__ s_row) {
  float mx = -INFINITY;
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) mx = fmaxf(mx, v[jj]);
  mx = row16_max(mx);
  float sum = 0.f;
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    const float e = (q16 + 16 * jj) < nk ? expf(v[jj] - mx) : 0.f;
    v[jj] = e;
    sum += e;
  }
  const float inv = dosx_softmax_inv<KP>(row16_sum(sum));
  float ps = 0.f;
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    const int j = q16 + 16 * jj;
    if (j >= NkP) continue;
    float pm = 0.f;
    if (j < Nk) {
      const float pr = v[jj] * inv;                    // (0 beyond nk)
      pm = (mask && (!KP || j < nk)) ? pr * mask[prow + j] : pr;
      if (rv) probs[prow + j] = pr;                    // the un-dropped P (the backward reads it)
    }
    s_row[j] = pm;
    ps += pm;
  }
  return mask ? row16_sum(ps) : dosx_psum_one<KP>(nk);
}

// ---- forward E, behind the caller's x1 = O o g0 + b0 sum(P o mask) + x and dosx_row16_stats of it: the LayerNorm-1 row
// y = (x1 - mean) rstd g + b -> y_row ----
template <int NG>
__device__ __forceinline__ void dosx_att_ln_row(const float4 (&x)[NG], const bool (&on)[NG], const float mean, const float rstd,
                                                const float4 (&g)[NG], const float4 (&b)[NG], float* __restrict__ y_row,
                                                const int q16) {
#pragma unroll
  for (int k = 0; k < NG; ++k) {
    if (!on[k]) continue;
    const float4 v = x[k];
    st4(y_row + q16 * 4 + 64 * k,
        make_float4((v.x - mean) * rstd * g[k].x + b[k].x, (v.y - mean) * rstd * g[k].y + b[k].y,
                    (v.z - mean) * rstd * g[k].z + b[k].z, (v.w - mean) * rstd * g[k].w + b[k].w));
  }
}

// ---- backward c: dp(j) = the row's dP of live key j, the caller's partial tiles summed in its own order; dP' = (dP + cq) o M with
// a dropout mask; dS = P o (dP' - sum_j P dP') scale -> ss_row, P' = P o M -> ps_row (zeros beyond nk / the data, up to NkP).
// (ss_row may be the row dp(j) reads: in place).  QO (query-only backward: no key gradient is wanted): P' feeds only the
// dK + dV share and is not stored, ps_row is not touched ----
template <bool QO = false, class DP>
__device__ __forceinline__ void dosx_att_bwd_ds_row(DP&& dp, const float (&pr)[4], const float (&mk)[4], const bool drop,
                                                    const float cq, const int nk, const int NkP, const bool rv, const float scale,
                                                    const int q16, float* ss_row, float* ps_row) {
  float d[4], dot = 0.f;
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    const int j = q16 + 16 * jj;
    float t = 0.f;
    if (j < nk) t = dp(j);
    if (drop) t = (t + cq) * mk[jj];
    if (j < nk) dot += pr[jj] * t;
    d[jj] = t;
  }
  dot = row16_sum(dot);
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    const int j = q16 + 16 * jj;
    if (j >= NkP) continue;
    const bool v = j < nk && rv;
    ss_row[j] = v ? pr[jj] * (d[jj] - dot) * scale : 0.f;
    if constexpr (!QO) ps_row[j] = v ? pr[jj] * mk[jj] : 0.f;
  }
}

// ---- backward e: dq_ln = (dS . K^) o g0 (dq_row); LayerNorm-0 backward + the residual dO (go(k)) -> dx_row; the row's dgamma0 /
// dbeta0 terms -> pg / pb (ACC: added to them, the caller keeps them across tiles); Ql = LN0(x) g0 + b0 -> ql_row (zeros beyond
// the data); QO (query-only backward): Ql feeds only the dK + dV share and is not stored, ql_row is not touched ----
template <int NG, bool ACC, bool QO = false, class GO>
__device__ __forceinline__ void dosx_att_bwd_ln0_row(const float* dq_row, const float4 (&xr)[NG], const bool (&on)[NG],
                                                     const float4 (&g0)[NG], const float4 (&b0)[NG], const float mean,
                                                     const float rstd, const float invH, const bool rv, GO&& go, float* dx_row,
                                                     float* ql_row, const int q16, float4 (&pg)[NG], float4 (&pb)[NG]) {
  float4 d[NG], xh[NG];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int k = 0; k < NG; ++k) {
    d[k] = f4zero(); xh[k] = f4zero();
    if (!(on[k] && rv)) continue;
    float4 dd = ld4(dq_row + q16 * 4 + 64 * k);
    dd = make_float4(dd.x * g0[k].x, dd.y * g0[k].y, dd.z * g0[k].z, dd.w * g0[k].w);
    const float4 xv = xr[k];
    const float4 h = make_float4((xv.x - mean) * rstd, (xv.y - mean) * rstd, (xv.z - mean) * rstd, (xv.w - mean) * rstd);
    d[k] = dd; xh[k] = h;
    const float4 tg = make_float4(dd.x * h.x, dd.y * h.y, dd.z * h.z, dd.w * h.w);
    if constexpr (ACC) { pg[k] = f4add(pg[k], tg); pb[k] = f4add(pb[k], dd); }
    else { pg[k] = tg; pb[k] = dd; }
    const float4 dh = make_float4(dd.x * g0[k].x, dd.y * g0[k].y, dd.z * g0[k].z, dd.w * g0[k].w);
    s1 += (dh.x + dh.y) + (dh.z + dh.w);
    s2 += (dh.x * h.x + dh.y * h.y) + (dh.z * h.z + dh.w * h.w);
  }
  s1 = row16_sum(s1) * invH; s2 = row16_sum(s2) * invH;
#pragma unroll
  for (int k = 0; k < NG; ++k) {
    if (!on[k]) continue;
    const float4 dd = d[k], h = xh[k];
    if (rv) {
      const float4 r = go(k);                          // (this row's dO: the residual path)
      st4(dx_row + q16 * 4 + 64 * k,
          make_float4(rstd * (dd.x * g0[k].x - s1 - h.x * s2) + r.x, rstd * (dd.y * g0[k].y - s1 - h.y * s2) + r.y,
                      rstd * (dd.z * g0[k].z - s1 - h.z * s2) + r.z, rstd * (dd.w * g0[k].w - s1 - h.w * s2) + r.w));
    }
    if constexpr (!QO)
      st4(ql_row + q16 * 4 + 64 * k,
          rv ? make_float4(h.x * g0[k].x + b0[k].x, h.y * g0[k].y + b0[k].y, h.z * g0[k].z + b0[k].z, h.w * g0[k].w + b0[k].w)
             : f4zero());
  }
}
