// The key-gradient reduction of the attention backward (DosxAttn / DosxFfnBwd: dkv_part + dkv_cnt), ONE copy for its three users:
//   attention.hip          attn_dkv_reduce_kernel (two-launch form) and the fused tail of attn_bwd_dq_stream_kernel
//   attention_aligned.hip  the last arriver of attn_al_bwd_kernel
//   ffn.hip                the last arriver of ffn_att_bwd_tile (ffn_bwd_kernel<.., ATT = 2>)
// Every query-side workgroup leaves its SHARE of a key crystal's gradient dK^ = P'^T.dO + dS^T.Q in a [Nk, H] slot of dkv_part:
// share (i, w), i < rep = Bq / Bk, w < wpc, of key crystal bk sits in slot ((bk + i Bk) nqt + w) (nqt slots per query batch entry;
// wpc = nqt where every query tile publishes one, fewer where a workgroup keeps its share across its tiles).  The reduction:
//   d[j]               = sum of the rep * wpc shares of key row j in (i, w) order, U of them requested per round - the loads of a
//                        ragged last round are clamped to the last share and masked out of the sum (fixed order: deterministic)
//   dkvhat[j]        (+)= d[j] o gamma0                      (+= with dkv_accumulate; the key-side chain rule)
//   partials_kv[bk][g] = [ sum_{j in g} d[j] o k^[j] | sum_{j in g} d[j] ]      per group g of 16 key rows, rows added in order
// KP (per-crystal key counts, key_ptr): a row past the crystal's own count is no key - nothing was published for it and nothing is
// fetched; it adds zeros to its group's sums and, without dkv_accumulate, its dkvhat row is zero-filled.
// One quarter wave (16 lanes) per key row, lane q owns columns 4q + 64k (k < NCB); a call covers NT / 16 * RPS rows from group
// grp0's first.  The forms agree bitwise wherever their shares do: "interchangeable per layer", "bitwise the two-launch result".
#pragma once
#include "common.h"

struct DkvReduce {
  const float *kvhat, *gamma0, *dkv_part;
  float *dkvhat, *partials_kv;
  const int32_t* key_ptr;
  int H, Nk, Bq, Bk, dkv_accumulate;
};
__device__ __forceinline__ DkvReduce dkv_reduce_operands(const DosxAttn& a) {
  return {a.kvhat, a.gamma0, a.dkv_part, a.dkvhat, a.partials_kv, a.key_ptr, a.H, a.Nk, a.Bq, a.Bk, a.dkv_accumulate};
}

// NCB: 64-column blocks per row (H <= 64 NCB); HC: H at compile time, 0 = a.H; U: shares requested per round; RPS: key rows per
// quarter-wave slot (rows slot, slot + NT / 16, ..: their loads go out together); NT: the participating threads - tid runs over
// 0 .. NT - 1 and ALL of them call (contains a barrier); SC1: the shares were published by other workgroups of THIS launch, so
// every load of them bypasses this CU's L1 (common.h: the publish / ticket protocol).
// Pp: [NT / 16 * RPS][2 * 64 NCB] floats of LDS.
template <int NCB, int HC, int U, bool KP, int RPS, int NT, bool SC1>
__device__ __forceinline__ void dosx_dkv_reduce(const DkvReduce& a, const int nqt, const int wpc, const int bk, const int grp0,
                                                float* __restrict__ Pp, const int tid) {
  constexpr int HP = 64 * NCB, NSLOT = NT / 16, ROWS = NSLOT * RPS;
  static_assert(ROWS % 16 == 0 && (RPS == 1 || RPS == 2) && (NT == 256 || NT == 512), "whole 16-row groups");
  const int q16 = tid & 15, slot = tid >> 4, j0 = grp0 * 16;
  const int H = HC ? HC : a.H, Nk = a.Nk, rep = a.Bq / a.Bk, ngroups = (Nk + 15) / 16;
  const int nk = dosx_live_keys<KP>(a.key_ptr, bk, Nk);  // (KP: a row past the crystal's own keys is no key - zeros)
  const int np = (KP && j0 + slot >= nk) ? 0 : rep * wpc;   // (KP: none of this slot's rows is a key - nothing to sum)
  const size_t pstride = (size_t)Nk * H;                 // between consecutive slots of dkv_part
  const __amdgpu_buffer_rsrc_t rP = __builtin_amdgcn_make_buffer_rsrc((void*)a.dkv_part, 0, 0x7fffffff, 0x00020000);
  float4 g0[NCB], d[RPS][NCB], kh[RPS][NCB], d0[RPS][NCB];
  bool jv[RPS];
  size_t krow[RPS];
#pragma unroll
  for (int k = 0; k < NCB; ++k) g0[k] = ld4(a.gamma0 + ((q16 * 4 + 64 * k) < H ? (q16 * 4 + 64 * k) : 0));
#pragma unroll
  for (int p = 0; p < RPS; ++p) {
    const int j = j0 + slot + NSLOT * p;
    jv[p] = j < nk;
    krow[p] = ((size_t)(jv[p] ? j : 0) * a.Bk + bk) * H;
#pragma unroll
    for (int k = 0; k < NCB; ++k) {
      const int c = q16 * 4 + 64 * k, cc = c < H ? c : 0;
      kh[p][k] = (!KP || jv[p]) ? ld4(a.kvhat + krow[p] + cc) : f4zero();
      d0[p][k] = (a.dkv_accumulate && (!KP || jv[p])) ? ld4(a.dkvhat + krow[p] + cc) : f4zero();
      d[p][k] = f4zero();
    }
  }
  for (int p0 = 0; p0 < np; p0 += U) {
    float4 v[RPS][U][NCB];
#pragma unroll
    for (int p = 0; p < RPS; ++p)
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int pi = min(p0 + u, np - 1), i = pi / wpc, ww = pi - i * wpc;
        const size_t off = ((size_t)(bk + i * a.Bk) * nqt + ww) * pstride + (size_t)(jv[p] ? j0 + slot + NSLOT * p : 0) * H;
#pragma unroll
        for (int k = 0; k < NCB; ++k) {
          const int c = q16 * 4 + 64 * k;
          if (KP && !jv[p]) v[p][u][k] = f4zero();       // (no key: nothing was published for it, nothing is fetched)
          else if constexpr (SC1)
            v[p][u][k] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(rP, (uint32_t)((off + (c < H ? c : 0)) * 4), 0, 16));   // sc1
          else v[p][u][k] = ld4(a.dkv_part + off + (c < H ? c : 0));
        }
      }
#pragma unroll
    for (int p = 0; p < RPS; ++p)
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (p0 + u < np) {
#pragma unroll
          for (int k = 0; k < NCB; ++k) d[p][k] = f4add(d[p][k], v[p][u][k]);
        }
  }
#pragma unroll
  for (int p = 0; p < RPS; ++p)
#pragma unroll
    for (int k = 0; k < NCB; ++k) {
      const int c = q16 * 4 + 64 * k, j = j0 + slot + NSLOT * p;
      float4 pg = f4zero(), pb = f4zero();
      if (jv[p] && c < H) {
        pg = make_float4(d[p][k].x * kh[p][k].x, d[p][k].y * kh[p][k].y, d[p][k].z * kh[p][k].z, d[p][k].w * kh[p][k].w);
        pb = d[p][k];
        st4(a.dkvhat + krow[p] + c, make_float4(d[p][k].x * g0[k].x + d0[p][k].x, d[p][k].y * g0[k].y + d0[p][k].y,
                                                d[p][k].z * g0[k].z + d0[p][k].z, d[p][k].w * g0[k].w + d0[p][k].w));
      }
      if constexpr (KP) {
        if (!jv[p] && j < Nk && c < H && !a.dkv_accumulate) st4(a.dkvhat + ((size_t)j * a.Bk + bk) * H + c, f4zero());
      }
      st4(Pp + (slot + NSLOT * p) * 2 * HP + c, pg);
      st4(Pp + (slot + NSLOT * p) * 2 * HP + HP + c, pb);
    }
  __syncthreads();
  const UDiv d2H(2 * H);
  const int ng = min(ngroups - grp0, ROWS / 16);         // groups of this call
  for (int o = tid; o < ng * 2 * H; o += NT) {
    const int g = ROWS == 16 ? 0 : d2H.div(o), c = o - g * 2 * H;
    const int hi = c >= H ? 1 : 0, col = hi * HP + (c - hi * H);      // (c < 2 H: [dgamma | dbeta])
    float t = 0.f;
#pragma unroll
    for (int sl = 0; sl < 16; ++sl) t += Pp[(g * 16 + sl) * 2 * HP + col];
    a.partials_kv[((size_t)bk * ngroups + grp0 + g) * 2 * H + c] = t;
  }
}
