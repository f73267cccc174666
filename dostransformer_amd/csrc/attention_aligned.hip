// Attention over the <= 64 keys of ONE crystal on crystal-aligned query tiles, stand-alone (round 5): the kernels
// dosx_attention_fwd / dosx_attention_bwd run for key sets of up to 64 rows when the layer's feed-forward half is NOT in the
// same launch (hidden 256: the Electron-DOS cross attention over a crystal's <= 64 atoms, layers/multihead_attention.py:49-76
// inside layers/transformer.py:131-139) - the tile arithmetic of ffn.hip's ffn_att_tile / ffn_att_bwd_tile for any hidden size
// up to 256, with a workgroup that STAYS on its crystal:
//   grid = Bq x wpc workgroups; workgroup (bq, w) owns the 32-row query tiles w, w + wpc, ... of query batch entry bq;
//   the crystal's key rows (pre-normalised, [NkP][H + 4], rows beyond Nk zero) are copied to LDS ONCE per workgroup;
//   per tile: quarter-wave row phases (LayerNorm-0 / softmax / residual) between 16 x 16 x 4 fp32 MFMA jobs dealt over the 8
//   waves; the next tile's rows are requested while the current one is multiplied.
// The kernels they replace for these shapes (attention.hip: attn_fwd_stream_kernel / attn_bwd_dq_stream_kernel, one 32-query
// tile per workgroup, keys re-staged per tile, 4 matrix waves) ran at 9-13 % of the fp32 MFMA peak in the Electron-DOS step.
// Backward: a workgroup keeps its share of dK^ = P'^T.dO + dS^T.Q in registers ACROSS its tiles (one [Nk, H] share per
// workgroup instead of one per tile), publishes it to its slot of dkv_part, takes a ticket on the key crystal's counter, and the
// last arriver finishes the key gradient (dkv_reduce.h) - DosxAttn's one-launch contract (include/dosx.h).  The query-side
// [dgamma | dbeta] partial rows: one per WORKGROUP in row (bq * nqt + w), the rows of the tiles it also owned are zeroed.
// Deterministic: fixed tile -> workgroup assignment, fixed summation orders.
#include <stdlib.h>

#include "attn_rows.h"
#include "common.h"
#include "dkv_reduce.h"
#include "mma16.h"

#ifdef DOSX_STAMPS
__device__ unsigned long long dosx_al_stamp_buf[64];
extern "C" int dosx_debug_read_attn_aligned_stamps(unsigned long long* host64) {
  return (int)hipMemcpyFromSymbol(host64, HIP_SYMBOL(dosx_al_stamp_buf), sizeof(unsigned long long) * 64);
}
// workgroup 0, wave 0: slot + 16 * (tile ordinal, first two tiles); slot 0 = kernel start, 15 = end (ordinal 3)
#define ASTAMP(slot) do { if (threadIdx.x == 0 && blockIdx.x == 0) dosx_al_stamp_buf[(slot)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define ASTAMP(slot) do { } while (0)
#endif

namespace {

constexpr int R = 32;          // query rows per tile (one quarter wave per row)

struct AlGeo {
  int wpc, KS;
};

// The two product shapes of a tile as PIPELINED job streams (stamps of the first version, tools/stamp_attn_aligned.py: a wave's jobs
// ran load-all-fragments -> wait -> MFMAs one after the other - 5.0-5.3 k clk per phase for 3.1 k clk of MFMA issue per SIMD):
// the fragments of the NEXT (half-)job are requested before the MFMAs of the current one, two register sets.
//
// kk: C[r][j] = sum_k A[r][k] B[j][k] (scores, dP): both operands k-contiguous rows of pitch LDK.  Unit (job, kq) = the 16 x 16
// tile job = (rt, ct) over the k-blocks [kq HPU, (kq + 1) HPU) of 64, HPU = NG / KS; partial tile kq of Sc gets `scale` x its sum.
// Units are dealt over the 8 waves; a wave walks its units k-block by k-block.
template <int NG, int LDK>
__device__ __forceinline__ void al_kk_phase(const float* __restrict__ As, const float* __restrict__ Ks, float* __restrict__ Sc,
                                            const int nctS, const int njobsS, const int KS, const float scale, const int wave,
                                            const int l15, const int g4) {
  // (KS and HPU = NG / KS are powers of two, a tile has two row blocks: shifts and one compare - run-time integer divisions
  //  cost ~40 instructions each, six per half-job were most of this phase's 5.5 k clk)
  const int ksl = KS == 4 ? 2 : (KS == 2 ? 1 : 0), hpl = (NG == 4 ? 2 : (NG == 2 ? 1 : 0)) - ksl;
  const int HPU = 1 << hpl, nunits = njobsS << ksl;
  // unit = wave + 8 i: waves w and w + 4 share a SIMD, so a partial last round (12 units: waves 0-3) still gives every SIMD the
  // same number of units (dealing the extra units to the even waves instead was measured: slower, 54.1 -> 56.9 us backward)
  const int nmine = wave < nunits ? (nunits - wave + 7) >> 3 : 0;
  const int nh = nmine << hpl;
  if (nh == 0) return;
  auto unit_of = [&](const int i) { return wave + 8 * i; };
  auto req = [&](const int hj, float4(&fa)[4], float4(&fb)[4]) {
    const int u = unit_of(hj >> hpl), kbi = hj & (HPU - 1);
    const int job = u >> ksl, kq = u & (KS - 1), rt = job >= nctS ? 1 : 0, ct = job - rt * nctS;
    const int k0 = 64 * ((kq << hpl) + kbi) + 4 * g4;
    const float* Ap = As + (16 * rt + l15) * LDK + k0;
    const float* Bp = Ks + (16 * ct + l15) * LDK + k0;
#pragma unroll
    for (int st = 0; st < 4; ++st) { fa[st] = ld4(Ap + 16 * st); fb[st] = ld4(Bp + 16 * st); }
  };
  // TWO accumulator chains per wave (even / odd steps, added at the end of the unit): a wave that is alone on its SIMD - the
  // waves with the extra unit of a partial round - cannot issue DEPENDENT MFMAs back to back
  f32x4 acc = {0.f, 0.f, 0.f, 0.f}, acc2 = {0.f, 0.f, 0.f, 0.f};
  auto mul = [&](const int hj, const float4(&fa)[4], const float4(&fb)[4]) {
#pragma unroll
    for (int st = 0; st < 4; st += 2) {
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[st].x, fb[st].x, acc, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[st + 1].x, fb[st + 1].x, acc2, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[st].y, fb[st].y, acc, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[st + 1].y, fb[st + 1].y, acc2, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[st].z, fb[st].z, acc, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[st + 1].z, fb[st + 1].z, acc2, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[st].w, fb[st].w, acc, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[st + 1].w, fb[st + 1].w, acc2, 0, 0, 0);
    }
    const int ui = hj >> hpl;
    if ((hj & (HPU - 1)) == HPU - 1) {               // the unit's last k-block: its partial tile
      const int u = unit_of(ui), job = u >> ksl, kq = u & (KS - 1), rt = job >= nctS ? 1 : 0, ct = job - rt * nctS;
      float* Sp = Sc + kq * R * 68;
#pragma unroll
      for (int i = 0; i < 4; ++i) Sp[(16 * rt + 4 * g4 + i) * 68 + 16 * ct + l15] = (acc[i] + acc2[i]) * scale;
      acc = f32x4{0.f, 0.f, 0.f, 0.f};
      acc2 = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
  float4 a0[4], b0[4], a1[4], b1[4];
  req(0, a0, b0);
  for (int hj = 0; hj < nh; hj += 2) {
    if (hj + 1 < nh) req(hj + 1, a1, b1);
    __builtin_amdgcn_sched_barrier(0);
    mul(hj, a0, b0);
    if (hj + 1 >= nh) break;
    if (hj + 2 < nh) req(hj + 2, a0, b0);
    __builtin_amdgcn_sched_barrier(0);
    mul(hj + 1, a1, b1);
  }
}

// kn: C[r][c] = sum_j A[r][j] B[j][c] (P.K, dS.K): A = [R][68] rows (j-contiguous), B = the key rows ([j][LDK], four ds_read_b32 per
// step), NkP / 16 steps of 16 keys per job; the 2 x H / 16 jobs are dealt over the 8 waves, output rows of pitch LDK.
template <int NG, int LDK, bool PIPE = true>
__device__ __forceinline__ void al_kn_phase(const float* __restrict__ Ss, const float* __restrict__ Ks, float* __restrict__ Os,
                                            const int nsteps, const int wave, const int l15, const int g4) {
  constexpr int nct = 4 * NG, njobs = (R / 16) * nct, NJ = njobs / 8;       // NJ = NG jobs per wave
  auto req = [&](const int i, float4(&fa)[4], float(&fb)[4][4]) {
    const int job = wave + 8 * i, rt = job / nct, ct = job - rt * nct;
    const float* Ap = Ss + (16 * rt + l15) * 68 + 4 * g4;
    const float* Bp = Ks + (4 * g4) * LDK + 16 * ct + l15;
#pragma unroll
    for (int st = 0; st < 4; ++st)
      if (st < nsteps) {
        fa[st] = ld4(Ap + 16 * st);
#pragma unroll
        for (int j = 0; j < 4; ++j) fb[st][j] = Bp[(16 * st + j) * LDK];
      }
  };
  auto mul = [&](const int i, const float4(&fa)[4], const float(&fb)[4][4]) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int st = 0; st < 4; ++st)
      if (st < nsteps) {
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[st].x, fb[st][0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[st].y, fb[st][1], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[st].z, fb[st][2], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[st].w, fb[st][3], acc, 0, 0, 0);
      }
    const int job = wave + 8 * i, rt = job / nct, ct = job - rt * nct;
#pragma unroll
    for (int r = 0; r < 4; ++r) Os[(16 * rt + 4 * g4 + r) * LDK + 16 * ct + l15] = acc[r];
  };
  float4 a0[4], a1[4];
  float b0[4][4], b1[4][4];
  if constexpr (!PIPE) {               // (the backward kernel at hidden 256 has no registers for the second set)
#pragma unroll
    for (int i = 0; i < NJ; ++i) {
      req(i, a0, b0);
      __builtin_amdgcn_sched_barrier(0);
      mul(i, a0, b0);
    }
    return;
  }
  req(0, a0, b0);
#pragma unroll
  for (int i = 0; i < NJ; i += 2) {
    if (i + 1 < NJ) req(i + 1, a1, b1);
    __builtin_amdgcn_sched_barrier(0);
    mul(i, a0, b0);
    if (i + 1 >= NJ) break;
    if (i + 2 < NJ) req(i + 2, a0, b0);
    __builtin_amdgcn_sched_barrier(0);
    mul(i + 1, a1, b1);
  }
}

// ------------------------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------------------------
template <int NG, bool KP>
__global__ __launch_bounds__(512) void attn_al_fwd_kernel(const DosxAttn a, const AlGeo geo) {
  DOSX_SET_MAIN_PRIO();
  extern __shared__ __align__(16) float sm[];
  constexpr int H = 64 * NG, LDK = H + 4;        // (hidden = 64 NG exactly: every tile offset is an immediate)
  const int Nk = a.Nk, NkP = (Nk + 15) & ~15, Sq = a.Sq;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q16 = lane & 15, l15 = q16, g4 = lane >> 4;
  const int wpc = geo.wpc, KS = geo.KS;
  const int bq = blockIdx.x / wpc, w = blockIdx.x - bq * wpc, bk = bq % a.Bk;
  const int nk = dosx_live_keys_fwd<KP>(a.key_ptr, bk, Nk);      // keys this crystal attends over (DosxAttn.key_ptr), else Nk
  const int nctL = dosx_live_tiles<KP, 4>(nk, NkP >> 4);         // 16-key tiles with live keys: the others take no loads and no MFMAs
  const int nqt = (Sq + R - 1) / R;
  float* Ks = sm;                      // [NkP][LDK]
  float* Qs = Ks + NkP * LDK;          // [R][LDK]   q o g0 -> O
  float* Sc = Qs + R * LDK;            // [KS][R][68] score partials; [0]: P o mask
  const float scale = rsqrtf((float)H), invH = 1.f / (float)H;
  const int lr = wave * 4 + g4;        // this quarter wave's row of the tile
  float4 g0[NG], b0[NG];
  bool on[NG];
#pragma unroll
  for (int k = 0; k < NG; ++k) {
    const int c = q16 * 4 + 64 * k;
    on[k] = c < H;
    g0[k] = ld4(a.gamma0 + (on[k] ? c : 0));
    b0[k] = ld4(a.beta0 + (on[k] ? c : 0));
  }
  auto load_x = [&](const int t, float4(&x)[NG]) {
    const int s = min(t * R + lr, Sq - 1);
    const float* xrow = a.x + ((size_t)s * a.q_stride_s + (size_t)bq * a.q_stride_b) * H;
#pragma unroll
    for (int k = 0; k < NG; ++k) x[k] = on[k] ? ld4(xrow + q16 * 4 + 64 * k) : f4zero();
  };
  ASTAMP(0);
  float4 xr[NG], xn[NG];
  load_x(w, xr);
  {   // the crystal's key rows -> Ks (rows beyond its nk keys zero, never fetched), behind the first tile's rows
    const int h4 = H >> 2;
    float4 kr[2 * NG];                 // NkP * h4 <= 64 * 16 NG = 2 NG float4 per thread
#pragma unroll
    for (int i = 0; i < 2 * NG; ++i) {
      const int e = tid + 512 * i, j = e / h4, c = (e - j * h4) * 4;
      kr[i] = (e < NkP * h4 && j < (KP ? nk : Nk)) ? ld4(a.kvhat + ((size_t)j * a.Bk + bk) * H + c) : f4zero();
    }
#pragma unroll
    for (int i = 0; i < 2 * NG; ++i) {
      const int e = tid + 512 * i, j = e / h4, c = (e - j * h4) * 4;
      if (e < 16 * nctL * h4) st4(Ks + j * LDK + c, kr[i]);
    }
  }
  const int nctS = nctL, njobsS = (R / 16) * nctS, klen = H / KS;       // (the score jobs: live key tiles only)
  for (int t = w; t < nqt; t += wpc) {
    const int s = min(t * R + lr, Sq - 1);
    const bool rv = (t * R + lr) < Sq;
    const size_t r = (size_t)s * a.Bq + bq;          // global row (valid memory also for the clamped duplicates)
    // ---- A: LayerNorm-0, the key gamma folded into q -> Qs ----
    float mean, rstd;
    dosx_row16_stats<NG>(xr, on, invH, mean, rstd);
#pragma unroll
    for (int k = 0; k < NG; ++k) {                     // (written out here and in ffn_att_tile: shared, it cost that kernel one VGPR)
      if (!on[k]) continue;
      const float4 v = xr[k];
      const float4 q = make_float4((v.x - mean) * rstd * g0[k].x + b0[k].x, (v.y - mean) * rstd * g0[k].y + b0[k].y,
                                   (v.z - mean) * rstd * g0[k].z + b0[k].z, (v.w - mean) * rstd * g0[k].w + b0[k].w);
      st4(Qs + lr * LDK + q16 * 4 + 64 * k, make_float4(q.x * g0[k].x, q.y * g0[k].y, q.z * g0[k].z, q.w * g0[k].w));
    }
    if (t + wpc < nqt) load_x(t + wpc, xn);           // the next tile's rows: in flight under this tile's products
    const int so = t == w ? 0 : (t == w + wpc ? 16 : 48);     // (stamps of the first two tiles)
    ASTAMP(so + 1);
    __syncthreads();
    ASTAMP(so + 2);
    // ---- B: S = Qs . Ks^T (scaled); the K range split KS ways, partial tiles added in a fixed order by phase C ----
    al_kk_phase<NG, LDK>(Qs, Ks, Sc, nctS, njobsS, KS, scale, wave, l15, g4);
    ASTAMP(so + 3);
    __syncthreads();
    ASTAMP(so + 4);
    // ---- C: exact fp32 softmax of this quarter wave's row; P written out; P o mask -> Sc ----
    float psum;
    {
      float* Sr = Sc + lr * 68;
      float v[4];
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int j = q16 + 16 * jj;
        v[jj] = -INFINITY;
        if (j < nk) {                                  // (nk: the crystal's own key count with DosxAttn.key_ptr, else Nk)
          v[jj] = Sr[j];
          for (int kq = 1; kq < KS; ++kq) v[jj] += Sr[kq * R * 68 + j];
        }
      }
      psum = dosx_att_softmax_row<KP>(v, nk, Nk, NkP, q16, a.drop_mask, a.probs, ((size_t)bq * Sq + s) * Nk, rv, Sr);
    }
    ASTAMP(so + 5);
    __syncthreads();
    ASTAMP(so + 6);
    // ---- D: O = (P o mask) . Ks -> Qs ----
    al_kn_phase<NG, LDK>(Sc, Ks, Qs, nctL, wave, l15, g4);
    ASTAMP(so + 7);
    __syncthreads();
    ASTAMP(so + 8);
    // ---- E: x1 = O o g0 + b0 sum(P o mask) + x; both rows of statistics ----
    {
      float4 x1[NG];
#pragma unroll
      for (int k = 0; k < NG; ++k) {                   // (written out here and in ffn_att_tile: shared, it cost that kernel one VGPR)
        const int c = q16 * 4 + 64 * k;
        x1[k] = f4zero();
        if (!on[k]) continue;
        const float4 o = ld4(Qs + lr * LDK + c);
        x1[k] = make_float4(o.x * g0[k].x + b0[k].x * psum + xr[k].x, o.y * g0[k].y + b0[k].y * psum + xr[k].y,
                            o.z * g0[k].z + b0[k].z * psum + xr[k].z, o.w * g0[k].w + b0[k].w * psum + xr[k].w);
        if (rv) st4(a.out + r * H + c, x1[k]);
      }
      if (a.out_stats) {
        float mean1, rstd1;
        dosx_row16_stats<NG>(x1, on, invH, mean1, rstd1);
        if (rv && q16 == 0) { a.out_stats[2 * r] = mean1; a.out_stats[2 * r + 1] = rstd1; }
        if (a.ln1_out && rv) {         // the next LayerNorm on the row still in registers (DosxAttn.ln1_*)
          float4 g1[NG], b1[NG];
#pragma unroll
          for (int k = 0; k < NG; ++k) { g1[k] = ld4(a.ln1_gamma + q16 * 4 + 64 * k); b1[k] = ld4(a.ln1_beta + q16 * 4 + 64 * k); }
          dosx_att_ln_row<NG>(x1, on, mean1, rstd1, g1, b1, a.ln1_out + r * H, q16);
        }
      }
      if (rv && q16 == 0) { a.qstats[2 * r] = mean; a.qstats[2 * r + 1] = rstd; }
    }
    // (no barrier: phase A of the next tile writes only this quarter wave's own row of Qs, which phase E has just read; the
    //  other waves read Qs / Sc again only behind the next tile's first barrier)
    ASTAMP(so + 9);
#pragma unroll
    for (int k = 0; k < NG; ++k) xr[k] = xn[k];
  }
  ASTAMP(63);
}

// ------------------------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------------------------
// QO (DOSX_ATTN_BWD_DQ_HALF with dkvhat == NULL: the query-only backward, for keys that come from frozen parameters): phases a - e
// as they are, their P' / Ql stores to LDS included (the row phases stay the text the full form compiles: with the two stores taken
// out of this kernel, the results with a dropout mask were no longer bitwise the full form's - the instantiation compiled to other
// arithmetic; ffn_att_bwd_tile's query-only form does drop them and stays bitwise, tests/test_gpu_attention_query_only.py) - dx and partials_q are bitwise the full
// form's - without phase f, the publication, the ticket and the last arriver's reduction; dkv_part / dkv_cnt / partials_kv /
// dkvhat are not touched.
template <int NG, bool KP, bool QO = false>
__global__ __launch_bounds__(512) void attn_al_bwd_kernel(const DosxAttn a, const AlGeo geo) {
  DOSX_SET_MAIN_PRIO();
  extern __shared__ __align__(16) float sm[];
  constexpr int HP = 64 * NG, NJW = 2 * NG;            // <= 4 x 4 NG key-tile x column-tile jobs of the share, 8 waves
  constexpr int H = 64 * NG, LDK = H + 4;        // (hidden = 64 NG exactly: every tile offset is an immediate)
  const int Nk = a.Nk, NkP = (Nk + 15) & ~15, Sq = a.Sq;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q16 = lane & 15, l15 = q16, g4 = lane >> 4;
  const int wpc = geo.wpc, KS = geo.KS;
  const int bq = blockIdx.x / wpc, w = blockIdx.x - bq * wpc, bk = bq % a.Bk;
  const int nk = dosx_live_keys<KP>(a.key_ptr, bk, Nk);  // KP: the keys this crystal attends over (DosxAttn.key_ptr), else Nk
  const int nctL = dosx_live_tiles<KP, 4>(nk, NkP >> 4); // 16-key tiles with live keys: the others take no loads and no MFMAs
  const int nqt = (Sq + R - 1) / R;
  float* Ks = sm;                      // [NkP][LDK]
  float* Os = Ks + NkP * LDK;          // [R][LDK]   dO rows
  float* Ds = Os + R * LDK;            // [R][LDK]   dO o g0 -> dq -> Ql = LN0(x) g0 + b0
  float* Sc = Ds + R * LDK;            // [2][R][68] dP partials -> [0]: dS (Ss), [1]: P o mask (Ps2)
  float* Ss = Sc;
  float* Ps2 = Sc + R * 68;
  const float scale = rsqrtf((float)H), invH = 1.f / (float)H;
  const int lr = wave * 4 + g4;
  float4 g0[NG], b0[NG];
  bool on[NG];
#pragma unroll
  for (int k = 0; k < NG; ++k) {
    const int c = q16 * 4 + 64 * k;
    on[k] = c < H;
    g0[k] = ld4(a.gamma0 + (on[k] ? c : 0));
    b0[k] = ld4(a.beta0 + (on[k] ? c : 0));
  }
  auto load_go = [&](const int t, float4(&go)[NG]) {
    const int s = min(t * R + lr, Sq - 1);
    const size_t orow = (size_t)s * a.Bq + bq;
#pragma unroll
    for (int k = 0; k < NG; ++k) go[k] = on[k] ? ld4(a.dout + orow * H + q16 * 4 + 64 * k) : f4zero();
  };
  ASTAMP(0);
  float4 ngo[NG];                      // the NEXT tile's dO row (requested one tile ahead)
  load_go(w, ngo);
  {   // the crystal's key rows -> Ks
    const int h4 = H >> 2;
    float4 kr[2 * NG];
#pragma unroll
    for (int i = 0; i < 2 * NG; ++i) {
      const int e = tid + 512 * i, j = e / h4, c = (e - j * h4) * 4;
      kr[i] = (e < NkP * h4 && j < nk) ? ld4(a.kvhat + ((size_t)j * a.Bk + bk) * H + c) : f4zero();
    }
#pragma unroll
    for (int i = 0; i < 2 * NG; ++i) {
      const int e = tid + 512 * i, j = e / h4, c = (e - j * h4) * 4;
      if (e < 16 * nctL * h4) st4(Ks + j * LDK + c, kr[i]);
    }
  }
  const int nctS = nctL, njobsS = (R / 16) * nctS, klen = H / KS;       // (dP, dq and key-gradient jobs: live key tiles only)
  constexpr int nct = H >> 4;
  f32x4 accK[NJW];
#pragma unroll
  for (int i = 0; i < NJW; ++i) accK[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  // Phase f / the publication: job i of this wave = key tile jt0 + JT(i), column tile ct0 + CT(i) with compile-time JT, CT, so
  // that every fragment address is one of FOUR lane bases + an immediate (run-time job coordinates made the compiler keep
  // ~250 precomputed addresses alive across the tile loop: 128 spilled registers at hidden 256)
  const int jt0 = nct >= 8 ? 0 : (wave >> 2), ct0 = nct >= 8 ? wave : (wave & 3);
  const float* pPs = Ps2 + (4 * g4) * 68 + 16 * jt0 + l15;
  const float* pSs = Ss + (4 * g4) * 68 + 16 * jt0 + l15;
  const float* pOs = Os + (4 * g4) * LDK + 16 * ct0 + l15;
  const float* pQl = Ds + (4 * g4) * LDK + 16 * ct0 + l15;
  float4 pg[NG], pb[NG];
#pragma unroll
  for (int k = 0; k < NG; ++k) { pg[k] = f4zero(); pb[k] = f4zero(); }

  for (int t = w; t < nqt; t += wpc) {
    const int s = min(t * R + lr, Sq - 1);
    const bool rv = (t * R + lr) < Sq;
    const size_t orow = (size_t)s * a.Bq + bq;
    // this row's softmax weights + dropout multipliers (phase c): requested now
    float pr[4], mk[4];
    {
      const size_t prow = ((size_t)bq * Sq + s) * Nk;
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int j = q16 + 16 * jj;
        pr[jj] = dosx_key_entry<KP>(a.probs, prow, j, nk, Nk, 0.f);
        mk[jj] = a.drop_mask ? dosx_key_entry<KP>(a.drop_mask, prow, j, nk, Nk, 1.f) : 1.f;
      }
    }
    // ---- a: dO -> Os (zeros beyond the data);  Ds = dO o g0;  cq = dO . b0 (dropout only) ----
    // (hand-written, like ffn_att_bwd_tile's: as a shared phase it cost the NG = 1 instantiations one VGPR)
    float cq = 0.f;
    {
      float u = 0.f;
#pragma unroll
      for (int k = 0; k < NG; ++k) {
        if (!on[k]) continue;
        const float4 go = rv ? ngo[k] : f4zero();
        st4(Os + lr * LDK + q16 * 4 + 64 * k, go);
        st4(Ds + lr * LDK + q16 * 4 + 64 * k, make_float4(go.x * g0[k].x, go.y * g0[k].y, go.z * g0[k].z, go.w * g0[k].w));
        u += (go.x * b0[k].x + go.y * b0[k].y) + (go.z * b0[k].z + go.w * b0[k].w);
      }
      if (a.drop_mask) cq = row16_sum(u);
    }
    if (t + wpc < nqt) load_go(t + wpc, ngo);
    const int so = t == w ? 0 : (t == w + wpc ? 16 : 48);
    ASTAMP(so + 1);
    __syncthreads();
    ASTAMP(so + 2);
    // ---- b: dP (up to a row constant) = Ds . Ks^T ----
    al_kk_phase<NG, LDK>(Ds, Ks, Sc, nctS, njobsS, KS, 1.f, wave, l15, g4);
    ASTAMP(so + 3);
    __syncthreads();
    ASTAMP(so + 4);
    // ---- c: dS = P o (dP' - sum_j P dP') scale -> Ss;  P' = P o M -> Ps2 (zeros beyond Nk / the data); in place, row-wise ----
    dosx_att_bwd_ds_row(
        [&](const int j) {
          float u = Sc[lr * 68 + j];
          if (KS > 1) u += Sc[R * 68 + lr * 68 + j];
          return u;
        },
        pr, mk, a.drop_mask != nullptr, cq, nk, NkP, rv, scale, q16, Ss + lr * 68, Ps2 + lr * 68);
    // this row's query + LayerNorm-0 statistics (phase e): in flight under phase d
    float4 xr[NG];
    {
      const float* xrow = a.x + ((size_t)s * a.q_stride_s + (size_t)bq * a.q_stride_b) * H;
#pragma unroll
      for (int k = 0; k < NG; ++k) xr[k] = on[k] ? ld4(xrow + q16 * 4 + 64 * k) : f4zero();
    }
    const float mean = a.qstats[2 * orow], rstd = a.qstats[2 * orow + 1];
    ASTAMP(so + 5);
    __syncthreads();
    ASTAMP(so + 6);
    // ---- d: dq = dS . Ks -> Ds ----
    al_kn_phase<NG, LDK, (NG < 4)>(Ss, Ks, Ds, nctL, wave, l15, g4);
    ASTAMP(so + 7);
    __syncthreads();
    ASTAMP(so + 8);
    // ---- e: LayerNorm-0 backward on the query rows + residual -> dx; query-side dg0 / db0 (kept per row slot across the
    //         tiles); Ql = LN0(x) g0 + b0 over this quarter wave's own row of Ds ----
    dosx_att_bwd_ln0_row<NG, true>(Ds + lr * LDK, xr, on, g0, b0, mean, rstd, invH, rv,
                                   [&](const int k) { return ld4(Os + lr * LDK + q16 * 4 + 64 * k); },   // (this row's dO)
                                   a.dx + orow * H, Ds + lr * LDK, q16, pg, pb);
    ASTAMP(so + 9);
    __syncthreads();
    ASTAMP(so + 10);
    // ---- f: this workgroup's share of dK + dV += P'^T . dO + dS^T . Ql   ([NkP keys] x [R queries] . [R queries] x [H]) ----
    if constexpr (!QO) {
#pragma unroll
    for (int i = 0; i < NJW; ++i) {
      // job i of this wave: key tile jt, column tile ct - jt a compile-time value (or one of two), ct = the wave's own column
      // tile(s), so that every fragment address is ONE lane base + an immediate (run-time job coordinates made the compiler
      // keep ~250 precomputed addresses alive across the tile loop: 128 spilled registers at hidden 256)
      const int JT = nct >= 8 ? i / (nct / 8) : 2 * i, CT = nct >= 8 ? 8 * (i % (nct / 8)) : 0;
      if (jt0 + JT >= nctS) continue;
      float pa[R / 4], sa[R / 4], b1[R / 4], b2[R / 4];
#pragma unroll
      for (int kk = 0; kk < R; kk += 16)
#pragma unroll
        for (int i2 = 0; i2 < 4; ++i2) {
          const int o = (kk >> 2) + i2;
          pa[o] = pPs[(kk + i2) * 68 + 16 * JT];
          sa[o] = pSs[(kk + i2) * 68 + 16 * JT];
          b1[o] = pOs[(kk + i2) * LDK + 16 * CT];
          b2[o] = pQl[(kk + i2) * LDK + 16 * CT];
        }
      __builtin_amdgcn_sched_barrier(0);               // (all 32 fragments of the job requested before its first MFMA)
#pragma unroll
      for (int o = 0; o < R / 4; ++o) {
        accK[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[o], b1[o], accK[i], 0, 0, 0);
        accK[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(sa[o], b2[o], accK[i], 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);               // (one job's 32 fragments at a time: the unrolled jobs must not be merged)
    }
    }
    ASTAMP(so + 11);
    __syncthreads();                   // (the next tile's phase a overwrites Os / Ds)
    ASTAMP(so + 12);
  }
  ASTAMP(60);
  // ---- publish this workgroup's share (write-through) ----
  if constexpr (!QO) {
    float* part = a.dkv_part + ((size_t)bq * nqt + w) * (size_t)Nk * H;
#pragma unroll
    for (int i = 0; i < NJW; ++i) {
      const int jt = jt0 + (nct >= 8 ? i / (nct / 8) : 2 * i), ct = ct0 + (nct >= 8 ? 8 * (i % (nct / 8)) : 0);
      if (jt >= nctS) continue;
#pragma unroll
      for (int i2 = 0; i2 < 4; ++i2) {
        const int j = 16 * jt + 4 * g4 + i2, col = 16 * ct + l15;
        if (j < (KP ? nk : Nk)) __hip_atomic_store(part + (size_t)j * H + col, accK[i][i2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // sc1
      }
    }
  }
  // ---- the query-side [dgamma | dbeta] row of this workgroup: 32 row slots -> column sums; zero rows for its other tiles ----
  {
    float* Pp = sm;                    // [32][2][HP]  (everything else in LDS is dead: the loop ended with a barrier)
#pragma unroll
    for (int k = 0; k < NG; ++k) {
      const int c = q16 * 4 + 64 * k;
      st4(Pp + lr * 2 * HP + c, pg[k]);
      st4(Pp + lr * 2 * HP + HP + c, pb[k]);
    }
    __syncthreads();
    float* prow = a.partials_q + ((size_t)bq * nqt + w) * 2 * H;
    for (int c = tid; c < 2 * H; c += 512) {
      const int o = (c / H) * HP + (c % H);
      float u = 0.f;
#pragma unroll
      for (int sl = 0; sl < 32; ++sl) u += Pp[sl * 2 * HP + o];
      prow[c] = u;
    }
    for (int t2 = w + wpc; t2 < nqt; t2 += wpc) {
      float* z = a.partials_q + ((size_t)bq * nqt + t2) * 2 * H;
      for (int c = tid; c < 2 * H; c += 512) z[c] = 0.f;
    }
  }
  if constexpr (QO) return;
  // ---- ticket: the last arriving workgroup of key crystal bk finishes its key gradient ----
  ASTAMP(61);
  const bool last = dosx_last_arriver_wg(a.dkv_cnt, bk, (a.Bq / a.Bk) * wpc, reinterpret_cast<int*>(sm), tid);
  __syncthreads();                     // (the flag word is about to be overwritten by the reduction's LDS rows)
  if (last) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // all <= 64 key rows at once, two per quarter-wave slot: sm = [64][2 * 64 NG] floats (al_bwd_smem)
    const DkvReduce r = dkv_reduce_operands(a);
    dosx_dkv_reduce<NG, 64 * NG, NG <= 2 ? 4 : 2, KP, 2, 512, true>(r, nqt, wpc, bk, 0, sm, tid);
    if (tid == 0) dosx_counter_reset(a.dkv_cnt + bk);
  }
  ASTAMP(63);
}

// which shapes take these kernels (dosx_attention_aligned_mode): 0 = none, 1 = hidden > 128 only, 2 = every shape they cover
// (the default: faster than attention.hip's at every BASELINE shape with <= 64 keys, profiles/r05_kernel_microbench.log `attn`)
int g_al_mode = 2;

// the query-only backward: the dq half alone, no key gradient wanted
inline bool al_query_only(const DosxAttn& a) { return a.flags == DOSX_ATTN_BWD_DQ_HALF && a.dkvhat == nullptr; }

inline bool al_shape_ok(const DosxAttn& a, const bool query_only = false) {
  const int m = g_al_mode;
  return m > 0 && (a.flags == 0 || query_only) && a.Nk >= 1 && a.Nk <= 64 && (a.H == 64 || a.H == 128 || a.H == 256) && (m > 1 || a.H > 128) &&
         a.qstats != nullptr;
}

inline AlGeo al_geo(const DosxAttn& a, const bool bwd) {
  const int nqt = ceil_div(a.Sq, R), NkP = (a.Nk + 15) & ~15;
  AlGeo g;
  g.wpc = 256 / a.Bq;
  if (g.wpc < 1) g.wpc = 1;
  if (g.wpc > nqt) g.wpc = nqt;
  const int njobsS = (R / 16) * (NkP >> 4);
  // K split of the score / dP jobs over otherwise idle waves, in whole k-blocks of 64 (KS divides NG = H / 64)
  int KS = njobsS >= 8 ? 1 : (njobsS >= 4 ? 2 : 4);
  if (bwd && KS > 2) KS = 2;                               // (two partial tiles of LDS in the backward kernel)
  const int ng = a.H / 64;
  while (KS > ng) KS >>= 1;
  g.KS = KS;
  return g;
}

inline size_t al_fwd_smem(const DosxAttn& a, const AlGeo& g) {
  const int NkP = (a.Nk + 15) & ~15, LDK = a.H + 4;
  return sizeof(float) * ((size_t)NkP * LDK + (size_t)R * LDK + (size_t)g.KS * R * 68);
}

inline size_t al_bwd_smem(const DosxAttn& a) {
  const int NkP = (a.Nk + 15) & ~15, LDK = a.H + 4, HP = 64 * ceil_div(a.H, 64);
  const size_t mainf = (size_t)NkP * LDK + 2 * (size_t)R * LDK + 2 * (size_t)R * 68, red = (size_t)64 * 2 * HP;
  return sizeof(float) * (mainf > red ? mainf : red);
}

}  // namespace

namespace dosx_detail {

// 1: launched; 0: not this shape (the caller runs attention.hip's kernels); < 0: error
int attn_aligned_fwd(const DosxAttn& a, hipStream_t st) {
  if (!al_shape_ok(a)) return 0;
  const AlGeo g = al_geo(a, false);
  const size_t smem = al_fwd_smem(a, g);
  if (smem > 160 * 1024) return 0;
  const dim3 grid(a.Bq * g.wpc);
#define DOSX_ALF1(NG_, KP_)                                                                                              \
  do {                                                                                                                   \
    static bool attr_set = false;                                                                                        \
    if (!attr_set) {                                                                                                     \
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_al_fwd_kernel<NG_, KP_>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); \
      attr_set = true;                                                                                                   \
    }                                                                                                                    \
    hipLaunchKernelGGL((attn_al_fwd_kernel<NG_, KP_>), grid, dim3(512), smem, st, a, g);                                 \
  } while (0)
#define DOSX_ALF(NG_) do { if (a.key_ptr) DOSX_ALF1(NG_, true); else DOSX_ALF1(NG_, false); } while (0)
  switch (ceil_div(a.H, 64)) {
    case 1: DOSX_ALF(1); break;
    case 2: DOSX_ALF(2); break;
    default: DOSX_ALF(4);
  }
#undef DOSX_ALF
#undef DOSX_ALF1
  DOSX_LAUNCH_CHECK();
  return 1;
}

int attn_aligned_bwd(const DosxAttn& a, hipStream_t st) {
  const bool qo = al_query_only(a);
  if (!al_shape_ok(a, qo) || (!qo && (!a.dkv_part || !a.dkv_cnt))) return 0;
  const AlGeo g = al_geo(a, true);
  if (g.KS > 2) return 0;
  const size_t smem = al_bwd_smem(a);
  if (smem > 160 * 1024 || (!qo && (size_t)a.Bq * ceil_div(a.Sq, R) * a.Nk * a.H * 4 >= 0x7fffffffull)) return 0;
  const dim3 grid(a.Bq * g.wpc);
#define DOSX_ALB1(NG_, KP_, QO_)                                                                                         \
  do {                                                                                                                   \
    static bool attr_set = false;                                                                                        \
    if (!attr_set) {                                                                                                     \
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_al_bwd_kernel<NG_, KP_, QO_>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); \
      attr_set = true;                                                                                                   \
    }                                                                                                                    \
    hipLaunchKernelGGL((attn_al_bwd_kernel<NG_, KP_, QO_>), grid, dim3(512), smem, st, a, g);                            \
  } while (0)
#define DOSX_ALB2(NG_, KP_) do { if (qo) DOSX_ALB1(NG_, KP_, true); else DOSX_ALB1(NG_, KP_, false); } while (0)
#define DOSX_ALB(NG_) do { if (a.key_ptr) DOSX_ALB2(NG_, true); else DOSX_ALB2(NG_, false); } while (0)
  switch (ceil_div(a.H, 64)) {
    case 1: DOSX_ALB(1); break;
    case 2: DOSX_ALB(2); break;
    default: DOSX_ALB(4);
  }
#undef DOSX_ALB
#undef DOSX_ALB2
#undef DOSX_ALB1
  DOSX_LAUNCH_CHECK();
  return 1;
}

}  // namespace dosx_detail

extern "C" int dosx_attention_aligned_mode(int mode) {
  const int prev = g_al_mode;
  if (mode >= 0) g_al_mode = mode > 2 ? 2 : mode;
  return prev;
}
