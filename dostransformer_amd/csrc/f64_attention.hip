// float64 attention of DOSTransformer_phonon (include/dosx.h, "float64 program"): one pre-norm encoder layer's attention
// half (layers/multihead_attention.py:49-76, layers/transformer.py:131-137) with the reference's numerics - scores and
// products in fp64, the softmax (and its backward) in fp32 between a rounding to fp32 and a promotion back - plus the
// zero-padded dense key rows (to_dense_batch + the parameter-free part of LayerNorm 0) and the prompt-row index sum.
// Written like f64.hip: one MFMA shape (v_mfma_f64_16x16x4_f64), operands straight from global memory, score rows kept in
// the saved-probability buffer (any number of keys), every reduction in a fixed order, no atomics.
#include <cmath>

#include "common.h"

typedef double f64x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int kQ = 16;        // query rows per workgroup of the forward / dq launches, keys per wave of the dkv launch
constexpr int kRowMax = 1024 / 64;

__device__ __forceinline__ double wave_sum64(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ double wave_max64(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ __forceinline__ float wave_sum32(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ float wave_max32(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// lane l supplies A[l & 15][k = l >> 4] and B[k = l >> 4][l & 15]; result register i of lane l is C[(l >> 4) + 4 i][l & 15]
__device__ __forceinline__ f64x4 mfma64(double a, double b, f64x4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// key / value element: LayerNorm 0's affine applied to the normalised key row (k = v, transformer.py:132-134)
__device__ __forceinline__ double kv_at(const DosxAttn64& d, const double* row, int h) {
  return row[h] * d.gamma0[h] + d.beta0[h];
}

// live keys of key crystal bk: all Nk without key_ptr, else its own count clamped to [0, Nk] (wave-uniform)
__device__ __forceinline__ int live_keys(const DosxAttn64& d, int bk) {
  if (d.key_ptr == nullptr) return d.Nk;
  return min(max(d.key_ptr[bk + 1] - d.key_ptr[bk], 0), d.Nk);
}

// C[s][j] (+)= sum_h A[s][h] * kv[j][h] for 16 rows [s0, s0+16) of A (row stride H) and 16 keys [j0, j0+16) below n
__device__ __forceinline__ f64x4 rows_times_keys(const DosxAttn64& d, const double* A, int nrows, int s0, const double* kv,
                                                 int n, int j0, int lane) {
  const int r = lane & 15, kl = lane >> 4;
  const double* arow = s0 + r < nrows ? A + (int64_t)(s0 + r) * d.H : nullptr;
  const double* krow = j0 + r < n ? kv + (int64_t)(j0 + r) * d.H : nullptr;
  f64x4 acc = {0.0, 0.0, 0.0, 0.0};
  for (int h0 = 0; h0 < d.H; h0 += 4) {
    const int h = h0 + kl;
    const bool hin = h < d.H;
    const double a = (arow != nullptr && hin) ? arow[h] : 0.0;
    const double b = (krow != nullptr && hin) ? kv_at(d, krow, h) : 0.0;
    acc = mfma64(a, b, acc);
  }
  return acc;
}

// out[s][c0 + 0..63] = sum_{j < n} W[s][j] * (mask) * kv[j][c] for the 16 query rows of the tile (W rows of stride Nk)
__device__ __forceinline__ void weights_times_values(const DosxAttn64& d, const double* W, const float* M, int Sq, int s0,
                                                     const double* kv, int n, int c0, int lane, f64x4 acc[4]) {
  const int r = lane & 15, kl = lane >> 4;
  const int sa = s0 + r;
  for (int t = 0; t < 4; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
  for (int j0 = 0; j0 < n; j0 += 4) {
    const int j = j0 + kl;
    const bool jin = j < n;
    double a = 0.0;
    if (sa < Sq && jin) {
      a = W[(int64_t)sa * d.Nk + j];
      if (M != nullptr) a *= (double)M[(int64_t)sa * d.Nk + j];
    }
    const double* vrow = jin ? kv + (int64_t)j * d.H : nullptr;
    for (int t = 0; t < 4; ++t) {
      const int h = c0 + 16 * t + r;
      const double b = (vrow != nullptr && h < d.H) ? kv_at(d, vrow, h) : 0.0;
      acc[t] = mfma64(a, b, acc[t]);
    }
  }
}

// Forward.  Workgroup: query rows [s0, s0+16) of crystal bq; 4 waves.  1) scores * H^-1/2 into probs (waves take key
// tiles in turn); 2) softmax of each row in place (a wave per row); 3) out = x + (p o mask) . v (waves take 64 columns).
// With key_ptr only the n live keys of the crystal exist: every loop ends at n, nothing past it is read, probs[s][j >= n]
// is written as 0.0 (n = 0: out = x).
__global__ __launch_bounds__(256) void attn64_fwd_kernel(DosxAttn64 d, double scale) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int bq = blockIdx.y, s0 = blockIdx.x * kQ, bk = bq % d.Bk;
  const int Sq = d.Sq, Nk = d.Nk, H = d.H;
  const int64_t q0 = (int64_t)bq * Sq;
  const double* kv = d.kvhat + (int64_t)bk * Nk * H;
  double* P = d.probs + q0 * Nk;
  const float* M = d.drop_mask ? d.drop_mask + q0 * Nk : nullptr;
  const double* Q = d.q + q0 * H;
  const int r = lane & 15, kl = lane >> 4;
  const int n = live_keys(d, bk);

  for (int j0 = wv * 16; j0 < n; j0 += 64) {
    const f64x4 acc = rows_times_keys(d, Q, Sq, s0, kv, n, j0, lane);
    for (int i = 0; i < 4; ++i) {
      const int s = s0 + kl + 4 * i, j = j0 + r;
      if (s < Sq && j < n) P[(int64_t)s * Nk + j] = acc[i] * scale;
    }
  }
  __syncthreads();

  for (int rr = wv; rr < kQ && s0 + rr < Sq; rr += 4) {
    double* row = P + (int64_t)(s0 + rr) * Nk;
    if (d.flags & DOSX_ATTN64_SOFTMAX_F64) {
      double mx = -INFINITY;
      for (int j = lane; j < n; j += 64) mx = fmax(mx, row[j]);
      mx = wave_max64(mx);
      double sum = 0.0;
      for (int j = lane; j < n; j += 64) {
        const double e = exp(row[j] - mx);
        row[j] = e;
        sum += e;
      }
      sum = wave_sum64(sum);
      for (int j = lane; j < n; j += 64) row[j] = row[j] / sum;
    } else {
      // F.softmax(w.float(), -1).type_as(w) (multihead_attention.py:69): fp32 scores, fp32 softmax, promoted
      float mx = -INFINITY;
      for (int j = lane; j < n; j += 64) mx = fmaxf(mx, (float)row[j]);
      mx = wave_max32(mx);
      float sum = 0.0f;
      for (int j = lane; j < n; j += 64) {
        const float e = expf((float)row[j] - mx);
        row[j] = (double)e;
        sum += e;
      }
      sum = wave_sum32(sum);
      for (int j = lane; j < n; j += 64) row[j] = (double)((float)row[j] / sum);
    }
    for (int j = n + lane; j < Nk; j += 64) row[j] = 0.0;
  }
  __syncthreads();

  for (int c0 = wv * 64; c0 < H; c0 += 256) {
    f64x4 acc[4];
    weights_times_values(d, P, M, Sq, s0, kv, n, c0, lane, acc);
    for (int t = 0; t < 4; ++t) {
      const int h = c0 + 16 * t + r;
      if (h >= H) continue;
      for (int i = 0; i < 4; ++i) {
        const int s = s0 + kl + 4 * i;
        if (s < Sq) d.out[(q0 + s) * H + h] = d.x[(q0 + s) * H + h] + acc[t][i];
      }
    }
  }
}

// Backward, query side.  Same tiling as the forward: 1) dP = dout . v^T, times the mask, into ds; 2) the softmax backward
// of each row in place, times H^-1/2; 3) dq = ds . k.  With key_ptr the same bounds as the forward; ds[s][j >= n] = 0.0.
__global__ __launch_bounds__(256) void attn64_dq_kernel(DosxAttn64 d, double scale) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int bq = blockIdx.y, s0 = blockIdx.x * kQ, bk = bq % d.Bk;
  const int Sq = d.Sq, Nk = d.Nk, H = d.H;
  const int64_t q0 = (int64_t)bq * Sq;
  const double* kv = d.kvhat + (int64_t)bk * Nk * H;
  const double* P = d.probs + q0 * Nk;
  double* DS = d.ds + q0 * Nk;
  const float* M = d.drop_mask ? d.drop_mask + q0 * Nk : nullptr;
  const double* DO = d.dout + q0 * H;
  const int r = lane & 15, kl = lane >> 4;
  const int n = live_keys(d, bk);

  for (int j0 = wv * 16; j0 < n; j0 += 64) {
    const f64x4 acc = rows_times_keys(d, DO, Sq, s0, kv, n, j0, lane);
    for (int i = 0; i < 4; ++i) {
      const int s = s0 + kl + 4 * i, j = j0 + r;
      if (s < Sq && j < n) {
        const int64_t o = (int64_t)s * Nk + j;
        DS[o] = M != nullptr ? acc[i] * (double)M[o] : acc[i];
      }
    }
  }
  __syncthreads();

  for (int rr = wv; rr < kQ && s0 + rr < Sq; rr += 4) {
    const double* prow = P + (int64_t)(s0 + rr) * Nk;
    double* row = DS + (int64_t)(s0 + rr) * Nk;
    if (d.flags & DOSX_ATTN64_SOFTMAX_F64) {
      double dot = 0.0;
      for (int j = lane; j < n; j += 64) dot += prow[j] * row[j];
      dot = wave_sum64(dot);
      for (int j = lane; j < n; j += 64) row[j] = prow[j] * (row[j] - dot) * scale;
    } else {
      // autograd of the forward's casts: the fp64 gradient rounded to fp32, softmax backward p (g - sum p g) in fp32,
      // promoted, then the fp64 scaling's backward
      float dot = 0.0f;
      for (int j = lane; j < n; j += 64) dot += (float)prow[j] * (float)row[j];
      dot = wave_sum32(dot);
      for (int j = lane; j < n; j += 64) {
        const float g = (float)row[j];
        row[j] = (double)((g - dot) * (float)prow[j]) * scale;
      }
    }
    for (int j = n + lane; j < Nk; j += 64) row[j] = 0.0;
  }
  __syncthreads();

  for (int c0 = wv * 64; c0 < H; c0 += 256) {
    f64x4 acc[4];
    weights_times_values(d, DS, nullptr, Sq, s0, kv, n, c0, lane, acc);
    for (int t = 0; t < 4; ++t) {
      const int h = c0 + 16 * t + r;
      if (h >= H) continue;
      for (int i = 0; i < 4; ++i) {
        const int s = s0 + kl + 4 * i;
        if (s < Sq) d.dq[(q0 + s) * H + h] = acc[t][i];
      }
    }
  }
}

// Backward, key side: dkv[j] = sum over every query row that reads key j (crystals bq = bk, bk + Bk, ... in order, rows s
// in order) of ds[s][j] q[s] + (p o mask)[s][j] dout[s].  A wave owns 16 keys x 64 columns; nothing else writes them.
// With key_ptr the rows j >= n of the crystal read nothing: their part rows are written as zeros, their dkvhat rows as
// zeros unless accumulate (then left alone); a wave whose whole tile is past n skips the query loop.
__global__ __launch_bounds__(256) void attn64_dkv_kernel(DosxAttn64 d) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int bk = blockIdx.y, j0 = (blockIdx.x * 4 + wv) * kQ, c0 = blockIdx.z * 64;
  if (j0 >= d.Nk) return;                         // wave-uniform
  const int Sq = d.Sq, Nk = d.Nk, H = d.H;
  const int r = lane & 15, kl = lane >> 4;
  const int ja = j0 + r;
  const int n = live_keys(d, bk);
  f64x4 acc[4];
  for (int t = 0; t < 4; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
  for (int bq = bk; bq < d.Bq && j0 < n; bq += d.Bk) {
    const int64_t q0 = (int64_t)bq * Sq;
    const double* DS = d.ds + q0 * Nk;
    const double* P = d.probs + q0 * Nk;
    const float* M = d.drop_mask ? d.drop_mask + q0 * Nk : nullptr;
    for (int sb = 0; sb < Sq; sb += 4) {
      const int s = sb + kl;
      const bool sin = s < Sq;
      double a1 = 0.0, a2 = 0.0;
      if (sin && ja < n) {
        const int64_t o = (int64_t)s * Nk + ja;
        a1 = DS[o];
        a2 = M != nullptr ? P[o] * (double)M[o] : P[o];
      }
      const double* qrow = d.q + (q0 + s) * H;
      const double* grow = d.dout + (q0 + s) * H;
      for (int t = 0; t < 4; ++t) {
        const int h = c0 + 16 * t + r;
        const bool ok = sin && h < H;
        acc[t] = mfma64(a1, ok ? qrow[h] : 0.0, acc[t]);
        acc[t] = mfma64(a2, ok ? grow[h] : 0.0, acc[t]);
      }
    }
  }
  for (int t = 0; t < 4; ++t) {
    const int h = c0 + 16 * t + r;
    if (h >= H) continue;
    for (int i = 0; i < 4; ++i) {
      const int j = j0 + kl + 4 * i;
      if (j >= Nk) continue;
      const int64_t row = (int64_t)bk * Nk + j;
      double* o = d.dkvhat + row * H + h;
      if (j >= n) {
        if (!d.accumulate) *o = 0.0;
        d.part[row * 2 * H + h] = 0.0;
        d.part[row * 2 * H + H + h] = 0.0;
        continue;
      }
      const double g = acc[t][i];
      const double v = g * d.gamma0[h];
      *o = d.accumulate ? *o + v : v;
      d.part[row * 2 * H + h] = g * d.kvhat[row * H + h];
      d.part[row * 2 * H + H + h] = g;
    }
  }
}

// one wave per dense row b * nmax + j: node graph_ptr[b] + j normalised (no affine, eps 1e-5), or a zero ghost row
__global__ __launch_bounds__(256) void dense_rows64_kernel(const double* x, const int32_t* graph_ptr, double* out, double* rstd,
                                                           int B, int nmax, int H) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= B * nmax) return;
  const int b = r / nmax, j = r % nmax;
  const int n = graph_ptr[b] + j;
  double* orow = out + (int64_t)r * H;
  if (n >= graph_ptr[b + 1]) {
    for (int c = lane; c < H; c += 64) orow[c] = 0.0;
    return;
  }
  const double* xr = x + (int64_t)n * H;
  double v[kRowMax];
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < kRowMax; ++i) {
    const int c = lane + 64 * i;
    v[i] = c < H ? xr[c] : 0.0;
    s += v[i];
  }
  const double mean = wave_sum64(s) / H;
  double q = 0.0;
#pragma unroll
  for (int i = 0; i < kRowMax; ++i) {
    const int c = lane + 64 * i;
    const double t = c < H ? v[i] - mean : 0.0;
    q += t * t;
  }
  const double rs = 1.0 / sqrt(wave_sum64(q) / H + 1e-5);
#pragma unroll
  for (int i = 0; i < kRowMax; ++i) {
    const int c = lane + 64 * i;
    if (c < H) orow[c] = (v[i] - mean) * rs;
  }
  if (lane == 0) rstd[n] = rs;
}

__global__ __launch_bounds__(256) void dense_rows64_bwd_kernel(const double* dout, const double* xhat, const double* rstd,
                                                               const int32_t* graph_ptr, double* dx, int B, int nmax, int H,
                                                               int accumulate) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= B * nmax) return;
  const int b = r / nmax, j = r % nmax;
  const int n = graph_ptr[b] + j;
  if (n >= graph_ptr[b + 1]) return;              // ghost row: nothing reaches a node
  const int64_t o = (int64_t)r * H;
  double g[kRowMax], xh[kRowMax];
  double s1 = 0.0, s2 = 0.0;
#pragma unroll
  for (int i = 0; i < kRowMax; ++i) {
    const int c = lane + 64 * i;
    g[i] = c < H ? dout[o + c] : 0.0;
    xh[i] = c < H ? xhat[o + c] : 0.0;
    s1 += g[i];
    s2 += g[i] * xh[i];
  }
  s1 = wave_sum64(s1) / H;
  s2 = wave_sum64(s2) / H;
  const double rs = rstd[n];
  double* dr = dx + (int64_t)n * H;
#pragma unroll
  for (int i = 0; i < kRowMax; ++i) {
    const int c = lane + 64 * i;
    if (c >= H) continue;
    const double v = rs * (g[i] - s1 - xh[i] * s2);
    dr[c] = accumulate ? dr[c] + v : v;
  }
}

__global__ void index_sum64_kernel(const double* src, int ld_src, const int32_t* idx, int n_src, double* dst, int ld_dst,
                                   int n_dst, int W, int accumulate) {
  const int64_t total = (int64_t)n_dst * W;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int i = (int)(t / W), c = (int)(t % W);
    double s = 0.0;
    for (int r = 0; r < n_src; ++r)
      if (idx[r] == i) s += src[(int64_t)r * ld_src + c];
    double* o = dst + (int64_t)i * ld_dst + c;
    *o = accumulate ? *o + s : s;
  }
}

int check_attn(const DosxAttn64* dp, const char* who) {
  DOSX_CHECK_ARG(dp != nullptr, "%s: NULL descriptor", who);
  const DosxAttn64& d = *dp;
  DOSX_CHECK_ARG(d.H >= 1 && d.H <= DOSX_ATTN64_MAX_H, "%s: H=%d (1 <= H <= %d)", who, d.H, DOSX_ATTN64_MAX_H);
  DOSX_CHECK_ARG(d.Sq >= 1 && d.Nk >= 1 && d.Bk >= 1 && d.Bq >= 1, "%s: Sq=%d Nk=%d Bq=%d Bk=%d", who, d.Sq, d.Nk, d.Bq, d.Bk);
  DOSX_CHECK_ARG(d.Bq % d.Bk == 0, "%s: Bq=%d is not a multiple of Bk=%d", who, d.Bq, d.Bk);
  DOSX_CHECK_ARG(d.Bq <= 65535 && ceil_div(d.Sq, kQ) <= 65535 && d.Bk <= 65535, "%s: Sq=%d Bq=%d Bk=%d too large", who, d.Sq,
                 d.Bq, d.Bk);
  DOSX_CHECK_ARG((d.flags & ~DOSX_ATTN64_SOFTMAX_F64) == 0, "%s: flags=%d", who, d.flags);
  DOSX_CHECK_ARG(d.q && d.kvhat && d.gamma0 && d.beta0 && d.probs, "%s: NULL q / kvhat / gamma0 / beta0 / probs", who);
  return 0;
}

}  // namespace

extern "C" int dosx_attention_f64(const DosxAttn64* dp, dosx_stream_t stream) {
  if (int rc = check_attn(dp, "dosx_attention_f64")) return rc;
  const DosxAttn64 d = *dp;
  DOSX_CHECK_ARG(d.x && d.out, "dosx_attention_f64: NULL x / out");
  const double scale = std::pow((double)d.H, -0.5);     // embed_dim ** -0.5 (multihead_attention.py:20)
  hipLaunchKernelGGL(attn64_fwd_kernel, dim3(ceil_div(d.Sq, kQ), d.Bq), dim3(256), 0, to_stream(stream), d, scale);
  DOSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int dosx_attention_bwd_f64(const DosxAttn64* dp, dosx_stream_t stream) {
  if (int rc = check_attn(dp, "dosx_attention_bwd_f64")) return rc;
  const DosxAttn64 d = *dp;
  DOSX_CHECK_ARG(d.dout && d.dq && d.ds && d.dkvhat && d.part, "dosx_attention_bwd_f64: NULL dout / dq / ds / dkvhat / part");
  const double scale = std::pow((double)d.H, -0.5);
  hipLaunchKernelGGL(attn64_dq_kernel, dim3(ceil_div(d.Sq, kQ), d.Bq), dim3(256), 0, to_stream(stream), d, scale);
  DOSX_LAUNCH_CHECK();
  hipLaunchKernelGGL(attn64_dkv_kernel, dim3(ceil_div(ceil_div(d.Nk, kQ), 4), d.Bk, ceil_div(d.H, 64)), dim3(256), 0,
                     to_stream(stream), d);
  DOSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int dosx_dense_rows_f64(const double* x, const int32_t* graph_ptr, double* out, double* rstd, int B, int nmax, int H,
                                   dosx_stream_t stream) {
  DOSX_CHECK_ARG(x && graph_ptr && out && rstd, "dosx_dense_rows_f64: NULL argument");
  DOSX_CHECK_ARG(B >= 0 && nmax >= 1 && H >= 1 && H <= 64 * kRowMax, "dosx_dense_rows_f64: B=%d nmax=%d H=%d (H <= %d)", B,
                 nmax, H, 64 * kRowMax);
  DOSX_CHECK_ARG((int64_t)B * nmax < (1 << 30), "dosx_dense_rows_f64: B*nmax too large");
  if (B == 0) return 0;
  hipLaunchKernelGGL(dense_rows64_kernel, dim3(ceil_div(B * nmax, 4)), dim3(256), 0, to_stream(stream), x, graph_ptr, out, rstd,
                     B, nmax, H);
  DOSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int dosx_dense_rows_bwd_f64(const double* dout, const double* xhat, const double* rstd, const int32_t* graph_ptr,
                                       double* dx, int B, int nmax, int H, int accumulate, dosx_stream_t stream) {
  DOSX_CHECK_ARG(dout && xhat && rstd && graph_ptr && dx, "dosx_dense_rows_bwd_f64: NULL argument");
  DOSX_CHECK_ARG(B >= 0 && nmax >= 1 && H >= 1 && H <= 64 * kRowMax, "dosx_dense_rows_bwd_f64: B=%d nmax=%d H=%d (H <= %d)", B,
                 nmax, H, 64 * kRowMax);
  DOSX_CHECK_ARG((int64_t)B * nmax < (1 << 30), "dosx_dense_rows_bwd_f64: B*nmax too large");
  if (B == 0) return 0;
  hipLaunchKernelGGL(dense_rows64_bwd_kernel, dim3(ceil_div(B * nmax, 4)), dim3(256), 0, to_stream(stream), dout, xhat, rstd,
                     graph_ptr, dx, B, nmax, H, accumulate);
  DOSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int dosx_index_sum_f64(const double* src, int ld_src, const int32_t* idx, int n_src, double* dst, int ld_dst,
                                  int n_dst, int W, int accumulate, dosx_stream_t stream) {
  DOSX_CHECK_ARG(src && idx && dst, "dosx_index_sum_f64: NULL argument");
  DOSX_CHECK_ARG(n_src >= 0 && n_dst >= 0 && W >= 1 && ld_src >= W && ld_dst >= W,
                 "dosx_index_sum_f64: n_src=%d n_dst=%d W=%d ld_src=%d ld_dst=%d", n_src, n_dst, W, ld_src, ld_dst);
  if (n_dst == 0) return 0;
  const int64_t total = (int64_t)n_dst * W;
  hipLaunchKernelGGL(index_sum64_kernel, dim3((int)std::min<int64_t>((total + 255) / 256, 8192)), dim3(256), 0,
                     to_stream(stream), src, ld_src, idx, n_src, dst, ld_dst, n_dst, W, accumulate);
  DOSX_LAUNCH_CHECK();
  return 0;
}
