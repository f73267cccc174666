// float64 kernels of the phonon program (include/dosx.h, "float64 program").  The reference trains the phonon models in
// float64 (main_phDOS.py:15-16); these kernels give a float64 module float64 arithmetic end to end.  They are written for
// clarity first: one MFMA shape, operands read straight from global memory (L1 / L2 serve the reuse), every reduction in
// a fixed order so that two runs are bitwise equal.  Nothing here is shared with the fp32 kernels.
#include "common.h"

typedef double f64x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int kTile = 64;   // output tile of the GEMM / weight-gradient workgroups: 4 waves x (16 rows x 64 columns)

__device__ __forceinline__ double wave_sum64(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// v_mfma_f64_16x16x4_f64: lane l supplies A[l & 15][k = l >> 4] and B[k = l >> 4][l & 15]; result register i of lane l
// is C[row (l >> 4) + 4 i][col l & 15] - NOT the f32 16x16x4 map (row 4 (l >> 4) + i).
__device__ __forceinline__ f64x4 mfma64(double a, double b, f64x4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

__global__ __launch_bounds__(256) void gemm64_kernel(DosxGemm64 d) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int row0 = blockIdx.y * kTile + wv * 16;
  if (row0 >= d.M) return;                        // wave-uniform
  const int col0 = blockIdx.x * kTile;
  const int ar = row0 + (lane & 15), kl = lane >> 4;
  f64x4 acc[4];
  for (int j = 0; j < 4; ++j) acc[j] = f64x4{0.0, 0.0, 0.0, 0.0};
  int kg = 0;
  for (int s = 0; s < d.nseg; ++s) {
    const DosxSeg64 sg = d.a[s];
    const double* arow = ar < d.M ? sg.p + (int64_t)dosx_map_row(sg.map, ar) * sg.ld : nullptr;
    for (int k0 = 0; k0 < sg.width; k0 += 4) {
      const int k = k0 + kl;
      const bool kin = k < sg.width;
      const double a = (arow != nullptr && kin) ? arow[k] : 0.0;
      const int64_t kw = kg + k;
      for (int j = 0; j < 4; ++j) {
        const int col = col0 + 16 * j + (lane & 15);
        double b = 0.0;
        if (kin && col < d.N) b = d.w_layout == 0 ? d.w[(int64_t)col * d.ldw + kw] : d.w[kw * d.ldw + col];
        acc[j] = mfma64(a, b, acc[j]);
      }
    }
    kg += sg.width;
  }
  const double alpha = d.act == DOSX_ACT64_PRELU ? *d.alpha : 0.0;
  for (int j = 0; j < 4; ++j) {
    const int col = col0 + 16 * j + (lane & 15);
    if (col >= d.N) continue;
    const double bias = d.bias ? d.bias[col] : 0.0;
    for (int i = 0; i < 4; ++i) {
      const int row = row0 + (lane >> 4) + 4 * i;
      if (row >= d.M) continue;
      double v = acc[j][i] + bias;
      if (d.pre) d.pre[(int64_t)row * d.ldo + col] = v;
      if (d.act == DOSX_ACT64_RELU) v = v > 0.0 ? v : 0.0;
      else if (d.act == DOSX_ACT64_LEAKY) v = v > 0.0 ? v : 0.01 * v;
      else if (d.act == DOSX_ACT64_PRELU) v = v >= 0.0 ? v : alpha * v;
      if (d.res) v += d.res[(int64_t)row * d.ldr + col];
      d.out[(int64_t)row * d.ldo + col] = v;
    }
  }
}

// dw[n][c] = sum_m dy[m][n] * X[m][c]: A = dy^T (row n, k = m), B = X (k = m, column c).  Workgroup: 64 n x 64 c, one
// row range of M (blockIdx.z of nsplit).
__global__ __launch_bounds__(256) void wgrad64_kernel(DosxWgrad64 d, int chunk) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int n0 = blockIdx.y * kTile + wv * 16;
  if (n0 >= d.N) return;                          // wave-uniform
  const int c0 = blockIdx.x * kTile;
  const int m_begin = blockIdx.z * chunk, m_end = min(d.M, m_begin + chunk);
  const int na = n0 + (lane & 15), kl = lane >> 4;
  // the X column (segment, column in it) this lane supplies for each of the 4 sub-tiles
  const double* xp[4];
  int xld[4];
  DosxRowMap xmap[4];
  for (int j = 0; j < 4; ++j) {
    int c = c0 + 16 * j + (lane & 15);
    xp[j] = nullptr;
    xld[j] = 0;
    xmap[j] = d.x[0].map;
    if (c < d.K) {
      int s = 0;
      while (c >= d.x[s].width) c -= d.x[s++].width;
      xp[j] = d.x[s].p + c;
      xld[j] = d.x[s].ld;
      xmap[j] = d.x[s].map;
    }
  }
  f64x4 acc[4];
  for (int j = 0; j < 4; ++j) acc[j] = f64x4{0.0, 0.0, 0.0, 0.0};
  for (int m0 = m_begin; m0 < m_end; m0 += 4) {
    const int m = m0 + kl;
    const bool min_ = m < m_end;
    const double a = (min_ && na < d.N) ? d.dy[(int64_t)m * d.lddy + na] : 0.0;
    for (int j = 0; j < 4; ++j) {
      const double b = (min_ && xp[j] != nullptr) ? xp[j][(int64_t)dosx_map_row(xmap[j], m) * xld[j]] : 0.0;
      acc[j] = mfma64(a, b, acc[j]);
    }
  }
  const bool direct = d.nsplit == 1;
  for (int j = 0; j < 4; ++j) {
    const int c = c0 + 16 * j + (lane & 15);
    if (c >= d.K) continue;
    for (int i = 0; i < 4; ++i) {
      const int n = n0 + (lane >> 4) + 4 * i;
      if (n >= d.N) continue;
      if (direct) {
        double* o = d.dw + (int64_t)n * d.ldd + c;
        *o = d.accumulate ? *o + acc[j][i] : acc[j][i];
      } else {
        d.partials[((int64_t)blockIdx.z * d.N + n) * d.K + c] = acc[j][i];
      }
    }
  }
}

__global__ void wgrad64_reduce_kernel(DosxWgrad64 d) {
  const int64_t total = (int64_t)d.N * d.K;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    double s = 0.0;
    for (int z = 0; z < d.nsplit; ++z) s += d.partials[z * total + t];
    const int n = (int)(t / d.K), c = (int)(t % d.K);
    double* o = d.dw + (int64_t)n * d.ldd + c;
    *o = d.accumulate ? *o + s : s;
  }
}

// out[c] (+)= sum over the rows [y * rows_per, ...) of column c, in row order (one thread per column)
__global__ void colsum64_kernel(const double* src, int M, int N, int ld, int rows_per, double* dst, int accumulate) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= N) return;
  const int r0 = blockIdx.y * rows_per, r1 = min(M, r0 + rows_per);
  double s = 0.0;
  for (int r = r0; r < r1; ++r) s += src[(int64_t)r * ld + c];
  double* o = dst + (int64_t)blockIdx.y * N + c;
  *o = accumulate ? *o + s : s;
}

constexpr int kRowMax = 1024 / 64;   // values per lane of a LayerNorm row (W <= 1024)

// one wave per row
__global__ __launch_bounds__(256) void layernorm64_kernel(const double* z, const double* gamma, const double* beta,
                                                          const double* alpha, double* xhat, double* rstd, double* out,
                                                          int M, int W) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= M) return;
  const double* zr = z + (int64_t)r * W;
  double v[kRowMax];
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < kRowMax; ++i) {
    const int c = lane + 64 * i;
    v[i] = c < W ? zr[c] : 0.0;
    s += v[i];
  }
  const double mean = wave_sum64(s) / W;
  double q = 0.0;
#pragma unroll
  for (int i = 0; i < kRowMax; ++i) {
    const int c = lane + 64 * i;
    const double t = c < W ? v[i] - mean : 0.0;
    q += t * t;
  }
  const double rs = 1.0 / sqrt(wave_sum64(q) / W + 1e-5);
  const double a = alpha ? *alpha : 0.0;
#pragma unroll
  for (int i = 0; i < kRowMax; ++i) {
    const int c = lane + 64 * i;
    if (c >= W) continue;
    const double xh = (v[i] - mean) * rs;
    double y = xh * gamma[c] + beta[c];
    if (alpha) y = y >= 0.0 ? y : a * y;
    xhat[(int64_t)r * W + c] = xh;
    out[(int64_t)r * W + c] = y;
  }
  if (lane == 0) rstd[r] = rs;
}

__global__ __launch_bounds__(256) void layernorm64_bwd_kernel(const double* dout, const double* xhat, const double* rstd,
                                                              const double* gamma, const double* beta, const double* alpha,
                                                              double* dz, double* part, int M, int W) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= M) return;
  const int64_t o = (int64_t)r * W;
  double* pr = part + (int64_t)r * (2 * W + 1);
  const double a = alpha ? *alpha : 0.0;
  double dxh[kRowMax], xh[kRowMax];
  double s1 = 0.0, s2 = 0.0, sa = 0.0;
#pragma unroll
  for (int i = 0; i < kRowMax; ++i) {
    const int c = lane + 64 * i;
    dxh[i] = xh[i] = 0.0;
    if (c >= W) continue;
    xh[i] = xhat[o + c];
    double g = dout[o + c];
    if (alpha) {
      const double y = xh[i] * gamma[c] + beta[c];
      if (y < 0.0) {
        sa += g * y;
        g *= a;
      }
    }
    pr[c] = g * xh[i];
    pr[W + c] = g;
    dxh[i] = g * gamma[c];
    s1 += dxh[i];
    s2 += dxh[i] * xh[i];
  }
  s1 = wave_sum64(s1) / W;
  s2 = wave_sum64(s2) / W;
  sa = wave_sum64(sa);
  const double rs = rstd[r];
#pragma unroll
  for (int i = 0; i < kRowMax; ++i) {
    const int c = lane + 64 * i;
    if (c < W) dz[o + c] = rs * (dxh[i] - s1 - xh[i] * s2);
  }
  if (lane == 0) pr[2 * W] = sa;
}

// one wave per row
__global__ __launch_bounds__(256) void act64_bwd_kernel(const double* dy, const double* z, int ld, int act, const double* alpha,
                                                        double* dz, double* part, int M, int W) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= M) return;
  const double a = act == DOSX_ACT64_PRELU ? *alpha : 0.0;
  double sa = 0.0;
  for (int c = lane; c < W; c += 64) {
    const double g = dy[(int64_t)r * W + c], v = z[(int64_t)r * ld + c];
    double out;
    if (act == DOSX_ACT64_RELU) out = v > 0.0 ? g : 0.0;
    else if (act == DOSX_ACT64_LEAKY) out = v > 0.0 ? g : g * 0.01;
    else {
      out = v >= 0.0 ? g : g * a;
      if (v < 0.0) sa += g * v;
    }
    dz[(int64_t)r * W + c] = out;
  }
  if (act == DOSX_ACT64_PRELU) {
    sa = wave_sum64(sa);
    if (lane == 0) part[r] = sa;
  }
}

__global__ void edge_feat64_kernel(const double* vec, double* out, int E, double r_max) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  const double x = vec[3 * (int64_t)e], y = vec[3 * (int64_t)e + 1], z = vec[3 * (int64_t)e + 2];
  const double len = sqrt(x * x + y * y + z * z);
  const double inv = 1.0 / fmax(len, 1e-12);
  const double u = 2.0 * (len / r_max - 1.0);
  double cut = (1.0 - cos(M_PI * u)) / 2.0;
  if (u > 0.0) cut = 0.0;
  if (u < -1.0) cut = 1.0;
  const double s3 = sqrt(3.0);
  double* o = out + 4 * (int64_t)e;
  o[0] = cut;
  o[1] = cut * (s3 * (x * inv));
  o[2] = cut * (s3 * (y * inv));
  o[3] = cut * (s3 * (z * inv));
}

__global__ void segment_mean64_kernel(const double* src, const int32_t* rowptr, double* out, int N, int H) {
  const int64_t total = (int64_t)N * H;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int n = (int)(t / H), c = (int)(t % H);
    const int e0 = rowptr[n], e1 = rowptr[n + 1];
    double s = 0.0;
    for (int e = e0; e < e1; ++e) s += src[(int64_t)e * H + c];
    out[t] = s / (double)max(e1 - e0, 1);
  }
}

__global__ void segment_mean64_bwd_kernel(const double* dagg, int ld_dagg, const int32_t* dst, const int32_t* rowptr,
                                          const double* res, double* out, int E, int H) {
  const int64_t total = (int64_t)E * H;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int e = (int)(t / H), c = (int)(t % H);
    const int n = dst[e];
    const double v = dagg[(int64_t)n * ld_dagg + c] / (double)max(rowptr[n + 1] - rowptr[n], 1);
    out[t] = res ? res[t] + v : v;
  }
}

__global__ void gather64_bwd_kernel(const double* dcat, int ldc, const int32_t* rowptr_src, const int32_t* perm_src,
                                    const int32_t* rowptr_dst, const double* base0, int ld0, const double* base1, int ld1,
                                    double* dx, int N, int H) {
  const int64_t total = (int64_t)N * H;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int n = (int)(t / H), c = (int)(t % H);
    double s = 0.0;
    if (base0) s += base0[(int64_t)n * ld0 + c];
    if (base1) s += base1[(int64_t)n * ld1 + c];
    double g = 0.0;
    for (int k = rowptr_src[n]; k < rowptr_src[n + 1]; ++k) g += dcat[(int64_t)perm_src[k] * ldc + c];
    for (int e = rowptr_dst[n]; e < rowptr_dst[n + 1]; ++e) g += dcat[(int64_t)e * ldc + H + c];
    dx[t] = s + g;
  }
}

__global__ void graph_pool64_kernel(const double* x, const int32_t* graph_ptr, double* out, int B, int H) {
  const int64_t total = (int64_t)B * H;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int b = (int)(t / H), c = (int)(t % H);
    double s = 0.0;
    for (int n = graph_ptr[b]; n < graph_ptr[b + 1]; ++n) s += x[(int64_t)n * H + c];
    out[t] = s;
  }
}

__global__ void rows_add64_kernel(const double* a, int lda, const int32_t* ia, const double* b, int ldb, const int32_t* ib,
                                  double* out, int ldo, int M, int W) {
  const int64_t total = (int64_t)M * W;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(t / W), c = (int)(t % W);
    double v = a[(int64_t)(ia ? ia[r] : r) * lda + c];
    if (b) v += b[(int64_t)(ib ? ib[r] : r) * ldb + c];
    out[(int64_t)r * ldo + c] = v;
  }
}

__global__ void reduce_rows64_kernel(const double* src, int ld_src, double* dst, int ld_dst, int n_out, int n_red,
                                     int stride_out, int stride_red, int width, int accumulate) {
  const int64_t total = (int64_t)n_out * width;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int i = (int)(t / width), c = (int)(t % width);
    double s = 0.0;
    for (int j = 0; j < n_red; ++j) s += src[((int64_t)i * stride_out + (int64_t)j * stride_red) * ld_src + c];
    double* o = dst + (int64_t)i * ld_dst + c;
    *o = accumulate ? *o + s : s;
  }
}

inline int elem_grid(int64_t total) { return (int)std::min<int64_t>((total + 255) / 256, 8192); }

int check_seg(const DosxSeg64& s, int i) {
  DOSX_CHECK_ARG(s.p != nullptr, "segment %d: NULL data", i);
  DOSX_CHECK_ARG(s.width >= 1 && s.ld >= s.width, "segment %d: width=%d ld=%d", i, s.width, s.ld);
  DOSX_CHECK_ARG(s.map.d >= 1, "segment %d: row map d=%d", i, s.map.d);
  return 0;
}

}  // namespace

extern "C" int dosx_gemm_f64(const DosxGemm64* dp, dosx_stream_t stream) {
  DOSX_CHECK_ARG(dp != nullptr, "dosx_gemm_f64: NULL descriptor");
  const DosxGemm64 d = *dp;
  DOSX_CHECK_ARG(d.M >= 0 && d.N >= 1 && d.K >= 1, "dosx_gemm_f64: M=%d N=%d K=%d", d.M, d.N, d.K);
  DOSX_CHECK_ARG(d.nseg >= 1 && d.nseg <= 3, "dosx_gemm_f64: nseg=%d", d.nseg);
  int k = 0;
  for (int i = 0; i < d.nseg; ++i) {
    if (int rc = check_seg(d.a[i], i)) return rc;
    k += d.a[i].width;
  }
  DOSX_CHECK_ARG(k == d.K, "dosx_gemm_f64: segment widths sum to %d, K=%d", k, d.K);
  DOSX_CHECK_ARG(d.w != nullptr && d.out != nullptr, "dosx_gemm_f64: NULL w / out");
  DOSX_CHECK_ARG(d.w_layout == 0 || d.w_layout == 1, "dosx_gemm_f64: w_layout=%d", d.w_layout);
  DOSX_CHECK_ARG(d.ldw >= (d.w_layout == 0 ? d.K : d.N), "dosx_gemm_f64: ldw=%d", d.ldw);
  DOSX_CHECK_ARG(d.ldo >= d.N, "dosx_gemm_f64: ldo=%d < N=%d", d.ldo, d.N);
  DOSX_CHECK_ARG(d.act >= DOSX_ACT64_NONE && d.act <= DOSX_ACT64_PRELU, "dosx_gemm_f64: act=%d", d.act);
  DOSX_CHECK_ARG(d.act != DOSX_ACT64_PRELU || d.alpha != nullptr, "dosx_gemm_f64: PReLU without alpha");
  DOSX_CHECK_ARG(d.res == nullptr || d.ldr >= d.N, "dosx_gemm_f64: ldr=%d < N=%d", d.ldr, d.N);
  if (d.M == 0) return 0;
  dim3 grid(ceil_div(d.N, kTile), ceil_div(d.M, kTile));
  DOSX_CHECK_ARG(grid.y <= 65535, "dosx_gemm_f64: M=%d too large", d.M);
  hipLaunchKernelGGL(gemm64_kernel, grid, dim3(256), 0, to_stream(stream), d);
  DOSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int dosx_wgrad_f64(const DosxWgrad64* dp, dosx_stream_t stream) {
  DOSX_CHECK_ARG(dp != nullptr, "dosx_wgrad_f64: NULL descriptor");
  const DosxWgrad64 d = *dp;
  DOSX_CHECK_ARG(d.M >= 0 && d.N >= 1 && d.K >= 1, "dosx_wgrad_f64: M=%d N=%d K=%d", d.M, d.N, d.K);
  DOSX_CHECK_ARG(d.nseg >= 1 && d.nseg <= 3, "dosx_wgrad_f64: nseg=%d", d.nseg);
  int k = 0;
  for (int i = 0; i < d.nseg; ++i) {
    if (int rc = check_seg(d.x[i], i)) return rc;
    k += d.x[i].width;
  }
  DOSX_CHECK_ARG(k == d.K, "dosx_wgrad_f64: segment widths sum to %d, K=%d", k, d.K);
  DOSX_CHECK_ARG(d.dy != nullptr && d.lddy >= d.N, "dosx_wgrad_f64: dy=%p lddy=%d", (const void*)d.dy, d.lddy);
  DOSX_CHECK_ARG(d.dw != nullptr && d.ldd >= d.K, "dosx_wgrad_f64: dw=%p ldd=%d", (void*)d.dw, d.ldd);
  DOSX_CHECK_ARG(d.nsplit >= 1 && d.nsplit <= 1024, "dosx_wgrad_f64: nsplit=%d", d.nsplit);
  DOSX_CHECK_ARG(d.nsplit == 1 || d.partials != nullptr, "dosx_wgrad_f64: nsplit=%d needs partials", d.nsplit);
  DosxWgrad64 e = d;
  if (d.M == 0) {   // empty sum: dw = 0 (or unchanged)
    if (!d.accumulate) {
      const hipError_t err = hipMemset2DAsync(d.dw, sizeof(double) * d.ldd, 0, sizeof(double) * d.K, d.N, to_stream(stream));
      DOSX_CHECK_ARG(err == hipSuccess, "dosx_wgrad_f64: clearing dw failed: %s", hipGetErrorString(err));
    }
    return 0;
  }
  const int chunk = (ceil_div(d.M, d.nsplit) + 3) / 4 * 4;
  e.nsplit = ceil_div(d.M, chunk);                 // row ranges that are not empty
  dim3 grid(ceil_div(d.K, kTile), ceil_div(d.N, kTile), e.nsplit);
  DOSX_CHECK_ARG(grid.y <= 65535, "dosx_wgrad_f64: N=%d too large", d.N);
  hipLaunchKernelGGL(wgrad64_kernel, grid, dim3(256), 0, to_stream(stream), e, chunk);
  DOSX_LAUNCH_CHECK();
  if (e.nsplit > 1) {
    hipLaunchKernelGGL(wgrad64_reduce_kernel, dim3(elem_grid((int64_t)d.N * d.K)), dim3(256), 0, to_stream(stream), e);
    DOSX_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int dosx_colsum_f64(const double* src, int M, int N, int ld, double* partials, double* out, int accumulate,
                               dosx_stream_t stream) {
  DOSX_CHECK_ARG(src != nullptr && out != nullptr, "dosx_colsum_f64: NULL src / out");
  DOSX_CHECK_ARG(M >= 0 && N >= 1 && ld >= N, "dosx_colsum_f64: M=%d N=%d ld=%d", M, N, ld);
  DOSX_CHECK_ARG(M <= DOSX_COLSUM64_ROWS || partials != nullptr, "dosx_colsum_f64: M=%d needs partials", M);
  const dim3 blk(64);
  if (M <= DOSX_COLSUM64_ROWS) {
    hipLaunchKernelGGL(colsum64_kernel, dim3(ceil_div(N, 64), 1), blk, 0, to_stream(stream), src, M, N, ld, M, out, accumulate);
    DOSX_LAUNCH_CHECK();
    return 0;
  }
  const int nb = ceil_div(M, DOSX_COLSUM64_ROWS);
  DOSX_CHECK_ARG(nb <= 65535, "dosx_colsum_f64: M=%d too large", M);
  hipLaunchKernelGGL(colsum64_kernel, dim3(ceil_div(N, 64), nb), blk, 0, to_stream(stream), src, M, N, ld,
                     DOSX_COLSUM64_ROWS, partials, 0);
  DOSX_LAUNCH_CHECK();
  hipLaunchKernelGGL(colsum64_kernel, dim3(ceil_div(N, 64), 1), blk, 0, to_stream(stream), (const double*)partials, nb, N, N,
                     nb, out, accumulate);
  DOSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int dosx_layernorm_f64(const double* z, const double* gamma, const double* beta, const double* alpha,
                                  double* xhat, double* rstd, double* out, int M, int W, dosx_stream_t stream) {
  DOSX_CHECK_ARG(z && gamma && beta && xhat && rstd && out, "dosx_layernorm_f64: NULL argument");
  DOSX_CHECK_ARG(M >= 0 && W >= 1 && W <= 64 * kRowMax, "dosx_layernorm_f64: M=%d W=%d (W <= %d)", M, W, 64 * kRowMax);
  if (M == 0) return 0;
  hipLaunchKernelGGL(layernorm64_kernel, dim3(ceil_div(M, 4)), dim3(256), 0, to_stream(stream), z, gamma, beta, alpha, xhat,
                     rstd, out, M, W);
  DOSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int dosx_layernorm_bwd_f64(const double* dout, const double* xhat, const double* rstd, const double* gamma,
                                      const double* beta, const double* alpha, double* dz, double* part, int M, int W,
                                      dosx_stream_t stream) {
  DOSX_CHECK_ARG(dout && xhat && rstd && gamma && beta && dz && part, "dosx_layernorm_bwd_f64: NULL argument");
  DOSX_CHECK_ARG(M >= 0 && W >= 1 && W <= 64 * kRowMax, "dosx_layernorm_bwd_f64: M=%d W=%d (W <= %d)", M, W, 64 * kRowMax);
  if (M == 0) return 0;
  hipLaunchKernelGGL(layernorm64_bwd_kernel, dim3(ceil_div(M, 4)), dim3(256), 0, to_stream(stream), dout, xhat, rstd, gamma,
                     beta, alpha, dz, part, M, W);
  DOSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int dosx_act_bwd_f64(const double* dy, const double* z, int ld, int act, const double* alpha, double* dz,
                                double* part, int M, int W, dosx_stream_t stream) {
  DOSX_CHECK_ARG(dy && z && dz, "dosx_act_bwd_f64: NULL argument");
  DOSX_CHECK_ARG(M >= 0 && W >= 1 && ld >= W, "dosx_act_bwd_f64: M=%d W=%d ld=%d", M, W, ld);
  DOSX_CHECK_ARG(act >= DOSX_ACT64_RELU && act <= DOSX_ACT64_PRELU, "dosx_act_bwd_f64: act=%d", act);
  DOSX_CHECK_ARG(act != DOSX_ACT64_PRELU || (alpha && part), "dosx_act_bwd_f64: PReLU needs alpha and part");
  if (M == 0) return 0;
  hipLaunchKernelGGL(act64_bwd_kernel, dim3(ceil_div(M, 4)), dim3(256), 0, to_stream(stream), dy, z, ld, act, alpha, dz, part,
                     M, W);
  DOSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int dosx_edge_feat_sh1_f64(const double* edge_vec, double* out, int E, double r_max, dosx_stream_t stream) {
  DOSX_CHECK_ARG(edge_vec && out, "dosx_edge_feat_sh1_f64: NULL argument");
  DOSX_CHECK_ARG(E >= 0 && r_max > 0.0, "dosx_edge_feat_sh1_f64: E=%d r_max=%g", E, r_max);
  if (E == 0) return 0;
  hipLaunchKernelGGL(edge_feat64_kernel, dim3(ceil_div(E, 256)), dim3(256), 0, to_stream(stream), edge_vec, out, E, r_max);
  DOSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int dosx_segment_mean_f64(const double* src, const int32_t* rowptr, double* out, int N, int H,
                                     dosx_stream_t stream) {
  DOSX_CHECK_ARG(src && rowptr && out, "dosx_segment_mean_f64: NULL argument");
  DOSX_CHECK_ARG(N >= 0 && H >= 1, "dosx_segment_mean_f64: N=%d H=%d", N, H);
  if (N == 0) return 0;
  hipLaunchKernelGGL(segment_mean64_kernel, dim3(elem_grid((int64_t)N * H)), dim3(256), 0, to_stream(stream), src, rowptr, out,
                     N, H);
  DOSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int dosx_segment_mean_bwd_f64(const double* dagg, int ld_dagg, const int32_t* dst, const int32_t* rowptr,
                                         const double* res, double* out, int E, int H, dosx_stream_t stream) {
  DOSX_CHECK_ARG(dagg && dst && rowptr && out, "dosx_segment_mean_bwd_f64: NULL argument");
  DOSX_CHECK_ARG(E >= 0 && H >= 1 && ld_dagg >= H, "dosx_segment_mean_bwd_f64: E=%d H=%d ld_dagg=%d", E, H, ld_dagg);
  if (E == 0) return 0;
  hipLaunchKernelGGL(segment_mean64_bwd_kernel, dim3(elem_grid((int64_t)E * H)), dim3(256), 0, to_stream(stream), dagg, ld_dagg,
                     dst, rowptr, res, out, E, H);
  DOSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int dosx_gather_bwd_f64(const double* dcat, int ldc, const int32_t* rowptr_src, const int32_t* perm_src,
                                   const int32_t* rowptr_dst, const double* base0, int ld0, const double* base1, int ld1,
                                   double* dx, int N, int H, dosx_stream_t stream) {
  DOSX_CHECK_ARG(dcat && rowptr_src && perm_src && rowptr_dst && dx, "dosx_gather_bwd_f64: NULL argument");
  DOSX_CHECK_ARG(N >= 0 && H >= 1 && ldc >= 2 * H, "dosx_gather_bwd_f64: N=%d H=%d ldc=%d", N, H, ldc);
  DOSX_CHECK_ARG((!base0 || ld0 >= H) && (!base1 || ld1 >= H), "dosx_gather_bwd_f64: ld0=%d ld1=%d", ld0, ld1);
  if (N == 0) return 0;
  hipLaunchKernelGGL(gather64_bwd_kernel, dim3(elem_grid((int64_t)N * H)), dim3(256), 0, to_stream(stream), dcat, ldc,
                     rowptr_src, perm_src, rowptr_dst, base0, ld0, base1, ld1, dx, N, H);
  DOSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int dosx_graph_pool_f64(const double* x, const int32_t* graph_ptr, double* out, int B, int H, dosx_stream_t stream) {
  DOSX_CHECK_ARG(x && graph_ptr && out, "dosx_graph_pool_f64: NULL argument");
  DOSX_CHECK_ARG(B >= 0 && H >= 1, "dosx_graph_pool_f64: B=%d H=%d", B, H);
  if (B == 0) return 0;
  hipLaunchKernelGGL(graph_pool64_kernel, dim3(elem_grid((int64_t)B * H)), dim3(256), 0, to_stream(stream), x, graph_ptr, out, B,
                     H);
  DOSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int dosx_rows_add_f64(const double* a, int lda, const int32_t* ia, const double* b, int ldb, const int32_t* ib,
                                 double* out, int ldo, int M, int W, dosx_stream_t stream) {
  DOSX_CHECK_ARG(a && out, "dosx_rows_add_f64: NULL a / out");
  DOSX_CHECK_ARG(M >= 0 && W >= 1 && lda >= W && ldo >= W && (!b || ldb >= W), "dosx_rows_add_f64: M=%d W=%d lda=%d ldb=%d ldo=%d",
                 M, W, lda, ldb, ldo);
  if (M == 0) return 0;
  hipLaunchKernelGGL(rows_add64_kernel, dim3(elem_grid((int64_t)M * W)), dim3(256), 0, to_stream(stream), a, lda, ia, b, ldb, ib,
                     out, ldo, M, W);
  DOSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int dosx_reduce_rows_f64(const double* src, int ld_src, double* dst, int ld_dst, int n_out, int n_red, int stride_out,
                                    int stride_red, int width, int accumulate, dosx_stream_t stream) {
  DOSX_CHECK_ARG(src && dst, "dosx_reduce_rows_f64: NULL argument");
  DOSX_CHECK_ARG(n_out >= 0 && n_red >= 0 && width >= 1 && ld_src >= width && ld_dst >= width && stride_out >= 0 && stride_red >= 0,
                 "dosx_reduce_rows_f64: n_out=%d n_red=%d width=%d", n_out, n_red, width);
  if (n_out == 0) return 0;
  hipLaunchKernelGGL(reduce_rows64_kernel, dim3(elem_grid((int64_t)n_out * width)), dim3(256), 0, to_stream(stream), src, ld_src,
                     dst, ld_dst, n_out, n_red, stride_out, stride_red, width, accumulate);
  DOSX_LAUNCH_CHECK();
  return 0;
}
