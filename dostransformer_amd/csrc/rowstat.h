// Two-pass LayerNorm statistics of one row (mean, then the centred second moment, like torch's LayerNorm; eps = DOSX_LN_EPS), in
// the two forms this library has, each with the rounding sequence of the kernels that use it - the sums are grouped differently, so
// the forms are not interchangeable (the LayerNorm epilogues of gemm.hip / mlp2.hip / edge_mlp.hip and the batched statistics of
// attention.hip sum in a third and a fourth order and keep their own code).
#pragma once
#include "common.h"

// Quarter wave per row, the row in registers: lane q16 holds the float4 columns 4 q16 + 64 k, on[k] = the column exists
// (v[k] is zero where it does not).  The row phases of attn_rows.h and ffn.hip's ffn_att_row.
template <int NG>
__device__ __forceinline__ void dosx_row16_stats(const float4 (&v)[NG], const bool (&on)[NG], const float invH, float& mean,
                                                 float& rstd) {
  float t = 0.f;
#pragma unroll
  for (int k = 0; k < NG; ++k) t += (v[k].x + v[k].y) + (v[k].z + v[k].w);
  mean = row16_sum(t) * invH;
  t = 0.f;
#pragma unroll
  for (int k = 0; k < NG; ++k) {
    if (!on[k]) continue;
    const float p0 = v[k].x - mean, p1 = v[k].y - mean, p2 = v[k].z - mean, p3 = v[k].w - mean;
    t += (p0 * p0 + p1 * p1) + (p2 * p2 + p3 * p3);
  }
  rstd = rsqrtf(row16_sum(t) * invH + DOSX_LN_EPS);
}

// Wave per row, the row (H % 4 == 0 floats) re-read from global memory in 256-column steps.  The second pass alone, for a
// caller that formed the mean while it wrote the row (mask_residual_kernel):
__device__ __forceinline__ float dosx_wave_row_rstd(const float* row, const int H, const int lane, const float mean) {
  float s2 = 0.f;
  for (int c = lane * 4; c < H; c += 256) {
    const float4 v = ld4(row + c);
    const float a = v.x - mean, b = v.y - mean, c2 = v.z - mean, d = v.w - mean;
    s2 += a * a + b * b + c2 * c2 + d * d;
  }
  return rsqrtf(wave_sum(s2) / (float)H + DOSX_LN_EPS);
}
__device__ __forceinline__ void dosx_wave_row_stats(const float* row, const int H, const int lane, float& mean, float& rstd) {
  float s1 = 0.f;
  for (int c = lane * 4; c < H; c += 256) {
    const float4 v = ld4(row + c);
    s1 += v.x + v.y + v.z + v.w;
  }
  mean = wave_sum(s1) / (float)H;
  rstd = dosx_wave_row_rstd(row, H, lane, mean);
}
// ... and out = (row - mean) rstd; returns rstd
__device__ __forceinline__ float dosx_wave_rownorm(const float* __restrict__ row, float* __restrict__ out, const int H, const int lane) {
  float mean, rstd;
  dosx_wave_row_stats(row, H, lane, mean, rstd);
  for (int c = lane * 4; c < H; c += 256) {
    const float4 v = ld4(row + c);
    st4(out + c, make_float4((v.x - mean) * rstd, (v.y - mean) * rstd, (v.z - mean) * rstd, (v.w - mean) * rstd));
  }
  return rstd;
}
