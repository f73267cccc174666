// What the per-crystal loss kernels share (csrc/loss_rows.hip, csrc/loss_functional.hip): the element and row helpers of the
// pointwise terms, the sample / bin weight helpers, the final sum over the crystals' shares, and the entries' common refusals.
// Everything here has internal linkage: each of the two files compiles its own copy, expression for expression the same.
#pragma once
#include "common.h"

#include <cmath>

namespace {

constexpr int ROWS_WAVES = 4;       // crystals per workgroup, one wavefront each
constexpr int ROWS_THREADS = 64 * ROWS_WAVES;

__device__ __forceinline__ float row_sum(float v) { return wave_sum(v); }
// double: xor butterfly; both partners of an exchange add the same two numbers, so all 64 lanes end with the same total
__device__ __forceinline__ double row_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ float sqrt_of(float v) { return sqrtf(v); }
__device__ __forceinline__ double sqrt_of(double v) { return sqrt(v); }
__device__ __forceinline__ float abs_of(float v) { return fabsf(v); }
__device__ __forceinline__ double abs_of(double v) { return fabs(v); }
// torch.where(y < 0, 0, y) as loss_edos_kernel spells it: fmax returns the other operand for a NaN, so a NaN TARGET becomes 0
// under clamp_target (documented in dosx.h); without the clamp it stays a NaN
__device__ __forceinline__ float target_of(float y, bool clamp) { return clamp ? fmaxf(y, 0.f) : y; }
__device__ __forceinline__ double target_of(double y, bool clamp) { return clamp ? fmax(y, 0.0) : y; }

// what one residual r = p - t adds to its crystal's sum
template <typename T, int KIND>
__device__ __forceinline__ T elem_loss(T r, T delta) {
  if constexpr (KIND == DOSX_LOSS_RMSE || KIND == DOSX_LOSS_MSE) {
    return r * r;
  } else if constexpr (KIND == DOSX_LOSS_MAE) {
    return abs_of(r);
  } else {
    const T a = abs_of(r);                                  // |r| == delta: quadratic branch (torch.nn.HuberLoss)
    return a <= delta ? (T)0.5 * r * r : delta * (a - (T)0.5 * delta);     // NaN: second branch, stays NaN
  }
}
// f(p_b) from the crystal's sum; den = S, or V = sum_s v_s under bin weights
template <typename T, int KIND>
__device__ __forceinline__ T row_term(T sum, T den) {
  if constexpr (KIND == DOSX_LOSS_RMSE) return sqrt_of(sum / den);
  else return sum / den;
}
// the per-crystal coefficient of the gradient; w = 1 / B_global (times beta for the second output, times w_b under sample weights)
template <typename T, int KIND>
__device__ __forceinline__ T row_coef(T w, T term, T den) {
  if constexpr (KIND == DOSX_LOSS_RMSE) return term == (T)0 ? (T)0 : w / (den * term);     // RMSE 0: zero gradient, never 0 / 0
  else if constexpr (KIND == DOSX_LOSS_MSE) return (T)2 * w / den;
  else return w / den;
}
// d loss[0] / d p of one element.  sign(0) = 0 (torch.sign); a NaN residual gives a NaN on every branch.
template <typename T, int KIND>
__device__ __forceinline__ T elem_grad(T r, T k, T delta) {
  if constexpr (KIND == DOSX_LOSS_RMSE || KIND == DOSX_LOSS_MSE) {
    return r * k;
  } else if constexpr (KIND == DOSX_LOSS_MAE) {
    return r > (T)0 ? k : r < (T)0 ? -k : r == (T)0 ? (T)0 : r;
  } else {
    const T dk = delta * k;
    return abs_of(r) <= delta ? r * k : r > (T)0 ? dk : r < (T)0 ? -dk : r;
  }
}

// The weighted forms (dosx_loss_rows_w): W = per-crystal sample weights w_b, BW = energy-bin weights v_s.  Without either flag
// every function below is the unweighted entry's code, expression for expression.
// w_b: w[b], or w[w_index[b]] out of a whole dataset's table - the gather costs no launch and no [B] staging tensor
template <typename T>
__device__ __forceinline__ T weight_of(const T* __restrict__ w, const int32_t* __restrict__ w_index, int b) {
  return w_index ? w[w_index[b]] : w[b];
}
// V = sum_s v_s by the crystal sums' own loop and reduction: fixed order, the same in every wavefront, no host read of bin_w
template <typename T>
__device__ __forceinline__ T bin_total(const T* __restrict__ bin_w, int S, int lane) {
  T v = (T)0;
  for (int s = lane; s < S; s += 64) v += bin_w[s];
  return row_sum(v);
}

// The tail both forms of the final sum share: thread t holds the sum of the shares t, t + 256, ... in rising order; wave
// reduction, then the four wave totals pairwise - sum_kernel's order (csrc/rowops.hip).
template <typename T>
__device__ __forceinline__ void finish_total(T s, T* red, T* __restrict__ loss) {
  s = row_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) loss[0] = (red[0] + red[1]) + (red[2] + red[3]);
}

// a crystal's share of loss[0]: l_b / B_global; with W (l_b w_b) / B_global, each product rounded (w_b = 1: the unweighted bits),
// and exactly 0 for w_b == 0, whatever l_b is
template <typename T, bool W>
__device__ __forceinline__ T share_of(T l, T inv_bglobal, const T* __restrict__ w, const int32_t* __restrict__ w_index, int b) {
#pragma clang fp contract(off)
  if constexpr (W) {
    const T wb = weight_of(w, w_index, b);
    if (wb == (T)0) return (T)0;
    const T lw = l * wb;
    return lw * inv_bglobal;
  } else {
    return l * inv_bglobal;
  }
}

// loss[0] = sum_b per_crystal[b] / B_global, one workgroup.  Each share is ROUNDED before it is added (what dosx_loss_edos stores
// and dosx_sum reads back): no contraction of the product into the sum here.
template <typename T, bool W>
__global__ __launch_bounds__(ROWS_THREADS) void loss_rows_total_kernel(const T* __restrict__ per_crystal, int B, T inv_bglobal,
                                                                       T* __restrict__ loss, const T* __restrict__ w,
                                                                       const int32_t* __restrict__ w_index) {
#pragma clang fp contract(off)
  __shared__ T red[ROWS_WAVES];
  T s = (T)0;
  for (int i = threadIdx.x; i < B; i += ROWS_THREADS) {
    const T share = share_of<T, W>(per_crystal[i], inv_bglobal, w, w_index, i);
    s += share;
  }
  finish_total(s, red, loss);
}

// [p, p + n) against the [B,S] operand q
template <typename T>
bool inside(const void* p, size_t n, const T* q, size_t count) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return p && q && a < b + count * sizeof(T) && b < a + n;
}

// What every per-crystal loss entry refuses, in dosx_loss_rows's order; `weighted`: the entries that take w, w_index and bin_w.
template <typename T>
int loss_rows_check(const char* who, const T* pg, const T* ps, const T* y, int B, int S, int B_global, int kind, T delta,
                    const T* dpg, const T* dps, const T* loss, bool weighted, const T* w, const int32_t* w_index, const T* bin_w) {
  DOSX_CHECK_ARG(pg && y && dpg && loss, "%s: NULL operand (only ps with dps, and per_crystal, may be NULL)", who);
  DOSX_CHECK_ARG((ps == nullptr) == (dps == nullptr),
                 "%s: ps and dps are both given (two outputs) or both NULL (one output), got ps %s and dps %s", who,
                 ps ? "set" : "NULL", dps ? "set" : "NULL");
  DOSX_CHECK_ARG(B > 0 && S > 0 && B_global > 0, "%s: B=%d S=%d B_global=%d must all be positive", who, B, S, B_global);
  DOSX_CHECK_ARG(kind >= DOSX_LOSS_RMSE && kind <= DOSX_LOSS_HUBER, "%s: kind=%d is not one of DOSX_LOSS_RMSE .. DOSX_LOSS_HUBER",
                 who, kind);
  DOSX_CHECK_ARG(kind != DOSX_LOSS_HUBER || (delta > (T)0 && std::isfinite((double)delta)),
                 "%s: DOSX_LOSS_HUBER needs a finite delta > 0, got %g", who, (double)delta);
  DOSX_CHECK_ARG((size_t)B * (size_t)S < ((size_t)1 << 31), "%s: B*S = %zu elements, at most 2^31 - 1", who,
                 (size_t)B * (size_t)S);
  if (weighted) {
    DOSX_CHECK_ARG(w || !w_index, "%s: w_index selects out of w, which is NULL", who);
    const size_t n = (size_t)B * (size_t)S;
    const struct { const char* name; const void* p; size_t bytes; } extra[] = {
        {"w", w, (w_index ? (size_t)1 : (size_t)B) * sizeof(T)}, {"bin_w", bin_w, (size_t)S * sizeof(T)}};
    for (const auto& e : extra)
      DOSX_CHECK_ARG(!inside(e.p, e.bytes, pg, n) && !inside(e.p, e.bytes, ps, n) && !inside(e.p, e.bytes, y, n) &&
                         !inside(e.p, e.bytes, dpg, n) && !inside(e.p, e.bytes, dps, n),
                     "%s: %s lies inside one of the [B,S] operands pg, ps, y, dpg, dps", who, e.name);
  }
  return 0;
}

}  // namespace

// dosx_loss_rows_w / _w_f64 under another entry's name in its refusals (csrc/loss_rows.hip): what dosx_loss_rows_fn / _fn_f64 run
// without a table or with lam == 0 - the weighted entries' kernels, bit for bit.  Not exported.
template <typename T>
__attribute__((visibility("hidden"))) int dosx_loss_rows_weighted_as(const char* who, const T* pg, const T* ps, const T* y, int B,
                                                                      int S, int B_global, int kind, int clamp_target, T beta,
                                                                      T delta, T* dpg, T* dps, T* per_crystal, T* loss, const T* w,
                                                                      const int32_t* w_index, const T* bin_w, dosx_stream_t stream);
