// Per-crystal training losses with their gradients (include/dosx.h "per-crystal losses"): RMSE, MSE, MAE and Huber of every row
// of a [B,S] batch on its own, averaged over the crystals - the objective of the reference's drivers at batch_size = 1
// (main_phDOS.py:52-55,109-114; main_eDOS.py:111-123) and the three other metrics the project reports (utils.test*).
// One wavefront per crystal, four crystals per 256-thread workgroup (as loss_edos_kernel, csrc/rowops.hip, and csrc/eval.hip);
// lane l takes the elements l, l + 64, ... in order and the 64 lane sums meet in one wave reduction, so a crystal's numbers
// depend on S alone and two runs are bitwise equal.  No fast-math in this build: sqrt and / are correctly rounded.
// kind = RMSE with clamp_target and two outputs repeats loss_edos_kernel's arithmetic operation by operation (same expressions,
// same order, same contraction): dpg, dps and per_crystal[b] / B_global are its bits, loss[0] is sum_kernel's.
// dosx_loss_rows_w / _w_f64 (include/dosx.h "weighted per-crystal losses") are the same kernels under two further template flags:
// W, per-crystal sample weights w_b (read per crystal, or gathered through w_index out of a dataset's table), and BW, energy-bin
// weights v_s with V = sum_s v_s in place of S.  The unweighted entries instantiate the unflagged forms alone.
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

// One crystal by one wavefront: l_b = f(pg_b) (+ beta f(ps_b) with TWO), returned in every lane; the crystal's gradient rows written.
// coef = 1 / B_global, times w_b with W; `zero` (W only): w_b == 0, the rows are +0.0 whatever the crystal holds.
// BW: den = V and every element carries v_s; a bin with v_s == 0 adds nothing to sum and gradient, a NaN in it included.
template <typename T, int KIND, bool TWO, bool W, bool BW>
__device__ __forceinline__ T loss_row(const T* __restrict__ pg, const T* __restrict__ ps, const T* __restrict__ y, size_t o, int S,
                                      int lane, bool clamp, T beta, T delta, T coef, bool zero, const T* __restrict__ bin_w, T den,
                                      T* __restrict__ dpg, T* __restrict__ dps) {
  T a = (T)0, c = (T)0;
  for (int s = lane; s < S; s += 64) {
    const T t = target_of(y[o + s], clamp);
    if constexpr (BW) {
      const T v = bin_w[s];
      if (v != (T)0) {
        a += v * elem_loss<T, KIND>(pg[o + s] - t, delta);
        if constexpr (TWO) c += v * elem_loss<T, KIND>(ps[o + s] - t, delta);
      }
    } else {
      a += elem_loss<T, KIND>(pg[o + s] - t, delta);
      if constexpr (TWO) c += elem_loss<T, KIND>(ps[o + s] - t, delta);
    }
  }
  a = row_sum(a);
  if constexpr (TWO) c = row_sum(c);
  const T r0 = row_term<T, KIND>(a, den);
  const T k0 = row_coef<T, KIND>(coef, r0, den);
  T r1 = (T)0, k1 = (T)0;
  if constexpr (TWO) {
    r1 = row_term<T, KIND>(c, den);
    k1 = row_coef<T, KIND>(beta * coef, r1, den);
  }
  if (W && zero) {
    for (int s = lane; s < S; s += 64) {
      dpg[o + s] = (T)0;
      if constexpr (TWO) dps[o + s] = (T)0;
    }
  } else {
    for (int s = lane; s < S; s += 64) {
      const T t = target_of(y[o + s], clamp);
      if constexpr (BW) {
        const T v = bin_w[s];
        dpg[o + s] = v != (T)0 ? v * elem_grad<T, KIND>(pg[o + s] - t, k0, delta) : (T)0;
        if constexpr (TWO) dps[o + s] = v != (T)0 ? v * elem_grad<T, KIND>(ps[o + s] - t, k1, delta) : (T)0;
      } else {
        dpg[o + s] = elem_grad<T, KIND>(pg[o + s] - t, k0, delta);
        if constexpr (TWO) dps[o + s] = elem_grad<T, KIND>(ps[o + s] - t, k1, delta);
      }
    }
  }
  if constexpr (TWO) return r0 + beta * r1;
  else return r0;
}

template <typename T, int KIND, bool TWO, bool W, bool BW>
__global__ __launch_bounds__(ROWS_THREADS) void loss_rows_kernel(const T* __restrict__ pg, const T* __restrict__ ps,
                                                                 const T* __restrict__ y, int B, int S, int clamp, T beta, T delta,
                                                                 T inv_bglobal, T* __restrict__ dpg, T* __restrict__ dps,
                                                                 T* __restrict__ per_crystal, const T* __restrict__ w,
                                                                 const int32_t* __restrict__ w_index,
                                                                 const T* __restrict__ bin_w) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * ROWS_WAVES + (threadIdx.x >> 6);
  if (b >= B) return;
  T coef = inv_bglobal, den = (T)S;
  bool zero = false;
  if constexpr (W) {
    const T wb = weight_of(w, w_index, b);
    zero = wb == (T)0;
    coef = wb * inv_bglobal;
  }
  if constexpr (BW) den = bin_total(bin_w, S, lane);
  const T l = loss_row<T, KIND, TWO, W, BW>(pg, ps, y, (size_t)b * S, S, lane, clamp != 0, beta, delta, coef, zero, bin_w, den, dpg,
                                            dps);
  if (lane == 0) per_crystal[b] = l;
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

// per_crystal == NULL: nowhere to leave the shares between two launches, so ONE workgroup does both - 256 crystals at a time,
// wave w the crystals w, w + 4, ... of the 256, shares through LDS, then every thread adds its own: the same numbers in the same
// order as the two launches above.
template <typename T, int KIND, bool TWO, bool W, bool BW>
__global__ __launch_bounds__(ROWS_THREADS) void loss_rows_solo_kernel(const T* __restrict__ pg, const T* __restrict__ ps,
                                                                      const T* __restrict__ y, int B, int S, int clamp, T beta,
                                                                      T delta, T inv_bglobal, T* __restrict__ dpg,
                                                                      T* __restrict__ dps, T* __restrict__ loss,
                                                                      const T* __restrict__ w, const int32_t* __restrict__ w_index,
                                                                      const T* __restrict__ bin_w) {
  __shared__ T share[ROWS_THREADS];
  __shared__ T red[ROWS_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  T den = (T)S;
  if constexpr (BW) den = bin_total(bin_w, S, lane);
  T s = (T)0;
  for (int base = 0; base < B; base += ROWS_THREADS) {
    for (int i = wave; i < ROWS_THREADS && base + i < B; i += ROWS_WAVES) {
      T coef = inv_bglobal;
      bool zero = false;
      if constexpr (W) {
        const T wb = weight_of(w, w_index, base + i);
        zero = wb == (T)0;
        coef = wb * inv_bglobal;
      }
      const T l = loss_row<T, KIND, TWO, W, BW>(pg, ps, y, (size_t)(base + i) * S, S, lane, clamp != 0, beta, delta, coef, zero,
                                                bin_w, den, dpg, dps);
      if (lane == 0) share[i] = share_of<T, W>(l, inv_bglobal, w, w_index, base + i);
    }
    __syncthreads();
    if (base + (int)threadIdx.x < B) s += share[threadIdx.x];
    __syncthreads();
  }
  finish_total(s, red, loss);
}

template <typename T>
struct RowsArgs {
  const T *pg, *ps, *y;
  int B, S, B_global, clamp;
  T beta, delta;
  T *dpg, *dps, *per_crystal, *loss;
  const T* w;
  const int32_t* w_index;
  const T* bin_w;
  hipStream_t stream;
};

template <typename T, int KIND, bool TWO, bool W, bool BW>
void launch_rows(const RowsArgs<T>& a) {
  const T inv_bglobal = (T)1 / (T)a.B_global;
  if (a.per_crystal) {
    hipLaunchKernelGGL((loss_rows_kernel<T, KIND, TWO, W, BW>), dim3(ceil_div(a.B, ROWS_WAVES)), dim3(ROWS_THREADS), 0, a.stream,
                       a.pg, a.ps, a.y, a.B, a.S, a.clamp, a.beta, a.delta, inv_bglobal, a.dpg, a.dps, a.per_crystal, a.w, a.w_index,
                       a.bin_w);
    hipLaunchKernelGGL((loss_rows_total_kernel<T, W>), dim3(1), dim3(ROWS_THREADS), 0, a.stream, (const T*)a.per_crystal, a.B,
                       inv_bglobal, a.loss, a.w, a.w_index);
  } else {
    hipLaunchKernelGGL((loss_rows_solo_kernel<T, KIND, TWO, W, BW>), dim3(1), dim3(ROWS_THREADS), 0, a.stream, a.pg, a.ps, a.y, a.B,
                       a.S, a.clamp, a.beta, a.delta, inv_bglobal, a.dpg, a.dps, a.loss, a.w, a.w_index, a.bin_w);
  }
}

template <typename T, int KIND, bool W, bool BW>
void launch_two(const RowsArgs<T>& a) {
  if (a.ps) launch_rows<T, KIND, true, W, BW>(a);
  else launch_rows<T, KIND, false, W, BW>(a);
}

// WEIGHTED = false (dosx_loss_rows / _f64): the unflagged forms alone are instantiated
template <typename T, int KIND, bool WEIGHTED>
void launch_kind(const RowsArgs<T>& a) {
  if constexpr (WEIGHTED) {
    if (a.w && a.bin_w) return launch_two<T, KIND, true, true>(a);
    if (a.bin_w) return launch_two<T, KIND, false, true>(a);
    if (a.w) return launch_two<T, KIND, true, false>(a);
  }
  launch_two<T, KIND, false, false>(a);
}

// [p, p + n) against the [B,S] operand q
template <typename T>
bool inside(const void* p, size_t n, const T* q, size_t count) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return p && q && a < b + count * sizeof(T) && b < a + n;
}

template <typename T, bool WEIGHTED>
int loss_rows(const char* who, const T* pg, const T* ps, const T* y, int B, int S, int B_global, int kind, int clamp_target, T beta,
              T delta, T* dpg, T* dps, T* per_crystal, T* loss, const T* w, const int32_t* w_index, const T* bin_w,
              dosx_stream_t stream) {
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
  if constexpr (WEIGHTED) {
    DOSX_CHECK_ARG(w || !w_index, "%s: w_index selects out of w, which is NULL", who);
    const size_t n = (size_t)B * (size_t)S;
    const struct { const char* name; const void* p; size_t bytes; } extra[] = {
        {"w", w, (w_index ? (size_t)1 : (size_t)B) * sizeof(T)}, {"bin_w", bin_w, (size_t)S * sizeof(T)}};
    for (const auto& e : extra)
      DOSX_CHECK_ARG(!inside(e.p, e.bytes, pg, n) && !inside(e.p, e.bytes, ps, n) && !inside(e.p, e.bytes, y, n) &&
                         !inside(e.p, e.bytes, dpg, n) && !inside(e.p, e.bytes, dps, n),
                     "%s: %s lies inside one of the [B,S] operands pg, ps, y, dpg, dps", who, e.name);
  }
  const RowsArgs<T> a{pg, ps, y, B, S, B_global, clamp_target != 0, beta, delta, dpg, dps, per_crystal, loss, w, w_index, bin_w,
                      to_stream(stream)};
  switch (kind) {
    case DOSX_LOSS_RMSE: launch_kind<T, DOSX_LOSS_RMSE, WEIGHTED>(a); break;
    case DOSX_LOSS_MSE: launch_kind<T, DOSX_LOSS_MSE, WEIGHTED>(a); break;
    case DOSX_LOSS_MAE: launch_kind<T, DOSX_LOSS_MAE, WEIGHTED>(a); break;
    default: launch_kind<T, DOSX_LOSS_HUBER, WEIGHTED>(a); break;
  }
  DOSX_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int dosx_loss_rows(const float* pg, const float* ps, const float* y, int B, int S, int B_global, int kind,
                              int clamp_target, float beta, float delta, float* dpg, float* dps, float* per_crystal, float* loss,
                              dosx_stream_t stream) {
  return loss_rows<float, false>("dosx_loss_rows", pg, ps, y, B, S, B_global, kind, clamp_target, beta, delta, dpg, dps,
                                 per_crystal, loss, nullptr, nullptr, nullptr, stream);
}

extern "C" int dosx_loss_rows_f64(const double* pg, const double* ps, const double* y, int B, int S, int B_global, int kind,
                                  int clamp_target, double beta, double delta, double* dpg, double* dps, double* per_crystal,
                                  double* loss, dosx_stream_t stream) {
  return loss_rows<double, false>("dosx_loss_rows_f64", pg, ps, y, B, S, B_global, kind, clamp_target, beta, delta, dpg, dps,
                                  per_crystal, loss, nullptr, nullptr, nullptr, stream);
}

extern "C" int dosx_loss_rows_w(const float* pg, const float* ps, const float* y, int B, int S, int B_global, int kind,
                                int clamp_target, float beta, float delta, float* dpg, float* dps, float* per_crystal, float* loss,
                                const float* w, const int32_t* w_index, const float* bin_w, dosx_stream_t stream) {
  return loss_rows<float, true>("dosx_loss_rows_w", pg, ps, y, B, S, B_global, kind, clamp_target, beta, delta, dpg, dps,
                                per_crystal, loss, w, w_index, bin_w, stream);
}

extern "C" int dosx_loss_rows_w_f64(const double* pg, const double* ps, const double* y, int B, int S, int B_global, int kind,
                                    int clamp_target, double beta, double delta, double* dpg, double* dps, double* per_crystal,
                                    double* loss, const double* w, const int32_t* w_index, const double* bin_w,
                                    dosx_stream_t stream) {
  return loss_rows<double, true>("dosx_loss_rows_w_f64", pg, ps, y, B, S, B_global, kind, clamp_target, beta, delta, dpg, dps,
                                 per_crystal, loss, w, w_index, bin_w, stream);
}
