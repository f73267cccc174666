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
// The element and row helpers, the final sum and the entries' refusals are in loss_rows.h, shared with csrc/loss_functional.hip.
#include "loss_rows.h"

namespace {

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

template <typename T, bool WEIGHTED>
int loss_rows(const char* who, const T* pg, const T* ps, const T* y, int B, int S, int B_global, int kind, int clamp_target, T beta,
              T delta, T* dpg, T* dps, T* per_crystal, T* loss, const T* w, const int32_t* w_index, const T* bin_w,
              dosx_stream_t stream) {
  if (const int rc = loss_rows_check<T>(who, pg, ps, y, B, S, B_global, kind, delta, dpg, dps, loss, WEIGHTED, w, w_index, bin_w))
    return rc;
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

// (loss_rows.h) the weighted entries under the name of dosx_loss_rows_fn / _fn_f64, for their calls without a table
template <typename T>
int dosx_loss_rows_weighted_as(const char* who, const T* pg, const T* ps, const T* y, int B, int S, int B_global, int kind,
                               int clamp_target, T beta, T delta, T* dpg, T* dps, T* per_crystal, T* loss, const T* w,
                               const int32_t* w_index, const T* bin_w, dosx_stream_t stream) {
  return loss_rows<T, true>(who, pg, ps, y, B, S, B_global, kind, clamp_target, beta, delta, dpg, dps, per_crystal, loss, w,
                            w_index, bin_w, stream);
}
template int dosx_loss_rows_weighted_as<float>(const char*, const float*, const float*, const float*, int, int, int, int, int,
                                               float, float, float*, float*, float*, float*, const float*, const int32_t*,
                                               const float*, dosx_stream_t);
template int dosx_loss_rows_weighted_as<double>(const char*, const double*, const double*, const double*, int, int, int, int, int,
                                                double, double, double*, double*, double*, double*, const double*, const int32_t*,
                                                const double*, dosx_stream_t);

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
