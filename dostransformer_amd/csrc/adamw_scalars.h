// The bias-correction scalars of AdamW, defined once for the host (the launcher of adamw.hip, dosx_grad_guard_*) and the device
// (grad_guard_kernel after a skipped step, the grouped guarded kernels when the record's t is not the caller's step): every
// mode of the optimizer step promises the bits of the plain one, so every place that needs a scalar calls these.
// T = float: dosx_adamw's roundings (the powers and quotients in double, the result rounded once); T = double: torch's.
// adamw_ema_decay, the decay schedule of the weight average (DosxAdamWEma), lives here under the same rule: the launcher
// evaluates it for the caller's step, a guarded EMA kernel for the record's t when that is another one.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include <type_traits>

// lr / (1 - beta1^t)
template <typename T>
__host__ __device__ inline T adamw_step_size(T lr, T beta1, int t) {
  const double bc1 = 1.0 - pow((double)beta1, (double)t);
  return (T)((double)lr / bc1);
}

// what sqrt(v) meets: fp32 multiplies by 1 / sqrt(1 - beta2^t), float64 divides by sqrt(1 - beta2^t) (torch's order)
template <typename T>
__host__ __device__ inline T adamw_bc2_scale(T beta2, int t) {
  const double bc2 = 1.0 - pow((double)beta2, (double)t);
  if constexpr (std::is_same<T, float>::value) return (float)(1.0 / sqrt(bc2));
  else return sqrt(bc2);
}

// 1 - lr wd, in T
template <typename T>
__host__ __device__ inline T adamw_decay(T lr, T weight_decay) { return (T)1 - lr * weight_decay; }

// the decay of the weight average (DosxAdamWEma) at t = AdamW's time - t0 steps of averaging: min(decay, (1 + t) / (10 + t)) under
// warm-up (torch-ema's / timm's schedule), else decay; in double, rounded once to T
template <typename T>
__host__ __device__ inline T adamw_ema_decay(double decay, int warmup, int t) {
  double d = decay;
  if (warmup) {
    const double w = (1.0 + (double)t) / (10.0 + (double)t);
    if (w < d) d = w;
  }
  return (T)d;
}
