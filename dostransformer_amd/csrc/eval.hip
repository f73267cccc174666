// Per-crystal evaluation metrics (evaluate.test_per_crystal): what utils.test / utils.test_phonon compute for one batch, taken
// over every row of a [B,S] batch on its own - the reference's numbers at batch_size = 1 (include/dosx.h "evaluation metrics").
// Plain IEEE double arithmetic (no fast-math in this build: sqrt() and / are correctly rounded); every sum has a fixed order that
// depends on S alone, so a row's four numbers are bitwise the same wherever the row stands in whatever launch.
#include "common.h"

namespace {

constexpr int EVAL_WAVES = 4;      // crystals per workgroup, one wavefront each (as loss_edos_kernel)

// Wave64 all-reduce of a double by an xor butterfly: after step k every lane holds the sum of its 2^k-lane group, and both
// partners of an exchange add the same two numbers (a + b == b + a bitwise), so all 64 lanes end with the same total.
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

template <typename T>
__device__ __forceinline__ T clamp0_of(T v, bool clamp) {
  return (clamp && v < (T)0) ? (T)0 : v;       // torch.clamp(v, min=0): a NaN stays a NaN
}

// Lane l of the row's wave takes the elements l, l + 64, ... in order; the 64 lane sums meet in wave_sum_f64.  The second pass
// (sum of (y - mean)^2, after the mean is known) reads the row's targets again - 51 or 201 numbers, still in cache.
template <typename T>
__global__ __launch_bounds__(64 * EVAL_WAVES) void eval_metrics_kernel(const T* pred, const T* y, int B, int S, int clamp0,
                                                                       double* metrics, T* pred_out, T* y_out) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * EVAL_WAVES + (threadIdx.x >> 6);
  if (b >= B) return;
  const size_t o = (size_t)b * S;
  const bool clamp = clamp0 != 0;
  double sse = 0.0, sae = 0.0, sy = 0.0;
  for (int s = lane; s < S; s += 64) {
    const T p = clamp0_of(pred[o + s], clamp), t = clamp0_of(y[o + s], clamp);
    if (pred_out) pred_out[o + s] = p;
    if (y_out) y_out[o + s] = t;
    const double d = (double)t - (double)p;
    sse += d * d;
    sae += fabs(d);
    sy += (double)t;
  }
  sse = wave_sum_f64(sse);
  sae = wave_sum_f64(sae);
  sy = wave_sum_f64(sy);
  const double mean = sy / (double)S;
  double sst = 0.0;
  for (int s = lane; s < S; s += 64) {
    const double c = (double)clamp0_of(y[o + s], clamp) - mean;
    sst += c * c;
  }
  sst = wave_sum_f64(sst);
  if (lane == 0) {
    const double mse = sse / (double)S;
    double* m = metrics + (size_t)b * 4;
    m[0] = sqrt(mse);
    m[1] = mse;
    m[2] = sae / (double)S;
    m[3] = 1.0 - sse / sst;
  }
}

template <typename T>
int eval_metrics(const char* who, const T* pred, const T* y, int B, int S, int clamp0, double* metrics, T* pred_out, T* y_out,
                 dosx_stream_t stream) {
  DOSX_CHECK_ARG(B >= 0 && S >= 1, "%s: B=%d S=%d (B >= 0 and S >= 1)", who, B, S);
  if (B == 0) return 0;
  DOSX_CHECK_ARG(pred && y && metrics, "%s: NULL operand (only pred_out / y_out may be NULL)", who);
  // (in place - pred_out == pred, y_out == y - is fine: the clamp is idempotent; crossed, the second pass would read predictions)
  DOSX_CHECK_ARG(!(pred_out && (const T*)pred_out == y) && !(y_out && (const T*)y_out == pred),
                 "%s: pred_out is the target buffer or y_out the prediction buffer", who);
  hipLaunchKernelGGL(eval_metrics_kernel<T>, dim3(ceil_div(B, EVAL_WAVES)), dim3(64 * EVAL_WAVES), 0, to_stream(stream), pred, y,
                     B, S, clamp0, metrics, pred_out, y_out);
  DOSX_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int dosx_eval_metrics(const float* pred, const float* y, int B, int S, int clamp0, double* metrics, float* pred_out,
                                 float* y_out, dosx_stream_t stream) {
  return eval_metrics<float>("dosx_eval_metrics", pred, y, B, S, clamp0, metrics, pred_out, y_out, stream);
}

extern "C" int dosx_eval_metrics_f64(const double* pred, const double* y, int B, int S, int clamp0, double* metrics,
                                     double* pred_out, double* y_out, dosx_stream_t stream) {
  return eval_metrics<double>("dosx_eval_metrics_f64", pred, y, B, S, clamp0, metrics, pred_out, y_out, stream);
}
