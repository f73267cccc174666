// Tail of the float64 training step of DOSTransformer_phonon (train64.Trainer64): the phonon loss with its gradient on double
// operands (include/dosx.h "float64 training step"; the flat AdamW update behind it is csrc/adamw.hip).  Plain IEEE double
// arithmetic: the build has no fast-math, sqrt() and / are correctly rounded; every reduction has a fixed order, so two runs are
// bitwise equal.
#include "common.h"

namespace {

constexpr int LOSS64_THREADS = 1024;

// loss = sqrt(sse_g / count) + beta sqrt(sse_s / count), dpg = (pg - y) / (count rmse_g), dps = beta (ps - y) / (count rmse_s).
// One workgroup (the gradient needs both sums first; count = B * S is a few thousand): lane t adds its elements t, t + 1024, ...
// in order, then a binary tree over the 1024 lane sums in shared memory - the same order on every run.
// An RMSE of exactly 0 (prediction == target everywhere) has no gradient direction: that branch's gradient is written as 0
// (never 0 / 0 = NaN) and it adds 0 to the loss.  A NaN / Inf operand still reaches the loss and the gradients.
__global__ __launch_bounds__(LOSS64_THREADS) void loss_phonon_f64_kernel(const double* __restrict__ pg, const double* __restrict__ ps,
                                                                         const double* __restrict__ y, double beta,
                                                                         double* __restrict__ dpg, double* __restrict__ dps,
                                                                         double* __restrict__ loss, double* __restrict__ sse,
                                                                         int count) {
  __shared__ double red[2][LOSS64_THREADS];
  const int t = threadIdx.x;
  double a = 0.0, b = 0.0;
  for (int i = t; i < count; i += LOSS64_THREADS) {
    const double yi = y[i], d0 = pg[i] - yi, d1 = ps[i] - yi;
    a += d0 * d0;
    b += d1 * d1;
  }
  red[0][t] = a;
  red[1][t] = b;
  __syncthreads();
  for (int s = LOSS64_THREADS / 2; s > 0; s >>= 1) {
    if (t < s) {
      red[0][t] += red[0][t + s];
      red[1][t] += red[1][t + s];
    }
    __syncthreads();
  }
  const double s0 = red[0][0], s1 = red[1][0];
  const double r0 = sqrt(s0 / (double)count), r1 = sqrt(s1 / (double)count);
  const double den0 = (double)count * r0, den1 = (double)count * r1;
  if (t == 0) {
    loss[0] = r0 + beta * r1;
    if (sse) { sse[0] = s0; sse[1] = s1; }
  }
  for (int i = t; i < count; i += LOSS64_THREADS) {
    const double yi = y[i];
    dpg[i] = r0 == 0.0 ? 0.0 : (pg[i] - yi) / den0;
    dps[i] = r1 == 0.0 ? 0.0 : beta * (ps[i] - yi) / den1;
  }
}

}  // namespace

extern "C" int dosx_loss_phonon_f64(const double* pg, const double* ps, const double* y, double beta, double* dpg, double* dps,
                                    double* loss, double* sse, int count, dosx_stream_t stream) {
  DOSX_CHECK_ARG(pg && ps && y && dpg && dps && loss, "dosx_loss_phonon_f64: NULL operand (only sse may be NULL)");
  DOSX_CHECK_ARG(count > 0, "dosx_loss_phonon_f64: count must be positive, got %d", count);
  hipLaunchKernelGGL(loss_phonon_f64_kernel, dim3(1), dim3(LOSS64_THREADS), 0, to_stream(stream), pg, ps, y, beta, dpg, dps,
                     loss, sse, count);
  DOSX_LAUNCH_CHECK();
  return 0;
}
