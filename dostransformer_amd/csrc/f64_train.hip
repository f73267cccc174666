// Tail of the float64 training step of DOSTransformer_phonon (train64.Trainer64): the phonon loss with its gradient and the
// flat AdamW update, both on double operands (include/dosx.h "float64 training step").  Plain IEEE double arithmetic: the
// build has no fast-math, sqrt() and / are correctly rounded; every reduction has a fixed order, so two runs are bitwise equal.
#include "common.h"

namespace {

constexpr int LOSS64_THREADS = 1024;
constexpr int ADAMW64_THREADS = 256;
constexpr int ADAMW64_MAX_WGS = 2048;     // 8 workgroups of 4 waves on each of the 256 CUs; larger buffers go round the grid

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

// torch's single-tensor AdamW on one element, in its operation order (torch/optim/adamw.py, _single_tensor_adamw):
//   p.mul_(1 - lr wd); m.lerp_(g, 1 - b1); v.mul_(b2).addcmul_(g, g, value = 1 - b2);
//   denom = (v.sqrt() / sqrt(bc2)).add_(eps); p.addcdiv_(m, denom, value = -lr / bc1)
// decay = 1 - lr wd, omb1 = 1 - b1, omb2 = 1 - b2, bc2_sqrt = sqrt(bc2), step_size = lr / bc1: doubles from the host.
__device__ __forceinline__ void adamw64_one(double& p, double g, double& m, double& v, double decay, double omb1, double b2,
                                            double omb2, double eps, double step_size, double bc2_sqrt) {
  const double pd = p * decay;
  m = m + (g - m) * omb1;
  v = v * b2 + omb2 * g * g;
  const double denom = sqrt(v) / bc2_sqrt + eps;
  p = pd - step_size * (m / denom);
}

// 56 B per parameter (reads p g m v, writes p m v): HBM-bound.  16-byte accesses (double2: one global_load / store_dwordx4 per
// lane, a wave moves 1 KiB per instruction), grid-stride over the pairs; an odd last element goes to thread 0 of the grid.
__global__ __launch_bounds__(ADAMW64_THREADS) void adamw_f64_kernel(double* __restrict__ p, const double* __restrict__ g,
                                                                    double* __restrict__ m, double* __restrict__ v, size_t n,
                                                                    double decay, double omb1, double b2, double omb2, double eps,
                                                                    double step_size, double bc2_sqrt) {
  const size_t n2 = n >> 1;
  double2* p2 = reinterpret_cast<double2*>(p);
  const double2* g2 = reinterpret_cast<const double2*>(g);
  double2* m2 = reinterpret_cast<double2*>(m);
  double2* v2 = reinterpret_cast<double2*>(v);
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (size_t i = tid; i < n2; i += (size_t)gridDim.x * blockDim.x) {
    double2 pp = p2[i], mm = m2[i], vv = v2[i];
    const double2 gg = g2[i];
    adamw64_one(pp.x, gg.x, mm.x, vv.x, decay, omb1, b2, omb2, eps, step_size, bc2_sqrt);
    adamw64_one(pp.y, gg.y, mm.y, vv.y, decay, omb1, b2, omb2, eps, step_size, bc2_sqrt);
    p2[i] = pp; m2[i] = mm; v2[i] = vv;
  }
  if (tid == 0 && (n & 1)) {
    const size_t i = n - 1;
    double pj = p[i], mj = m[i], vj = v[i];
    adamw64_one(pj, g[i], mj, vj, decay, omb1, b2, omb2, eps, step_size, bc2_sqrt);
    p[i] = pj; m[i] = mj; v[i] = vj;
  }
}

// adamw_f64_kernel behind a gradient guard (include/dosx.h: DosxStepGuard): adamw64_one on g * clip (clip = 1.0: g itself, bit
// for bit), the verdict of dosx_grad_guard_f64 read from device memory by every thread (plain uniform loads of a record no one
// writes during this launch); skip != 0 returns before any store.
__global__ __launch_bounds__(ADAMW64_THREADS) void adamw_guarded_f64_kernel(double* __restrict__ p, const double* __restrict__ g,
                                                                            double* __restrict__ m, double* __restrict__ v, size_t n,
                                                                            double decay, double omb1, double b2, double omb2,
                                                                            double eps, const DosxStepGuard* __restrict__ rec) {
  if (rec->skip != 0) return;
  const double clip = rec->clip, step_size = rec->step_size, bc2_sqrt = rec->bc2_scale;
  const size_t n2 = n >> 1;
  double2* p2 = reinterpret_cast<double2*>(p);
  const double2* g2 = reinterpret_cast<const double2*>(g);
  double2* m2 = reinterpret_cast<double2*>(m);
  double2* v2 = reinterpret_cast<double2*>(v);
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (size_t i = tid; i < n2; i += (size_t)gridDim.x * blockDim.x) {
    double2 pp = p2[i], mm = m2[i], vv = v2[i];
    const double2 gg = g2[i];
    adamw64_one(pp.x, gg.x * clip, mm.x, vv.x, decay, omb1, b2, omb2, eps, step_size, bc2_sqrt);
    adamw64_one(pp.y, gg.y * clip, mm.y, vv.y, decay, omb1, b2, omb2, eps, step_size, bc2_sqrt);
    p2[i] = pp; m2[i] = mm; v2[i] = vv;
  }
  if (tid == 0 && (n & 1)) {
    const size_t i = n - 1;
    double pj = p[i], mj = m[i], vj = v[i];
    adamw64_one(pj, g[i] * clip, mj, vj, decay, omb1, b2, omb2, eps, step_size, bc2_sqrt);
    p[i] = pj; m[i] = mj; v[i] = vj;
  }
}

// adamw_f64_kernel / adamw_guarded_f64_kernel with parameter groups (include/dosx.h: DosxAdamWGroups): adamw64_one with decay and
// step_size looked up per 64-element chunk.  The table arrives by value and is only ever indexed by constants: the first
// DOSX_ADAMW_MAX_GROUPS lanes of a workgroup stage one {decay, step_size} pair each into LDS, once, behind one barrier (a double2
// never straddles a chunk: 32 neighbouring lanes share the byte and the pair).  GUARDED: skip / clip / bc2_scale from the record;
// rec->t == step: the host's step_size_k, else lr_k / (1 - beta1^t) by grad_guard_kernel's expression.
struct AdamW64GroupTable {
  double decay[DOSX_ADAMW_MAX_GROUPS], step_size[DOSX_ADAMW_MAX_GROUPS], lr[DOSX_ADAMW_MAX_GROUPS];
  int n_groups;
};

template <bool GUARDED>
__global__ __launch_bounds__(ADAMW64_THREADS) void adamw_grouped_f64_kernel(double* __restrict__ p, const double* __restrict__ g,
                                                                            double* __restrict__ m, double* __restrict__ v, size_t n,
                                                                            const uint8_t* __restrict__ chunk_group,
                                                                            const AdamW64GroupTable tab, double beta1, double omb1,
                                                                            double b2, double omb2, double eps, double bc2_sqrt,
                                                                            int step, const DosxStepGuard* __restrict__ rec) {
  __shared__ double2 s_tab[DOSX_ADAMW_MAX_GROUPS];
  bool host_step = true;
  int t = step;
  double clip = 1.0;
  if constexpr (GUARDED) {
    if (rec->skip != 0) return;
    clip = rec->clip;
    bc2_sqrt = rec->bc2_scale;
    t = rec->t;
    host_step = t == step || t < 1;
  }
  const int lane = (int)threadIdx.x;
  if (lane < DOSX_ADAMW_MAX_GROUPS) {
    double d = 0.0, s = 0.0, lr = 0.0;
#pragma unroll
    for (int k = 0; k < DOSX_ADAMW_MAX_GROUPS; ++k)
      if (lane == k) { d = tab.decay[k]; s = tab.step_size[k]; lr = tab.lr[k]; }
    if constexpr (GUARDED) {
      if (!host_step) {
        const double bc1 = 1.0 - pow(beta1, (double)t);
        s = lr / bc1;
      }
    }
    s_tab[lane] = make_double2(d, s);
  }
  __syncthreads();
  const unsigned n_groups = (unsigned)tab.n_groups;
  const size_t n2 = n >> 1;
  double2* p2 = reinterpret_cast<double2*>(p);
  const double2* g2 = reinterpret_cast<const double2*>(g);
  double2* m2 = reinterpret_cast<double2*>(m);
  double2* v2 = reinterpret_cast<double2*>(v);
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (size_t i = tid; i < n2; i += (size_t)gridDim.x * blockDim.x) {
    unsigned k = chunk_group[i >> 5];                    // 32 double2 per 64-element chunk
    if (k >= n_groups) k = 0;
    const double2 ds = s_tab[k];
    double2 pp = p2[i], mm = m2[i], vv = v2[i];
    const double2 gg = g2[i];
    if constexpr (GUARDED) {
      adamw64_one(pp.x, gg.x * clip, mm.x, vv.x, ds.x, omb1, b2, omb2, eps, ds.y, bc2_sqrt);
      adamw64_one(pp.y, gg.y * clip, mm.y, vv.y, ds.x, omb1, b2, omb2, eps, ds.y, bc2_sqrt);
    } else {
      adamw64_one(pp.x, gg.x, mm.x, vv.x, ds.x, omb1, b2, omb2, eps, ds.y, bc2_sqrt);
      adamw64_one(pp.y, gg.y, mm.y, vv.y, ds.x, omb1, b2, omb2, eps, ds.y, bc2_sqrt);
    }
    p2[i] = pp; m2[i] = mm; v2[i] = vv;
  }
}

// the host half of both grouped float64 entries: dosx_adamw_f64's expressions, once per group
template <bool GUARDED>
int adamw_grouped_f64_launch(const char* who, double* p, const double* g, double* m, double* v, int64_t n, const void* chunk_group,
                             const DosxAdamWGroups* groups, double beta1, double beta2, double eps, int step, const void* guard,
                             dosx_stream_t stream) {
  if (int rc = dosx_adamw_grouped_check(who, p, g, m, v, n, chunk_group, groups, step, GUARDED, guard)) return rc;
  if (n == 0) return 0;
  const double bc1 = 1.0 - pow(beta1, (double)step);
  const double bc2 = 1.0 - pow(beta2, (double)step);
  AdamW64GroupTable tab = {};
  tab.n_groups = groups->n_groups;
  for (int k = 0; k < groups->n_groups; ++k) {
    const double lr = groups->lr[k], weight_decay = groups->weight_decay[k];
    tab.lr[k] = lr;
    tab.step_size[k] = lr / bc1;
    tab.decay[k] = 1.0 - lr * weight_decay;
  }
  size_t wgs = ((size_t)n / 2 + ADAMW64_THREADS - 1) / ADAMW64_THREADS;      // dosx_adamw_f64's grid
  if (wgs > (size_t)ADAMW64_MAX_WGS) wgs = ADAMW64_MAX_WGS;
  if (wgs < 1) wgs = 1;
  hipLaunchKernelGGL(adamw_grouped_f64_kernel<GUARDED>, dim3((unsigned)wgs), dim3(ADAMW64_THREADS), 0, to_stream(stream), p, g, m, v,
                     (size_t)n, static_cast<const uint8_t*>(chunk_group), tab, beta1, 1.0 - beta1, beta2, 1.0 - beta2, eps, sqrt(bc2),
                     step, static_cast<const DosxStepGuard*>(guard));
  DOSX_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int dosx_adamw_grouped_f64(double* p, const double* g, double* m, double* v, int64_t n, const void* chunk_group,
                                      const DosxAdamWGroups* groups, double beta1, double beta2, double eps, int step,
                                      dosx_stream_t stream) {
  return adamw_grouped_f64_launch<false>("dosx_adamw_grouped_f64", p, g, m, v, n, chunk_group, groups, beta1, beta2, eps, step,
                                         nullptr, stream);
}

extern "C" int dosx_adamw_grouped_guarded_f64(double* p, const double* g, double* m, double* v, int64_t n, const void* chunk_group,
                                              const DosxAdamWGroups* groups, double beta1, double beta2, double eps, int step,
                                              const void* guard, dosx_stream_t stream) {
  return adamw_grouped_f64_launch<true>("dosx_adamw_grouped_guarded_f64", p, g, m, v, n, chunk_group, groups, beta1, beta2, eps, step,
                                        guard, stream);
}

extern "C" int dosx_loss_phonon_f64(const double* pg, const double* ps, const double* y, double beta, double* dpg, double* dps,
                                    double* loss, double* sse, int count, dosx_stream_t stream) {
  DOSX_CHECK_ARG(pg && ps && y && dpg && dps && loss, "dosx_loss_phonon_f64: NULL operand (only sse may be NULL)");
  DOSX_CHECK_ARG(count > 0, "dosx_loss_phonon_f64: count must be positive, got %d", count);
  hipLaunchKernelGGL(loss_phonon_f64_kernel, dim3(1), dim3(LOSS64_THREADS), 0, to_stream(stream), pg, ps, y, beta, dpg, dps,
                     loss, sse, count);
  DOSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int dosx_adamw_f64(double* p, const double* g, double* m, double* v, int64_t n, double lr, double beta1, double beta2,
                              double eps, double weight_decay, int step, dosx_stream_t stream) {
  DOSX_CHECK_ARG(p && g && m && v, "dosx_adamw_f64: NULL buffer");
  DOSX_CHECK_ARG(n >= 0, "dosx_adamw_f64: n must not be negative, got %lld", (long long)n);
  DOSX_CHECK_ARG(step >= 1, "dosx_adamw_f64: step is the 1-based step count, got %d", step);
  DOSX_CHECK_ARG(((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                   reinterpret_cast<uintptr_t>(v)) & 15) == 0, "dosx_adamw_f64: buffers must be 16-byte aligned");
  if (n == 0) return 0;
  const double bc1 = 1.0 - pow(beta1, (double)step);
  const double bc2 = 1.0 - pow(beta2, (double)step);
  size_t wgs = ((size_t)n / 2 + ADAMW64_THREADS - 1) / ADAMW64_THREADS;
  if (wgs > (size_t)ADAMW64_MAX_WGS) wgs = ADAMW64_MAX_WGS;
  if (wgs < 1) wgs = 1;
  hipLaunchKernelGGL(adamw_f64_kernel, dim3((unsigned)wgs), dim3(ADAMW64_THREADS), 0, to_stream(stream), p, g, m, v, (size_t)n,
                     1.0 - lr * weight_decay, 1.0 - beta1, beta2, 1.0 - beta2, eps, lr / bc1, sqrt(bc2));
  DOSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int dosx_adamw_guarded_f64(double* p, const double* g, double* m, double* v, int64_t n, double lr, double beta1,
                                      double beta2, double eps, double weight_decay, const void* guard, dosx_stream_t stream) {
  DOSX_CHECK_ARG(p && g && m && v && guard, "dosx_adamw_guarded_f64: NULL buffer or record");
  DOSX_CHECK_ARG(n >= 0, "dosx_adamw_guarded_f64: n must not be negative, got %lld", (long long)n);
  DOSX_CHECK_ARG(((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                   reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(guard)) & 15) == 0,
                 "dosx_adamw_guarded_f64: buffers must be 16-byte aligned");
  if (n == 0) return 0;
  size_t wgs = ((size_t)n / 2 + ADAMW64_THREADS - 1) / ADAMW64_THREADS;      // dosx_adamw_f64's grid
  if (wgs > (size_t)ADAMW64_MAX_WGS) wgs = ADAMW64_MAX_WGS;
  if (wgs < 1) wgs = 1;
  hipLaunchKernelGGL(adamw_guarded_f64_kernel, dim3((unsigned)wgs), dim3(ADAMW64_THREADS), 0, to_stream(stream), p, g, m, v,
                     (size_t)n, 1.0 - lr * weight_decay, 1.0 - beta1, beta2, 1.0 - beta2, eps, static_cast<const DosxStepGuard*>(guard));
  DOSX_LAUNCH_CHECK();
  return 0;
}
