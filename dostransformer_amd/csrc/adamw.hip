// AdamW on the flat buffers: the eight entries of include/dosx.h - dosx_adamw, _f64, _guarded*, _grouped*, _grouped_guarded* -
// and the two that also keep an exponential moving average of the parameters (dosx_adamw_ema, _f64: the EMA instantiations)
// are one kernel template and one host launcher.  Guarded without a trip == unguarded, grouped == ungrouped run by run, and a
// resumed guarded run == the unguarded one hold bit for bit because each precision's element update is written once (adamw_one)
// and every bias-correction scalar comes from adamw_scalars.h.
// 28 B (fp32) / 56 B (float64) per parameter - reads p g m v, writes p m v: HBM-bound.  16-byte accesses (float4 / double2),
// grid-stride over the vectors.  No fast-math in the build: sqrt and / are correctly rounded.
// EMA: + 8 B / 16 B per parameter (reads and writes ema): 36 B / 72 B.  dosx_swap_buffers, at the end of the file, is what puts
// such an average in the parameters' place and back.
#include "common.h"
#include "adamw_scalars.h"

#include <type_traits>

namespace {

constexpr int ADAMW_THREADS = 256;
// the grid's cap, larger buffers go round it: fp32 4096 workgroups (4096 x 256 x 4 floats a sweep); float64 2048 - 8 workgroups
// of 4 waves on each of the 256 CUs
template <typename T>
constexpr int ADAMW_MAX_WGS = sizeof(T) == 4 ? 4096 : 2048;
static_assert(sizeof(((DosxAdamWGroups*)0)->lr) / sizeof(double) == DOSX_ADAMW_MAX_GROUPS, "DosxAdamWGroups holds DOSX_ADAMW_MAX_GROUPS");

// What a launch reads besides p, g, m, v and n.  NG = 1: the ungrouped launch - one decay, one step size, no chunk map (the
// pointer and n_groups are not read); NG = DOSX_ADAMW_MAX_GROUPS: the table of a grouped launch, by value and only ever indexed
// by constants.  omb_k = 1 - beta_k, rounded in T on the host.  lr, beta1, step: for the grouped guarded forms alone.
// EMA: the buffer of the average, 1 - d_t rounded in T on the host, and what d_t is recomputed from on the device when the
// record's t is not the caller's step (adamw_scalars.h: adamw_ema_decay).  An empty base without EMA: AdamWArgs<T, NG, false> is
// laid out as it always was.
template <typename T, bool EMA>
struct AdamWEmaArgs {};
template <typename T>
struct AdamWEmaArgs<T, true> {
  T* ema;
  double ema_decay;
  int ema_warmup, ema_t0;
  T omd;
};

template <typename T, int NG, bool EMA>
struct AdamWArgs : AdamWEmaArgs<T, EMA> {
  T omb1, beta2, omb2, eps;
  T bc2_scale, gscale;                    // unguarded; a guarded launch takes them from the record (clip stands for gscale)
  T decay[NG], step_size[NG], lr[NG];
  T beta1;
  int step, n_groups;
  const uint8_t* chunk_group;
  const DosxStepGuard* rec;
};

// fp32, one element: g * gscale always, sqrt(v) TIMES inv_bc2s = (float)(1 / sqrt(bc2)).  The fmas are written out and nothing
// else may contract (the pragma): they are the contraction the fp32 kernels have always been compiled to, no longer left to the
// compiler - (g gscale - m), m + d omb1 and sqrt(v') inv_bc2s + eps with one rounding each everywhere; v' and p' with one rounding
// in the vector body (FUSED) but with their products rounded first in the scalar tail, where the compiler had packed the two
// products of each into one v_pk_mul: an element's bits depend on which of the two paths it takes, as they always did.
template <bool GUARDED, bool FUSED>
__device__ __forceinline__ void adamw_one(float& p, float g, float& m, float& v, float decay, float omb1, float beta2, float omb2,
                                          float eps, float step_size, float inv_bc2s, float gscale) {
#pragma clang fp contract(off)
  const float gr = g * gscale;
  m = fmaf(fmaf(g, gscale, -m), omb1, m);
  v = FUSED ? fmaf(omb2 * gr, gr, v * beta2) : v * beta2 + omb2 * gr * gr;
  const float step = -step_size * (m / fmaf(sqrtf(v), inv_bc2s, eps));      // (the sign on the uniform factor: exact, and free)
  p = FUSED ? fmaf(p, decay, step) : p * decay + step;
}

// float64, one element: torch's single-tensor AdamW in its operation order (torch/optim/adamw.py, _single_tensor_adamw):
//   p.mul_(1 - lr wd); m.lerp_(g, 1 - b1); v.mul_(b2).addcmul_(g, g, value = 1 - b2);
//   denom = (v.sqrt() / sqrt(bc2)).add_(eps); p.addcdiv_(m, denom, value = -lr / bc1)
// sqrt(v) DIVIDED by bc2_sqrt = sqrt(bc2); g * clip in the guarded instantiations only (clip = 1.0: g itself, bit for bit).
// The fmas are written out - m + (g - m) omb1, v b2 + (omb2 g) g and p decay - step_size (m / denom) with ONE rounding each, and
// g clip - m likewise: the contraction every float64 kernel has always been compiled to, vector body and tail alike, no longer
// left to the compiler (which, given v b2 + omb2 g g, fuses one product or the other as its operand order falls).
template <bool GUARDED, bool FUSED>
__device__ __forceinline__ void adamw_one(double& p, double g, double& m, double& v, double decay, double omb1, double beta2,
                                          double omb2, double eps, double step_size, double bc2_sqrt, double clip) {
  double d = g - m;
  if constexpr (GUARDED) {
    d = fma(g, clip, -m);
    g = g * clip;
  }
  m = fma(d, omb1, m);
  v = fma(v, beta2, omb2 * g * g);
  const double denom = sqrt(v) / bc2_sqrt + eps;
  p = fma(p, decay, -(step_size * (m / denom)));
}

// The average of the parameters, one element: e + (p' - e) omd - adamw_one's first-moment update read with g := p', m := e,
// omb1 := omd, gscale = 1 (float64: its unguarded form), one rounding of the difference and one of the fma, vector body and tail
// alike.
__device__ __forceinline__ float ema_one(float e, float p, float omd) {
#pragma clang fp contract(off)
  return fmaf(fmaf(p, 1.f, -e), omd, e);
}

__device__ __forceinline__ double ema_one(double e, double p, double omd) {
#pragma clang fp contract(off)
  const double d = p - e;
  return fma(d, omd, e);
}

// (the fp32 ungrouped kernels never carried a launch bound: 1024 is what a kernel without one gets)
template <typename T, bool GROUPED>
constexpr int adamw_bound = std::is_same<T, float>::value && !GROUPED ? 1024 : ADAMW_THREADS;

// GUARDED (include/dosx.h: DosxStepGuard): the verdict of dosx_grad_guard_* read from device memory by every thread (plain
// uniform loads of a record no one writes during this launch) - skip != 0 returns before any store (and before the barrier, for
// every thread alike), clip, bc2_scale and - ungrouped - step_size are the record's.
// GROUPED (DosxAdamWGroups): decay and step_size per 64-element chunk.  The first DOSX_ADAMW_MAX_GROUPS lanes of a workgroup
// stage one {decay, step_size} pair each into LDS, once, behind one barrier; the loop reads the pair of its chunk's group from
// there (a vector never straddles a chunk; a byte >= n_groups is stepped as group 0).  The record holds ONE step size, so a
// guarded grouped launch uses the host's step_size_k when rec->t == step, else lr_k / (1 - beta1^t) by adamw_step_size.
// The scalar tail (n not a multiple of the vector) exists only ungrouped: thread tid of the grid takes element t0 + tid - up to
// three floats, or the one odd double (thread 0).
// EMA (DosxAdamWEma): the thread that has p' in registers also reads ema, writes ema' = ema_one(ema, p', 1 - d_t) with the same
// 16-byte access (the tail: the same element) and touches nothing else; p', m', v' are those of the launch without EMA.  d_t is
// the host's for AdamW's time `step`; a guarded launch whose record says another time (steps were skipped) recomputes it for
// that time, every thread alike.  The skip return stands in front of the ema store too.
template <typename T, bool GUARDED, bool GROUPED, bool EMA>
__global__ __launch_bounds__((adamw_bound<T, GROUPED>)) void adamw_kernel(
    T* __restrict__ p, const T* __restrict__ g, T* __restrict__ m, T* __restrict__ v, const size_t n,
    const AdamWArgs<T, GROUPED ? DOSX_ADAMW_MAX_GROUPS : 1, EMA> a) {
  using Vec = typename std::conditional<sizeof(T) == 4, float4, double2>::type;
  using Pair = typename std::conditional<sizeof(T) == 4, float2, double2>::type;
  constexpr int PER = 16 / (int)sizeof(T);
  __shared__ Pair s_tab[DOSX_ADAMW_MAX_GROUPS];           // (referenced by the grouped instantiations alone: no LDS otherwise)
  T gscale = a.gscale, bc2_scale = a.bc2_scale, decay = a.decay[0], step_size = a.step_size[0];
  int t = a.step;
  if constexpr (GUARDED) {
    if (a.rec->skip != 0) return;
    gscale = (T)a.rec->clip;
    bc2_scale = (T)a.rec->bc2_scale;
    step_size = (T)a.rec->step_size;
    t = a.rec->t;
  }
  T* __restrict__ ema = nullptr;
  T omd = 0;
  if constexpr (EMA) {
    ema = a.ema;
    omd = a.omd;
    if constexpr (GUARDED) {
      if (t != a.step) omd = (T)1 - adamw_ema_decay<T>(a.ema_decay, a.ema_warmup, t > a.ema_t0 ? t - a.ema_t0 : 1);
    }
  }
  if constexpr (GROUPED) {
    const int lane = (int)threadIdx.x;
    if (lane < DOSX_ADAMW_MAX_GROUPS) {
      T d = 0, s = 0, lr = 0;
#pragma unroll
      for (int k = 0; k < DOSX_ADAMW_MAX_GROUPS; ++k)
        if (lane == k) { d = a.decay[k]; s = a.step_size[k]; lr = a.lr[k]; }
      if constexpr (GUARDED) {
        if (t != a.step && t >= 1) s = adamw_step_size<T>(lr, a.beta1, t);
      }
      s_tab[lane] = Pair{d, s};
    }
    __syncthreads();
  }
  const size_t nvec = n / PER;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (size_t i = tid; i < nvec; i += (size_t)gridDim.x * blockDim.x) {
    if constexpr (GROUPED) {
      unsigned k = a.chunk_group[i / (DOSX_ADAMW_GROUP_CHUNK / PER)];
      if (k >= (unsigned)a.n_groups) k = 0;
      const Pair ds = s_tab[k];
      decay = ds.x; step_size = ds.y;
    }
    Vec pp = reinterpret_cast<Vec*>(p)[i], mm = reinterpret_cast<Vec*>(m)[i], vv = reinterpret_cast<Vec*>(v)[i];
    const Vec gg = reinterpret_cast<const Vec*>(g)[i];
    Vec ee = {};
    if constexpr (EMA) ee = reinterpret_cast<Vec*>(ema)[i];
    T* P = &pp.x; const T* G = &gg.x; T* M = &mm.x; T* V = &vv.x;
#pragma unroll
    for (int j = 0; j < PER; ++j)
      adamw_one<GUARDED, true>(P[j], G[j], M[j], V[j], decay, a.omb1, a.beta2, a.omb2, a.eps, step_size, bc2_scale, gscale);
    reinterpret_cast<Vec*>(p)[i] = pp; reinterpret_cast<Vec*>(m)[i] = mm; reinterpret_cast<Vec*>(v)[i] = vv;
    if constexpr (EMA) {
      T* E = &ee.x;
#pragma unroll
      for (int j = 0; j < PER; ++j) E[j] = ema_one(E[j], P[j], omd);
      reinterpret_cast<Vec*>(ema)[i] = ee;
    }
  }
  if constexpr (!GROUPED) {
    const size_t t0 = nvec * PER;
    if (tid < n - t0) {
      const size_t i = t0 + tid;
      T pj = p[i], mj = m[i], vj = v[i];
      adamw_one<GUARDED, false>(pj, g[i], mj, vj, decay, a.omb1, a.beta2, a.omb2, a.eps, step_size, bc2_scale, gscale);
      p[i] = pj; m[i] = mj; v[i] = vj;
      if constexpr (EMA) ema[i] = ema_one(ema[i], pj, omd);
    }
  }
}

// The host half of all ten entries: refusals (include/dosx.h states them per entry), scalars, grid, launch.  The ungrouped
// entries arrive as one group of their (lr, weight_decay) - a float survives the trip through DosxAdamWGroups' doubles - and the
// guarded ungrouped ones with step = 1: their kernel reads neither the step nor the host's bias corrections.  The EMA entries
// (e: their descriptor, else NULL) pass the caller's step to every form: the average's warm-up counts from it.
template <typename T, bool GUARDED, bool GROUPED, bool EMA = false>
int adamw_launch(const char* who, T* p, const T* g, T* m, T* v, int64_t n, const void* chunk_group, const DosxAdamWGroups* groups,
                 T beta1, T beta2, T eps, int step, T grad_scale, const void* guard, dosx_stream_t stream,
                 const DosxAdamWEma* e = nullptr) {
  if constexpr (std::is_same<T, float>::value && !GUARDED && !GROUPED && !EMA) {      // dosx_adamw: the oldest entry keeps its own wording
    if (n <= 0) return 0;
    DOSX_CHECK_ARG(p && g && m && v && step >= 1, "%s: bad args", who);
  } else {
    DOSX_CHECK_ARG(p && g && m && v && (!GROUPED || (chunk_group && groups)) && (!GUARDED || guard), "%s: NULL buffer%s%s", who,
                   GROUPED ? ", chunk map, groups" : "", GUARDED ? " or record" : "");
    DOSX_CHECK_ARG(n >= 0, "%s: n must not be negative, got %lld", who, (long long)n);
    DOSX_CHECK_ARG(step >= 1, "%s: step is the 1-based step count, got %d", who, step);
  }
  if constexpr (GROUPED) {
    DOSX_CHECK_ARG(n % DOSX_ADAMW_GROUP_CHUNK == 0, "%s: n must be a multiple of %d (one chunk_group byte per %d elements), got %lld",
                   who, DOSX_ADAMW_GROUP_CHUNK, DOSX_ADAMW_GROUP_CHUNK, (long long)n);
    DOSX_CHECK_ARG(groups->n_groups >= 1 && groups->n_groups <= DOSX_ADAMW_MAX_GROUPS, "%s: n_groups must be in [1, %d], got %d", who,
                   DOSX_ADAMW_MAX_GROUPS, groups->n_groups);
    for (int k = 0; k < groups->n_groups; ++k) {
      DOSX_CHECK_ARG(groups->lr[k] >= 0.0, "%s: lr[%d] must be a non-negative number, got %g", who, k, groups->lr[k]);
      DOSX_CHECK_ARG(groups->weight_decay[k] >= 0.0, "%s: weight_decay[%d] must be a non-negative number, got %g", who, k,
                     groups->weight_decay[k]);
    }
  }
  DOSX_CHECK_ARG(((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                   reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(guard)) & 15) == 0,
                 "%s: buffers must be 16-byte aligned", who);
  if constexpr (EMA) {
    DOSX_CHECK_ARG(e && e->ema, "%s: NULL ema descriptor or ema buffer", who);
    const uintptr_t ea = reinterpret_cast<uintptr_t>(e->ema), pa = reinterpret_cast<uintptr_t>(p), bytes = (uintptr_t)n * sizeof(T);
    DOSX_CHECK_ARG((ea & 15) == 0, "%s: ema must be 16-byte aligned", who);
    DOSX_CHECK_ARG(ea != pa && (ea >= pa + bytes || pa >= ea + bytes), "%s: ema must not alias p (the average is a buffer of its own)", who);
    DOSX_CHECK_ARG(e->decay >= 0.0 && e->decay < 1.0, "%s: ema decay must be in [0, 1), got %g", who, e->decay);
    DOSX_CHECK_ARG(e->t0 >= 0 && e->t0 < step, "%s: ema t0 (AdamW's time when averaging began) must be in [0, step = %d), got %d",
                   who, step, e->t0);
  }
  if (n == 0) return 0;
  AdamWArgs<T, GROUPED ? DOSX_ADAMW_MAX_GROUPS : 1, EMA> a = {};
  if constexpr (EMA) {
    a.ema = static_cast<T*>(e->ema); a.ema_decay = e->decay; a.ema_warmup = e->warmup; a.ema_t0 = e->t0;
    a.omd = (T)1 - adamw_ema_decay<T>(e->decay, e->warmup, step - e->t0);
  }
  a.omb1 = (T)1 - beta1; a.beta2 = beta2; a.omb2 = (T)1 - beta2; a.eps = eps;
  a.bc2_scale = adamw_bc2_scale<T>(beta2, step); a.gscale = grad_scale;
  for (int k = 0; k < groups->n_groups; ++k) {
    const T lr = (T)groups->lr[k];
    a.lr[k] = lr;
    a.step_size[k] = adamw_step_size<T>(lr, beta1, step);
    a.decay[k] = adamw_decay<T>(lr, (T)groups->weight_decay[k]);
  }
  a.beta1 = beta1; a.step = step; a.n_groups = groups->n_groups;
  a.chunk_group = static_cast<const uint8_t*>(chunk_group);
  a.rec = static_cast<const DosxStepGuard*>(guard);
  size_t wgs = ((size_t)n / (16 / sizeof(T)) + ADAMW_THREADS - 1) / ADAMW_THREADS;
  if (wgs > (size_t)ADAMW_MAX_WGS<T>) wgs = ADAMW_MAX_WGS<T>;
  if (wgs < 1) wgs = 1;
  hipLaunchKernelGGL((adamw_kernel<T, GUARDED, GROUPED, EMA>), dim3((unsigned)wgs), dim3(ADAMW_THREADS), 0, to_stream(stream), p, g, m, v,
                     (size_t)n, a);
  DOSX_LAUNCH_CHECK();
  return 0;
}

inline DosxAdamWGroups one_group(double lr, double weight_decay) {
  DosxAdamWGroups one = {};
  one.n_groups = 1; one.lr[0] = lr; one.weight_decay[0] = weight_decay;
  return one;
}

// The two EMA entries: which of the four forms follows from the nullable operands - chunk_group and groups (both or neither:
// grouped, lr and weight_decay are then not read) and guard (grad_scale is then not read: clip stands there).
template <typename T>
int adamw_ema_entry(const char* who, T* p, const T* g, T* m, T* v, int64_t n, T lr, T beta1, T beta2, T eps, T weight_decay, int step,
                    T grad_scale, const void* chunk_group, const DosxAdamWGroups* groups, const void* guard, const DosxAdamWEma* e,
                    dosx_stream_t stream) {
  DOSX_CHECK_ARG((chunk_group != nullptr) == (groups != nullptr), "%s: chunk map and groups go together (both, or both NULL)", who);
  const DosxAdamWGroups one = one_group(lr, weight_decay);
  if (groups && guard)
    return adamw_launch<T, true, true, true>(who, p, g, m, v, n, chunk_group, groups, beta1, beta2, eps, step, (T)1, guard, stream, e);
  if (groups)
    return adamw_launch<T, false, true, true>(who, p, g, m, v, n, chunk_group, groups, beta1, beta2, eps, step, grad_scale, nullptr, stream, e);
  if (guard)
    return adamw_launch<T, true, false, true>(who, p, g, m, v, n, nullptr, &one, beta1, beta2, eps, step, (T)1, guard, stream, e);
  return adamw_launch<T, false, false, true>(who, p, g, m, v, n, nullptr, &one, beta1, beta2, eps, step, grad_scale, nullptr, stream, e);
}

// dosx_swap_buffers: a[i] <-> b[i], one 16-byte vector per thread and trip
__global__ __launch_bounds__(DOSX_SWAP_THREADS) void swap_kernel(uint4* __restrict__ a, uint4* __restrict__ b, const size_t nvec) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (size_t)gridDim.x * blockDim.x) {
    const uint4 x = a[i], y = b[i];
    a[i] = y; b[i] = x;
  }
}

}  // namespace

extern "C" int dosx_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                          float eps, float weight_decay, int step, float grad_scale, dosx_stream_t stream) {
  const DosxAdamWGroups one = one_group(lr, weight_decay);
  return adamw_launch<float, false, false>("dosx_adamw", p, g, m, v, n, nullptr, &one, beta1, beta2, eps, step, grad_scale, nullptr, stream);
}

extern "C" int dosx_adamw_f64(double* p, const double* g, double* m, double* v, int64_t n, double lr, double beta1, double beta2,
                              double eps, double weight_decay, int step, dosx_stream_t stream) {
  const DosxAdamWGroups one = one_group(lr, weight_decay);
  return adamw_launch<double, false, false>("dosx_adamw_f64", p, g, m, v, n, nullptr, &one, beta1, beta2, eps, step, 1.0, nullptr, stream);
}

extern "C" int dosx_adamw_guarded(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                                  float eps, float weight_decay, const void* guard, dosx_stream_t stream) {
  const DosxAdamWGroups one = one_group(lr, weight_decay);
  return adamw_launch<float, true, false>("dosx_adamw_guarded", p, g, m, v, n, nullptr, &one, beta1, beta2, eps, 1, 1.f, guard, stream);
}

extern "C" int dosx_adamw_guarded_f64(double* p, const double* g, double* m, double* v, int64_t n, double lr, double beta1,
                                      double beta2, double eps, double weight_decay, const void* guard, dosx_stream_t stream) {
  const DosxAdamWGroups one = one_group(lr, weight_decay);
  return adamw_launch<double, true, false>("dosx_adamw_guarded_f64", p, g, m, v, n, nullptr, &one, beta1, beta2, eps, 1, 1.0, guard, stream);
}

extern "C" int dosx_adamw_grouped(float* p, const float* g, float* m, float* v, int64_t n, const void* chunk_group,
                                  const DosxAdamWGroups* groups, float beta1, float beta2, float eps, int step, float grad_scale,
                                  dosx_stream_t stream) {
  return adamw_launch<float, false, true>("dosx_adamw_grouped", p, g, m, v, n, chunk_group, groups, beta1, beta2, eps, step, grad_scale,
                                          nullptr, stream);
}

extern "C" int dosx_adamw_grouped_f64(double* p, const double* g, double* m, double* v, int64_t n, const void* chunk_group,
                                      const DosxAdamWGroups* groups, double beta1, double beta2, double eps, int step,
                                      dosx_stream_t stream) {
  return adamw_launch<double, false, true>("dosx_adamw_grouped_f64", p, g, m, v, n, chunk_group, groups, beta1, beta2, eps, step, 1.0,
                                           nullptr, stream);
}

extern "C" int dosx_adamw_grouped_guarded(float* p, const float* g, float* m, float* v, int64_t n, const void* chunk_group,
                                          const DosxAdamWGroups* groups, float beta1, float beta2, float eps, int step,
                                          const void* guard, dosx_stream_t stream) {
  return adamw_launch<float, true, true>("dosx_adamw_grouped_guarded", p, g, m, v, n, chunk_group, groups, beta1, beta2, eps, step, 1.f,
                                         guard, stream);
}

extern "C" int dosx_adamw_grouped_guarded_f64(double* p, const double* g, double* m, double* v, int64_t n, const void* chunk_group,
                                              const DosxAdamWGroups* groups, double beta1, double beta2, double eps, int step,
                                              const void* guard, dosx_stream_t stream) {
  return adamw_launch<double, true, true>("dosx_adamw_grouped_guarded_f64", p, g, m, v, n, chunk_group, groups, beta1, beta2, eps, step,
                                          1.0, guard, stream);
}

extern "C" int dosx_adamw_ema(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                              float weight_decay, int step, float grad_scale, const void* chunk_group, const DosxAdamWGroups* groups,
                              const void* guard, const DosxAdamWEma* ema, dosx_stream_t stream) {
  return adamw_ema_entry<float>("dosx_adamw_ema", p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, chunk_group,
                                groups, guard, ema, stream);
}

extern "C" int dosx_adamw_ema_f64(double* p, const double* g, double* m, double* v, int64_t n, double lr, double beta1, double beta2,
                                  double eps, double weight_decay, int step, const void* chunk_group, const DosxAdamWGroups* groups,
                                  const void* guard, const DosxAdamWEma* ema, dosx_stream_t stream) {
  return adamw_ema_entry<double>("dosx_adamw_ema_f64", p, g, m, v, n, lr, beta1, beta2, eps, weight_decay, step, 1.0, chunk_group,
                                 groups, guard, ema, stream);
}

extern "C" double dosx_adamw_ema_decay(double decay, int warmup, int t, int elem_bytes) {
  return elem_bytes == 4 ? (double)adamw_ema_decay<float>(decay, warmup, t) : adamw_ema_decay<double>(decay, warmup, t);
}

extern "C" int dosx_swap_buffers(void* a, void* b, int64_t bytes, dosx_stream_t stream) {
  DOSX_CHECK_ARG(a && b, "dosx_swap_buffers: NULL buffer");
  DOSX_CHECK_ARG(bytes >= 0 && bytes % 16 == 0, "dosx_swap_buffers: bytes must be a non-negative multiple of 16, got %lld", (long long)bytes);
  const uintptr_t ua = reinterpret_cast<uintptr_t>(a), ub = reinterpret_cast<uintptr_t>(b);
  DOSX_CHECK_ARG(((ua | ub) & 15) == 0, "dosx_swap_buffers: buffers must be 16-byte aligned");
  DOSX_CHECK_ARG(ua != ub && (ua >= ub + (uintptr_t)bytes || ub >= ua + (uintptr_t)bytes), "dosx_swap_buffers: the buffers overlap");
  if (bytes == 0) return 0;
  const size_t nvec = (size_t)bytes / 16;
  size_t wgs = (nvec + DOSX_SWAP_THREADS - 1) / DOSX_SWAP_THREADS;
  if (wgs > (size_t)DOSX_SWAP_MAX_BLOCKS) wgs = DOSX_SWAP_MAX_BLOCKS;
  hipLaunchKernelGGL(swap_kernel, dim3((unsigned)wgs), dim3(DOSX_SWAP_THREADS), 0, to_stream(stream), static_cast<uint4*>(a),
                     static_cast<uint4*>(b), nvec);
  DOSX_LAUNCH_CHECK();
  return 0;
}
