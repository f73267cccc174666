// Gradient statistics of the guarded optimizer step (include/dosx.h: DosxStepGuard, dosx_grad_guard_f32 / _f64): one launch over
// the flat gradient, behind the recorded program and in front of the guarded AdamW, which reads the verdict from device memory.
// Per workgroup: the sum of squares of its finite elements (in double for both dtypes: the square of a float is exact there), the
// count of its non-finite elements and the lowest flat index among them.  Non-finite = all exponent bits set, tested on the bit
// pattern as csrc/validate.hip does.  The partials go through the publish / ticket / last-arriver protocol of common.h - used
// unchanged: sc1 publishes, dosx_last_arriver_wg, sc1 read-back, dosx_counter_reset - and the last arriver sums them in an order
// that depends on the grid alone, which depends on n alone.  No workgroup waits for another one: there is no poll.
#include "common.h"
#include "adamw_scalars.h"

#include <limits.h>
#include <math.h>

#include <type_traits>

namespace {

constexpr int GUARD_THREADS = DOSX_GUARD_THREADS;
constexpr int GUARD_MAX_BLOCKS = DOSX_GUARD_MAX_BLOCKS;
constexpr size_t GUARD_SLAB_OFFSET = 64;                  // the ticket counter owns the first 64 bytes of the workspace
static_assert(GUARD_SLAB_OFFSET + (size_t)GUARD_MAX_BLOCKS * 24 == DOSX_GUARD_WORKSPACE_BYTES, "workspace size of dosx.h");
static_assert(sizeof(DosxStepGuard) == 96, "DosxStepGuard is six 16-byte rows");
static_assert((GUARD_THREADS & (GUARD_THREADS - 1)) == 0, "the tree below halves the thread count");

// what the finishing thread needs beside the partials
struct GuardScalars {
  double max_norm;                 // < 0: none
  double lr, beta1, beta2;                     // (of an fp32 entry: floats, widened exactly)
  double host_step_size, host_bc2_scale;      // the unguarded entry's scalars for t = step (adamw_scalars.h)
  int step;
};

template <typename T>
inline long long guard_blocks(long long n) {
  constexpr long long PER = 16 / (long long)sizeof(T);
  const long long b = (n / PER + GUARD_THREADS - 1) / GUARD_THREADS;
  return b < 1 ? 1 : b > GUARD_MAX_BLOCKS ? GUARD_MAX_BLOCKS : b;
}

__device__ __forceinline__ bool nonfinite_bits(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }
__device__ __forceinline__ bool nonfinite_bits(double x) { return ((uint32_t)__double2hiint(x) & 0x7ff00000u) == 0x7ff00000u; }

struct GuardPartial {
  double sum;
  long long bad, first;
  template <typename T>
  __device__ __forceinline__ void take(T x, long long index) {
    if (nonfinite_bits(x)) { ++bad; first = index < first ? index : first; }
    else sum = fma((double)x, (double)x, sum);
  }
  __device__ __forceinline__ void merge(const GuardPartial& o) {
    sum += o.sum; bad += o.bad; first = o.first < first ? o.first : first;
  }
};

// the workgroup's partials -> thread 0, pairwise over halving distances: the order is a function of GUARD_THREADS alone
__device__ __forceinline__ GuardPartial guard_tree(GuardPartial v, double* s_sum, long long* s_bad, long long* s_first, int tid) {
  s_sum[tid] = v.sum; s_bad[tid] = v.bad; s_first[tid] = v.first;
  __syncthreads();
#pragma unroll
  for (int o = GUARD_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) {
      s_sum[tid] += s_sum[tid + o];
      s_bad[tid] += s_bad[tid + o];
      s_first[tid] = s_first[tid + o] < s_first[tid] ? s_first[tid + o] : s_first[tid];
    }
    __syncthreads();
  }
  return GuardPartial{s_sum[0], s_bad[0], s_first[0]};
}

template <typename T>
__global__ __launch_bounds__(GUARD_THREADS) void grad_guard_kernel(const T* __restrict__ g, const long long n, int* counter,
                                                                   double* slab_sum, long long* slab_bad, long long* slab_first,
                                                                   const int32_t* status, DosxStepGuard* rec, const GuardScalars a) {
  constexpr int PER = 16 / (int)sizeof(T);
  __shared__ double s_sum[GUARD_THREADS];
  __shared__ long long s_bad[GUARD_THREADS];
  __shared__ long long s_first[GUARD_THREADS];
  __shared__ int s_flag;
  const int tid = (int)threadIdx.x;
  const int nb = (int)gridDim.x;
  const long long nvec = n / PER;
  const long long stride = (long long)nb * GUARD_THREADS;
  const long long t0 = (long long)blockIdx.x * GUARD_THREADS + tid;
  GuardPartial mine{0.0, 0, LLONG_MAX};
  using Vec = typename std::conditional<PER == 4, float4, double2>::type;
  const Vec* gv = reinterpret_cast<const Vec*>(g);
  auto take_vec = [&](const Vec& w, long long v) {
    if constexpr (PER == 4) { mine.take(w.x, v * 4); mine.take(w.y, v * 4 + 1); mine.take(w.z, v * 4 + 2); mine.take(w.w, v * 4 + 3); }
    else { mine.take(w.x, v * 2); mine.take(w.y, v * 2 + 1); }
  };
  // four 16-byte loads in flight per lane, taken in the order of the plain grid-stride loop: the sums do not know the unrolling
  long long v = t0;
  for (; v + 3 * stride < nvec; v += 4 * stride) {
    const Vec w0 = gv[v], w1 = gv[v + stride], w2 = gv[v + 2 * stride], w3 = gv[v + 3 * stride];
    take_vec(w0, v); take_vec(w1, v + stride); take_vec(w2, v + 2 * stride); take_vec(w3, v + 3 * stride);
  }
  for (; v < nvec; v += stride) take_vec(gv[v], v);
  // scalar tail: fewer than PER elements, the first threads of the grid take one each
  const long long tail0 = nvec * PER;
  if (t0 < n - tail0) mine.take(g[tail0 + t0], tail0 + t0);

  const GuardPartial wg = guard_tree(mine, s_sum, s_bad, s_first, tid);
  if (tid == 0) {                                          // publish: agent-scope relaxed atomic stores = sc1 stores
    __hip_atomic_store(slab_sum + blockIdx.x, wg.sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(slab_bad + blockIdx.x, wg.bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(slab_first + blockIdx.x, wg.first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  const bool last = dosx_last_arriver_wg(counter, 0, nb, &s_flag, tid);
  if (!last) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   // (no instruction: keeps the loads below the ticket)
  // ---- last arriver: thread t reads the slots t, t + GUARD_THREADS, ... in rising order (sc1 loads), then the tree ----
  GuardPartial all{0.0, 0, LLONG_MAX};
  for (int i = tid; i < nb; i += GUARD_THREADS) {
    GuardPartial p;
    p.sum = __hip_atomic_load(slab_sum + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    p.bad = __hip_atomic_load(slab_bad + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    p.first = __hip_atomic_load(slab_first + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    all.merge(p);
  }
  const GuardPartial tot = guard_tree(all, s_sum, s_bad, s_first, tid);
  if (tid != 0) return;
  dosx_counter_reset(counter);                             // ready for the next launch

  // ---- the finishing thread ----
  const double sumsq = tot.sum;
  int reason = 0;
  if (tot.bad) reason |= DOSX_GUARD_NONFINITE;
  if (nonfinite_bits(sumsq)) reason |= DOSX_GUARD_OVERFLOW;
  if (status && __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != DOSX_EXCHANGE_OK) reason |= DOSX_GUARD_STALLED;
  const double norm = sqrt(sumsq);
  double clip = 1.0;
  if (a.max_norm >= 0.0) {
    const double c = a.max_norm / (norm + 1e-6);           // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max = 1)
    if (c < 1.0) clip = c;
  }
  const int skip = reason != 0;
  int applied = rec->applied, skipped = rec->skipped;
  if (skip) {
    if (skipped == 0) { rec->first_skip_step = a.step; rec->first_skip_reason = reason; rec->first_skip_bad = tot.bad ? tot.first : -1; }
    ++skipped;
  } else {
    ++applied;
  }
  // AdamW's time: a skipped step does not advance it.  Nothing skipped: the host's scalars, so that the run is the unguarded one
  const int t = a.step - skipped;
  double step_size = a.host_step_size, bc2_scale = a.host_bc2_scale;
  if (skipped != 0 && t >= 1) {
    step_size = (double)adamw_step_size<T>((T)a.lr, (T)a.beta1, t);
    bc2_scale = (double)adamw_bc2_scale<T>((T)a.beta2, t);
  }
  rec->sumsq = sumsq; rec->norm = norm; rec->clip = clip;
  rec->step_size = step_size; rec->bc2_scale = bc2_scale;
  rec->n_bad = tot.bad; rec->first_bad = tot.bad ? tot.first : -1;
  rec->skip = skip; rec->reason = reason; rec->t = t;
  rec->applied = applied; rec->skipped = skipped;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <typename T>
int grad_guard(const char* who, const T* g, int64_t n, double max_norm, const int32_t* status, T lr, T beta1, T beta2, int step,
               void* guard, void* workspace, dosx_stream_t stream) {
  DOSX_CHECK_ARG(g && guard && workspace, "%s: NULL gradient, record or workspace", who);
  DOSX_CHECK_ARG(n >= 0, "%s: n must not be negative, got %lld", who, (long long)n);
  DOSX_CHECK_ARG(step >= 1, "%s: step is the 1-based attempt count, got %d", who, step);
  DOSX_CHECK_ARG(max_norm == max_norm, "%s: max_norm is NaN (negative: no clipping)", who);
  DOSX_CHECK_ARG(aligned16(g) && aligned16(guard) && aligned16(workspace), "%s: buffers must be 16-byte aligned", who);
  DOSX_CHECK_ARG((reinterpret_cast<uintptr_t>(status) & 3) == 0, "%s: exchange_status must be 4-byte aligned", who);
  char* ws = static_cast<char*>(workspace);
  double* slab_sum = reinterpret_cast<double*>(ws + GUARD_SLAB_OFFSET);
  long long* slab_bad = reinterpret_cast<long long*>(slab_sum + GUARD_MAX_BLOCKS);
  long long* slab_first = slab_bad + GUARD_MAX_BLOCKS;
  const long long blocks = guard_blocks<T>((long long)n);
  const GuardScalars a{max_norm, (double)lr, (double)beta1, (double)beta2, (double)adamw_step_size<T>(lr, beta1, step),
                       (double)adamw_bc2_scale<T>(beta2, step), step};
  hipLaunchKernelGGL(grad_guard_kernel<T>, dim3((unsigned)blocks), dim3(GUARD_THREADS), 0, to_stream(stream), g, (long long)n,
                     reinterpret_cast<int*>(ws), slab_sum, slab_bad, slab_first, status, static_cast<DosxStepGuard*>(guard), a);
  DOSX_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int dosx_grad_guard_blocks(int64_t n, int elem_bytes) {
  DOSX_CHECK_ARG(n >= 0 && (elem_bytes == 4 || elem_bytes == 8), "dosx_grad_guard_blocks: n=%lld, elem_bytes=%d (4 or 8)", (long long)n, elem_bytes);
  return (int)(elem_bytes == 4 ? guard_blocks<float>((long long)n) : guard_blocks<double>((long long)n));
}

extern "C" int dosx_grad_guard_f32(const float* g, int64_t n, double max_norm, const int32_t* exchange_status, float lr, float beta1,
                                   float beta2, int step, void* guard, void* workspace, dosx_stream_t stream) {
  return grad_guard<float>("dosx_grad_guard_f32", g, n, max_norm, exchange_status, lr, beta1, beta2, step, guard, workspace, stream);
}

extern "C" int dosx_grad_guard_f64(const double* g, int64_t n, double max_norm, const int32_t* exchange_status, double lr,
                                   double beta1, double beta2, int step, void* guard, void* workspace, dosx_stream_t stream) {
  return grad_guard<double>("dosx_grad_guard_f64", g, n, max_norm, exchange_status, lr, beta1, beta2, step, guard, workspace, stream);
}
