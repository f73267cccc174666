// Batch validation (include/dosx.h: dosx_batch_check, dosx_finite_check_f32 / _f64): the fail-loudly path in front of everything
// that dereferences a batch.  The checkers run over the CALLER'S arrays in the reference schema (edge_index [2,E] / batch [N] /
// system [B], int64) before any metadata is derived from them, and are written so that no value they read can steer a read:
// array lengths are the caller's tensor shapes, an index is compared with its bounds as a 64-bit value before it is used, and the
// only indexed reads - batch[src], batch[dst] of R2 and crystal_count[batch[i]] - sit behind the range test of that very value.
// The report is a handful of {count, first} pairs formed with vector atomics (a saturating sum and a minimum: the same pair in
// whatever order they arrive): offending threads gather in LDS, one thread per workgroup and rule adds to the report; the violation
// path is cold, a clean batch issues no atomic but the per-crystal node counts.
#include "common.h"

#include <limits.h>

namespace {

constexpr int CHECK_THREADS = DOSX_CHECK_THREADS;
constexpr int CHECK_MAX_BLOCKS = DOSX_CHECK_MAX_BLOCKS;
constexpr int FINITE_THREADS = 256;
constexpr int FINITE_MAX_BLOCKS = 2048;       // 8 workgroups of 4 waves per CU: enough 16-byte loads in flight for a streaming read

// workgroups for `items` (> 0) items: one thread each up to the cap, then the grid strides (64-bit: items may be close to INT32_MAX)
inline int check_blocks(int items) {
  const long long b = ((long long)items + CHECK_THREADS - 1) / CHECK_THREADS;
  return (int)(b < CHECK_MAX_BLOCKS ? b : CHECK_MAX_BLOCKS);
}

// count += v saturating at INT32_MAX; first = min(first, index).  Called by ONE thread per workgroup and rule, and only when the
// workgroup found a violation: the compare-and-swap loop has at most gridDim.x contenders (a loop that every offending THREAD
// entered would serialise on this one word - quadratically in the offenders).
__device__ __forceinline__ void report_add(int32_t* slot, long long v, int32_t index) {
  int32_t old = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  while (true) {
    const long long sum = (long long)old + v;
    const int32_t want = sum > (long long)INT_MAX ? INT_MAX : (int32_t)sum;
    if (want == old) break;
    const int32_t seen = atomicCAS(slot, old, want);
    if (seen == old) break;
    old = seen;
  }
  atomicMin(slot + 1, index);
}
__device__ __forceinline__ int32_t clamp_index(long long index) {
  return (int32_t)(index > (long long)(INT_MAX - 1) ? (long long)(INT_MAX - 1) : index);
}

// A workgroup's findings, gathered in LDS (count and smallest index per slot; only offending threads touch them) and handed to the
// report by one thread per slot.  NSLOT slots; rule_of[k] = the rule slot k reports.
template <int NSLOT>
struct WgFindings {
  unsigned long long count[NSLOT];
  int32_t first[NSLOT];
  __device__ __forceinline__ void init(int tid) {
    if (tid < NSLOT) { count[tid] = 0ull; first[tid] = INT_MAX; }
    __syncthreads();
  }
  __device__ __forceinline__ void add(int k, long long n, long long index) {
    atomicAdd(&count[k], (unsigned long long)n);
    atomicMin(&first[k], clamp_index(index));
  }
  // slot k of the workgroup -> report pair `pair_of(k)`
  template <typename F>
  __device__ __forceinline__ void flush(int tid, int32_t* report, F pair_of) {
    __syncthreads();
    if (tid < NSLOT && count[tid]) report_add(report + 2 * pair_of(tid), (long long)count[tid], first[tid]);
  }
};

// R1, R2, R7 over the edges; R3 and the per-crystal node counts over the nodes.  One grid-stride sweep over max(E, N) items.
__global__ __launch_bounds__(CHECK_THREADS) void batch_check_kernel(const DosxBatchCheck a, int32_t* report) {
  __shared__ WgFindings<4> found;                   // slots: R1, R2, R3, R7
  const int tid = (int)threadIdx.x;
  found.init(tid);
  const long long N = a.N, E = a.E, B = a.B;
  const long long* src = a.edge_index;
  const long long* dst = a.edge_index + E;
  const long long items = E > N ? E : N;
  const long long stride = (long long)gridDim.x * CHECK_THREADS;
  for (long long i = (long long)blockIdx.x * CHECK_THREADS + tid; i < items; i += stride) {
    if (i < E) {
      const long long s = src[i], d = dst[i];
      if (s < 0 || s >= N || d < 0 || d >= N) found.add(0, 1, i);
      else if (a.batch[s] != a.batch[d]) found.add(1, 1, i);                 // (both endpoints passed their range test)
      if (a.require_sorted && i > 0 && d < dst[i - 1]) found.add(3, 1, i);
    }
    if (i < N) {
      const long long b = a.batch[i];
      const bool in_range = b >= 0 && b < B;
      if (!in_range || (i > 0 ? b < a.batch[i - 1] : b != 0)) found.add(2, 1, i);
      if (in_range) atomicAdd(a.crystal_count + b, 1);
    }
  }
  found.flush(tid, report, [](int k) { return k < 3 ? k : 6; });             // pairs of R1, R2, R3, R7
}

// R4, R5, R6 over the crystals, behind the node counts of the launch above.
__global__ __launch_bounds__(CHECK_THREADS) void crystal_check_kernel(const DosxBatchCheck a, int32_t* report) {
  __shared__ WgFindings<3> found;                   // slots: R4, R5, R6
  const int tid = (int)threadIdx.x;
  found.init(tid);
  const int stride = (int)gridDim.x * CHECK_THREADS;
  for (int b = (int)blockIdx.x * CHECK_THREADS + tid; b < a.B; b += stride) {
    const int32_t n = a.crystal_count[b];
    if (n == 0) found.add(0, 1, b);
    if (a.system) {
      const long long s = a.system[b];
      if (s < 0 || s >= (long long)a.prompts) found.add(1, 1, b);
    }
    if (a.n_max > 0 && n > a.n_max) found.add(2, 1, b);
  }
  found.flush(tid, report, [](int k) { return 3 + k; });                     // pairs of R4, R5, R6
}

// Non-finite = all exponent bits set; tested on the bit pattern, so no floating-point mode or compiler flag has a say.
__device__ __forceinline__ int nonfinite32(uint32_t w) { return (w & 0x7f800000u) == 0x7f800000u; }
__device__ __forceinline__ int nonfinite64(uint32_t hi) { return (hi & 0x7ff00000u) == 0x7ff00000u; }

// T = float: 4 elements per 16-byte load, T = double: 2.  head: leading elements in front of the first 16-byte boundary.
template <typename T>
__global__ __launch_bounds__(FINITE_THREADS) void finite_check_kernel(const T* p, const long long n, const long long head, int32_t* slot) {
  constexpr int PER = 16 / (int)sizeof(T);
  __shared__ WgFindings<1> found;
  const int tid = (int)threadIdx.x;
  found.init(tid);
  const long long nvec = (n - head) / PER;
  const uint4* pv = reinterpret_cast<const uint4*>(p + head);
  const long long stride = (long long)gridDim.x * FINITE_THREADS;
  const long long t0 = (long long)blockIdx.x * FINITE_THREADS + threadIdx.x;
  long long bad = 0, first = LLONG_MAX;
  for (long long v = t0; v < nvec; v += stride) {
    const uint4 w = pv[v];
    int hit[4];
    if constexpr (PER == 4) { hit[0] = nonfinite32(w.x); hit[1] = nonfinite32(w.y); hit[2] = nonfinite32(w.z); hit[3] = nonfinite32(w.w); }
    else { hit[0] = nonfinite64(w.y); hit[1] = nonfinite64(w.w); hit[2] = hit[3] = 0; }
    if (hit[0] | hit[1] | hit[2] | hit[3]) {
#pragma unroll
      for (int k = PER - 1; k >= 0; --k)
        if (hit[k]) { ++bad; const long long idx = head + v * PER + k; first = idx < first ? idx : first; }
    }
  }
  // scalar head and tail: fewer than 2 * PER elements, the first threads of the grid take one each
  const long long tail0 = head + nvec * PER;
  const long long nscalar = head + (n - tail0);
  if (t0 < nscalar) {
    const long long idx = t0 < head ? t0 : tail0 + (t0 - head);
    int hit;
    if constexpr (PER == 4) hit = nonfinite32(reinterpret_cast<const uint32_t*>(p)[idx]);
    else hit = nonfinite64(reinterpret_cast<const uint32_t*>(p)[2 * idx + 1]);
    if (hit) { ++bad; first = idx < first ? idx : first; }
  }
  if (bad) found.add(0, bad, first);
  found.flush(tid, slot, [](int) { return 0; });
}

template <typename T>
int finite_check(const char* who, const T* p, int64_t n, int32_t* slot, dosx_stream_t stream) {
  DOSX_CHECK_ARG(n >= 0, "%s: negative size n=%lld", who, (long long)n);
  DOSX_CHECK_ARG(slot != nullptr, "%s: null report slot", who);
  if (n == 0) return 0;
  DOSX_CHECK_ARG(p != nullptr, "%s: null tensor with n=%lld", who, (long long)n);
  DOSX_CHECK_ARG((reinterpret_cast<uintptr_t>(p) & (sizeof(T) - 1)) == 0, "%s: tensor not aligned to its element size", who);
  constexpr int PER = 16 / (int)sizeof(T);
  long long head = (long long)((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) / (long long)sizeof(T);
  if (head > n) head = n;
  const long long nvec = (n - head) / PER;
  long long blocks = (nvec + FINITE_THREADS - 1) / FINITE_THREADS;
  blocks = blocks < 1 ? 1 : blocks > FINITE_MAX_BLOCKS ? FINITE_MAX_BLOCKS : blocks;      // (one workgroup covers head + tail: < 2 * PER)
  hipLaunchKernelGGL(finite_check_kernel<T>, dim3((unsigned)blocks), dim3(FINITE_THREADS), 0, to_stream(stream), p, (long long)n, head, slot);
  DOSX_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int dosx_batch_check(const DosxBatchCheck* dp, int32_t* report, dosx_stream_t stream) {
  DOSX_CHECK_ARG(dp != nullptr, "dosx_batch_check: null descriptor");
  const DosxBatchCheck& d = *dp;
  DOSX_CHECK_ARG(report != nullptr, "dosx_batch_check: null report (%d {count, first} pairs of device memory)", DOSX_CHECK_RULES);
  DOSX_CHECK_ARG(d.N >= 0 && d.E >= 0 && d.B >= 0 && d.n_max >= 0 && d.prompts >= 0,
                 "dosx_batch_check: negative size (N=%d E=%d B=%d n_max=%d prompts=%d)", d.N, d.E, d.B, d.n_max, d.prompts);
  DOSX_CHECK_ARG(d.edge_index != nullptr || d.E == 0, "dosx_batch_check: null edge_index with E=%d", d.E);
  DOSX_CHECK_ARG(d.batch != nullptr || d.N == 0, "dosx_batch_check: null batch with N=%d", d.N);
  DOSX_CHECK_ARG(d.crystal_count != nullptr || d.B == 0, "dosx_batch_check: null crystal_count scratch with B=%d", d.B);
  hipStream_t st = to_stream(stream);
  if (d.B > 0) {
    const hipError_t e = hipMemsetAsync(d.crystal_count, 0, sizeof(int32_t) * (size_t)d.B, st);
    if (e != hipSuccess) {
      dosx_set_error("dosx_batch_check: clearing the crystal counts failed: %s", hipGetErrorString(e));
      return -5;
    }
  }
  const int items = d.E > d.N ? d.E : d.N;
  if (items > 0) {
    const int blocks = check_blocks(items);
    hipLaunchKernelGGL(batch_check_kernel, dim3(blocks), dim3(CHECK_THREADS), 0, st, d, report);
    DOSX_LAUNCH_CHECK();
  }
  if (d.B > 0) {
    const int blocks = check_blocks(d.B);
    hipLaunchKernelGGL(crystal_check_kernel, dim3(blocks), dim3(CHECK_THREADS), 0, st, d, report);
    DOSX_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int dosx_finite_check_f32(const float* p, int64_t n, int32_t* report_slot, dosx_stream_t stream) {
  return finite_check<float>("dosx_finite_check_f32", p, n, report_slot, stream);
}

extern "C" int dosx_finite_check_f64(const double* p, int64_t n, int32_t* report_slot, dosx_stream_t stream) {
  return finite_check<double>("dosx_finite_check_f64", p, n, report_slot, stream);
}
