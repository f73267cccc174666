// dosx_grad_accumulate / _f64 (include/dosx.h): dst[i] = a[i] + b[i] over the flat gradient, or dst[i] = a[i] (b == NULL) - what
// sums the gradients of the micro-batches of one optimizer step (train.py: step_accumulate), one launch behind each micro-batch's
// recorded program - and the same for ONE scalar (the window's loss).  One kernel template over the element type; 16-byte
// accesses (float4 / double2) as adamw.hip's, grid-stride over the vectors, the < 16-byte tail by the first threads of the grid
// one element each.  12 B (fp32) / 24 B (float64) per element, 8 / 16 for the copy: HBM-bound.
// Every element is ONE IEEE add of two loaded values: there is no product to contract and no atomic, so two runs are bitwise
// equal and the result is torch's a + b.  The copy form never reads dst.
// dst may BE a or b (not restrict-qualified): thread i reads the i-th vector of both operands before it stores the i-th of dst,
// and no other thread touches that vector.
#include "common.h"

#include <type_traits>

namespace {

template <typename T, bool ADD>
__global__ __launch_bounds__(DOSX_ACCUM_THREADS) void grad_accumulate_kernel(T* dst, const T* a, const T* b, const size_t n, T* sdst,
                                                                             const T* sa, const T* sb) {
  using Vec = typename std::conditional<sizeof(T) == 4, float4, double2>::type;
  constexpr int PER = 16 / (int)sizeof(T);
  const size_t nvec = n / PER;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (size_t i = tid; i < nvec; i += (size_t)gridDim.x * blockDim.x) {
    Vec x = reinterpret_cast<const Vec*>(a)[i];
    if constexpr (ADD) {
      const Vec y = reinterpret_cast<const Vec*>(b)[i];
      T* X = &x.x; const T* Y = &y.x;
#pragma unroll
      for (int j = 0; j < PER; ++j) X[j] = X[j] + Y[j];
    }
    reinterpret_cast<Vec*>(dst)[i] = x;
  }
  const size_t t0 = nvec * PER;
  if (tid < n - t0) {
    const size_t i = t0 + tid;
    T x = a[i];
    if constexpr (ADD) x = x + b[i];
    dst[i] = x;
  }
  if (sdst != nullptr && tid == 0) {        // the scalar triple: its own operands, its own add-or-copy (sb), one thread
    T s = sa[0];
    if (sb != nullptr) s = s + sb[0];
    sdst[0] = s;
  }
}

inline bool disjoint(uintptr_t x, uintptr_t xbytes, uintptr_t y, uintptr_t ybytes) { return x >= y + ybytes || y >= x + xbytes; }

template <typename T>
int grad_accumulate(const char* who, T* dst, const T* a, const T* b, int64_t n, T* sdst, const T* sa, const T* sb, dosx_stream_t stream) {
  DOSX_CHECK_ARG(dst && a, "%s: NULL dst or a", who);
  DOSX_CHECK_ARG(n >= 0, "%s: n must not be negative, got %lld", who, (long long)n);
  const uintptr_t ud = reinterpret_cast<uintptr_t>(dst), ua = reinterpret_cast<uintptr_t>(a), ub = reinterpret_cast<uintptr_t>(b);
  DOSX_CHECK_ARG(((ud | ua | ub) & 15) == 0, "%s: dst, a and b must be 16-byte aligned", who);
  const uintptr_t bytes = (uintptr_t)n * sizeof(T);
  DOSX_CHECK_ARG(ud == ua || disjoint(ud, bytes, ua, bytes), "%s: dst overlaps a partially (dst may be exactly a, or apart from it)", who);
  DOSX_CHECK_ARG(!b || ud == ub || disjoint(ud, bytes, ub, bytes), "%s: dst overlaps b partially (dst may be exactly b, or apart from it)",
                 who);
  DOSX_CHECK_ARG((sdst != nullptr) == (sa != nullptr), "%s: sdst and sa go together (both, or all three scalars NULL)", who);
  DOSX_CHECK_ARG(sdst || !sb, "%s: sb without sdst and sa", who);
  if (sdst) {
    const uintptr_t us[3] = {reinterpret_cast<uintptr_t>(sdst), reinterpret_cast<uintptr_t>(sa), reinterpret_cast<uintptr_t>(sb)};
    DOSX_CHECK_ARG(((us[0] | us[1] | us[2]) & (sizeof(T) - 1)) == 0, "%s: sdst, sa and sb must be aligned to their element", who);
    // another thread than the scalar's writes dst and reads a and b: the scalars live elsewhere
    for (int k = 0; k < 3; ++k)
      DOSX_CHECK_ARG(!us[k] || disjoint(us[k], sizeof(T), ud, bytes), "%s: a scalar operand lies inside dst[0, n)", who);
    DOSX_CHECK_ARG(disjoint(us[0], sizeof(T), ua, bytes) && (!b || disjoint(us[0], sizeof(T), ub, bytes)),
                   "%s: sdst lies inside a[0, n) or b[0, n)", who);
  }
  if (n == 0) return 0;
  size_t wgs = ((size_t)n / (16 / sizeof(T)) + DOSX_ACCUM_THREADS - 1) / DOSX_ACCUM_THREADS;
  if (wgs > (size_t)DOSX_ACCUM_MAX_BLOCKS) wgs = DOSX_ACCUM_MAX_BLOCKS;
  if (wgs < 1) wgs = 1;
  if (b)
    hipLaunchKernelGGL((grad_accumulate_kernel<T, true>), dim3((unsigned)wgs), dim3(DOSX_ACCUM_THREADS), 0, to_stream(stream), dst, a, b,
                       (size_t)n, sdst, sa, sb);
  else
    hipLaunchKernelGGL((grad_accumulate_kernel<T, false>), dim3((unsigned)wgs), dim3(DOSX_ACCUM_THREADS), 0, to_stream(stream), dst, a, b,
                       (size_t)n, sdst, sa, sb);
  DOSX_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int dosx_grad_accumulate(float* dst, const float* a, const float* b, int64_t n, float* sdst, const float* sa, const float* sb,
                                    dosx_stream_t stream) {
  return grad_accumulate<float>("dosx_grad_accumulate", dst, a, b, n, sdst, sa, sb, stream);
}

extern "C" int dosx_grad_accumulate_f64(double* dst, const double* a, const double* b, int64_t n, double* sdst, const double* sa,
                                        const double* sb, dosx_stream_t stream) {
  return grad_accumulate<double>("dosx_grad_accumulate_f64", dst, a, b, n, sdst, sa, sb, stream);
}
