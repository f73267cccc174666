// The float64 twin of pair_head.hip: the output head of Graphnetwork_phonon (graphnetwork_phonon.py:26,66-70) on its rank
// structure, in double - the phonon reference trains in float64 (main_phDOS.py:15-16).  With E1 = emb . W0[:, :H]^T + b0 [S, H] and
// C = graph . W0[:, H:]^T [B, H] (two small dosx_gemm_f64 calls on the caller's side)
//
//     dos[b, s] = b2 + sum_h w2[h] * leaky(E1[s, h] + C[b, h])                                   pair_head_fwd64_kernel
//
// and from ddos [B, S]                                                                           pair_head_bwd64_kernel
//
//     gate = E1[s, h] + C[b, h] > 0 ? 1 : slope
//     dE1[s, h] = w2[h] * sum_b ddos[b, s] * gate          dC[b, h] = w2[h] * sum_s ddos[b, s] * gate
//     partials[s] = [ sum_b ddos[b, s] * leaky(E1[s, :] + C[b, :])  (H) | sum_b ddos[b, s] ]      column sums = dw2, db2
//
// Nothing of S * B * H elements exists in memory.  A 16-byte access is a double2 - TWO columns, not the four of the fp32
// kernel - so the items are (row, 2-column chunk) and there are H / 2 chunks per row: the forward gives a (b, s) output 16
// lanes that take the chunks q, q + 16, ..., the backward's "b" workgroups own 64 (b, chunk) items and walk all S bins (one wave
// per quarter of them, the four quarter sums added in a fixed order through LDS), its "s" workgroups own 256 (s, chunk) items
// and walk all B crystals.  At S 51, B 64, H 128 that is 64 + 13 workgroups for 4 * 10^5 leaky-FMAs formed twice: the launches are
// latency-bound, and forming every pre-activation twice buys a backward without any hand-off between workgroups - every sum is
// one thread's sequential chain (plus the fixed four-term LDS sum, plus the fixed 16-lane tree of the forward): no atomics, the
// same bits on every run.  Plain loads and stores: E1, C and ddos together are well under 1 MB and stay in L2.
#include "common.h"

namespace {

__device__ __forceinline__ double leaky64(double p, double slope) { return p > 0.0 ? p : slope * p; }
__device__ __forceinline__ double2 ld2(const double* p) { return *reinterpret_cast<const double2*>(p); }
__device__ __forceinline__ void st2(double* p, double2 v) { *reinterpret_cast<double2*>(p) = v; }

// 16 lanes per output element (b, s): lane q takes the 2-column chunks q, q + 16, ...; one workgroup = 16 bins of one crystal.
__global__ __launch_bounds__(256) void pair_head_fwd64_kernel(const DosxPairHead64 a) {
  const int tid = threadIdx.x, q = tid & 15, grp = tid >> 4;
  const int S = a.S, H = a.H, H2 = H >> 1;
  const int nst = (S + 15) >> 4;
  const int b = (int)blockIdx.x / nst, st = (int)blockIdx.x - b * nst;
  const int s = st * 16 + grp, sc = min(s, S - 1);          // (rows past S recompute the last bin: every lane takes part in the sum)
  const double slope = a.slope;
  const double* e = a.e1 + (size_t)sc * H;
  const double* c = a.c + (size_t)b * H;
  double acc = 0.0;
  for (int k = q; k < H2; k += 16) {
    const double2 ev = ld2(e + 2 * k), cv = ld2(c + 2 * k), w = ld2(a.w2 + 2 * k);
    acc = fma(w.x, leaky64(ev.x + cv.x, slope), acc);
    acc = fma(w.y, leaky64(ev.y + cv.y, slope), acc);
  }
  // the 16 lanes' sums in a fixed tree (xor 8, 4, 2, 1 stays inside the 16-lane group); every lane ends with the same total
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (q == 0 && s < S) a.dos[(size_t)b * S + s] = acc + a.b2[0];
}

__global__ __launch_bounds__(256) void pair_head_bwd64_kernel(const DosxPairHead64 a, const int n_bblocks) {
  __shared__ __align__(16) double red[4 * 64 * 2];
  const int tid = threadIdx.x;
  const int S = a.S, B = a.B, H = a.H, H2 = H >> 1;
  const double slope = a.slope;
  if ((int)blockIdx.x < n_bblocks) {
    // ---- "b" workgroups: dC.  item = (b, 2-column chunk); wave w walks the bins w, w + 4, ... ----
    const int lane = tid & 63, wv = tid >> 6;
    const int it = (int)blockIdx.x * 64 + lane;
    const bool valid = it < B * H2;
    const int itc = valid ? it : B * H2 - 1;
    const int b = itc / H2, k = itc - b * H2;
    const double2 cv = ld2(a.c + (size_t)b * H + 2 * k);
    const double* dd = a.ddos + (size_t)b * S;
    double gx = 0.0, gy = 0.0;
#pragma unroll 4
    for (int s = wv; s < S; s += 4) {
      const double2 ev = ld2(a.e1 + (size_t)s * H + 2 * k);
      const double d = dd[s], ds = d * slope;
      gx += ev.x + cv.x > 0.0 ? d : ds;
      gy += ev.y + cv.y > 0.0 ? d : ds;
    }
    st2(red + (wv * 64 + lane) * 2, make_double2(gx, gy));
    __syncthreads();
    if (wv == 0 && valid) {
      const double2 g0 = ld2(red + lane * 2), g1 = ld2(red + (64 + lane) * 2), g2 = ld2(red + (128 + lane) * 2),
                    g3 = ld2(red + (192 + lane) * 2);
      const double2 w = ld2(a.w2 + 2 * k);
      st2(a.dc + (size_t)b * H + 2 * k, make_double2(w.x * ((g0.x + g1.x) + (g2.x + g3.x)), w.y * ((g0.y + g1.y) + (g2.y + g3.y))));
    }
    return;
  }
  // ---- "s" workgroups: dE1 and the parameter partials.  item = (s, 2-column chunk), all B crystals in order ----
  const int it = ((int)blockIdx.x - n_bblocks) * 256 + tid;
  if (it >= S * H2) return;
  const int s = it / H2, k = it - s * H2;
  const double2 ev = ld2(a.e1 + (size_t)s * H + 2 * k);
  double gx = 0.0, gy = 0.0, lx = 0.0, ly = 0.0, sd = 0.0;
#pragma unroll 4
  for (int b = 0; b < B; ++b) {
    const double2 cv = ld2(a.c + (size_t)b * H + 2 * k);
    const double d = a.ddos[(size_t)b * S + s], ds = d * slope;
    const double px = ev.x + cv.x, py = ev.y + cv.y;
    gx += px > 0.0 ? d : ds;
    gy += py > 0.0 ? d : ds;
    lx = fma(d, leaky64(px, slope), lx);
    ly = fma(d, leaky64(py, slope), ly);
    sd += d;
  }
  const double2 w = ld2(a.w2 + 2 * k);
  st2(a.de1 + (size_t)s * H + 2 * k, make_double2(w.x * gx, w.y * gy));
  double* prow = a.partials + (size_t)s * (H + 1) + 2 * k;      // (rows of H + 1 doubles: not 16-byte aligned)
  prow[0] = lx; prow[1] = ly;
  if (k == 0) a.partials[(size_t)s * (H + 1) + H] = sd;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// what both entries check; `who` names the entry in the message
int check_common(const DosxPairHead64* ap, const char* who) {
  DOSX_CHECK_ARG(ap != nullptr, "%s: null descriptor", who);
  const DosxPairHead64& a = *ap;
  DOSX_CHECK_ARG(a.S > 0 && a.B > 0 && a.H > 0, "%s: sizes must be positive, got S=%d B=%d H=%d", who, a.S, a.B, a.H);
  DOSX_CHECK_ARG(a.H % 8 == 0 && a.H <= 512, "%s: hidden %d unsupported (a multiple of 8, at most 512)", who, a.H);
  DOSX_CHECK_ARG((long long)a.S * a.B * a.H < (1LL << 31), "%s: S*B*H = %lld is past the 32-bit index range", who,
                 (long long)a.S * a.B * a.H);
  DOSX_CHECK_ARG(a.e1 && a.c && a.w2, "%s: null operand (e1 / c / w2)", who);
  DOSX_CHECK_ARG(aligned16(a.e1) && aligned16(a.c) && aligned16(a.w2), "%s: e1 / c / w2 must be 16-byte aligned", who);
  return 0;
}

}  // namespace

extern "C" int dosx_pair_head_fwd_f64(const DosxPairHead64* ap, dosx_stream_t stream) {
  if (const int rc = check_common(ap, "dosx_pair_head_fwd_f64")) return rc;
  const DosxPairHead64& a = *ap;
  DOSX_CHECK_ARG(a.b2 && a.dos, "dosx_pair_head_fwd_f64: null operand (b2 / dos)");
  const dim3 grid(a.B * ceil_div(a.S, 16));
  hipLaunchKernelGGL(pair_head_fwd64_kernel, grid, dim3(256), 0, to_stream(stream), a);
  DOSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int dosx_pair_head_bwd_f64(const DosxPairHead64* ap, dosx_stream_t stream) {
  if (const int rc = check_common(ap, "dosx_pair_head_bwd_f64")) return rc;
  const DosxPairHead64& a = *ap;
  DOSX_CHECK_ARG(a.ddos && a.de1 && a.dc && a.partials, "dosx_pair_head_bwd_f64: null operand (ddos / de1 / dc / partials)");
  DOSX_CHECK_ARG(aligned16(a.de1) && aligned16(a.dc), "dosx_pair_head_bwd_f64: de1 / dc must be 16-byte aligned");
  const int H2 = a.H / 2;
  const int nb = ceil_div(a.B * H2, 64), ns = ceil_div(a.S * H2, 256);
  hipLaunchKernelGGL(pair_head_bwd64_kernel, dim3(nb + ns), dim3(256), 0, to_stream(stream), a, nb);
  DOSX_LAUNCH_CHECK();
  return 0;
}
