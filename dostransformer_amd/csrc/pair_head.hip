// The output head of the GNN-only baselines (graphnetwork_phonon.py:26,66-70, graphnetwork.py:22,38-42, mlp.py:20,30-34) on its
// rank structure.  The head's input row (s, b) is cat[emb[s] | graph[b]], so the first Linear is E1[s] + C[b] with
// E1 = emb . W0[:, :H]^T + b0 [S, H] and C = graph . W0[:, H:]^T [B, H] (two small dosx_gemm calls); what is left is
//
//     dos[b, s] = b2 + sum_h w2[h] * leaky(E1[s, h] + C[b, h])                                   pair_head_fwd_kernel
//
// and its backward from ddos [B, S]                                                              pair_head_bwd_kernel
//
//     gate = E1[s, h] + C[b, h] > 0 ? 1 : slope
//     dE1[s, h] = w2[h] * sum_b ddos[b, s] * gate          dC[b, h] = w2[h] * sum_s ddos[b, s] * gate
//     dw2[h]    = sum_{s, b} ddos[b, s] * leaky(pre)       db2      = sum_{s, b} ddos[b, s]
//
// Nothing of S * B * H elements exists in memory.  The work is S * B * H leaky-FMAs (3.3 M at Electron-DOS width): the
// launches are latency-bound, so the backward spends arithmetic to stay free of any hand-off between workgroups.  Its
// grid has two kinds of workgroups: the "b" kind owns 64 (b, 4-column) items and walks all S bins (one wave per quarter of
// them, the four quarter sums added in a fixed order through LDS) - dC; the "s" kind owns 256 (s, 4-column) items and walks
// all B crystals - dE1 and one row of parameter partials [dw2 (H) | db2] per bin, which the caller's GradSink reduces with
// its other row partials.  Every pre-activation is thus formed twice (6.6 M instead of 3.3 M adds - less than a microsecond
// of one round of workgroups), and in exchange no slab is published, no ticket is drawn and nothing is read back: every sum
// is one thread's sequential chain (plus the fixed four-term LDS sum), the same on every run.
// Plain loads: E1, C and ddos together are under 400 KB and stay in L2.
#include "common.h"

namespace {

__device__ __forceinline__ float leaky(float p, float slope) { return p > 0.f ? p : slope * p; }

// 16 lanes per output element (b, s): lane q takes the 4-column chunks q, q + 16, ...; one workgroup = 16 bins of one crystal.
__global__ __launch_bounds__(256) void pair_head_fwd_kernel(const DosxPairHead a) {
  DOSX_SET_MAIN_PRIO();
  const int tid = threadIdx.x, q = tid & 15, grp = tid >> 4;
  const int S = a.S, H = a.H, H4 = H >> 2;
  const int nst = (S + 15) >> 4;
  const int b = (int)blockIdx.x / nst, st = (int)blockIdx.x - b * nst;
  const int s = st * 16 + grp, sc = min(s, S - 1);          // (rows past S recompute the last bin: every lane reaches the row sum)
  const float slope = a.slope;
  const float* e = a.e1 + (size_t)sc * H;
  const float* c = a.c + (size_t)b * H;
  float acc = 0.f;
  for (int k = q; k < H4; k += 16) {
    const float4 ev = ld4(e + 4 * k), cv = ld4(c + 4 * k), w = ld4(a.w2 + 4 * k);
    acc = fmaf(w.x, leaky(ev.x + cv.x, slope), acc);
    acc = fmaf(w.y, leaky(ev.y + cv.y, slope), acc);
    acc = fmaf(w.z, leaky(ev.z + cv.z, slope), acc);
    acc = fmaf(w.w, leaky(ev.w + cv.w, slope), acc);
  }
  acc = row16_sum(acc);
  if (q == 0 && s < S) a.dos[(size_t)b * S + s] = acc + a.b2[0];
}

__global__ __launch_bounds__(256) void pair_head_bwd_kernel(const DosxPairHead a, const int n_bblocks) {
  DOSX_SET_MAIN_PRIO();
  __shared__ __align__(16) float red[4 * 64 * 4];
  const int tid = threadIdx.x;
  const int S = a.S, B = a.B, H = a.H, H4 = H >> 2;
  const float slope = a.slope;
  if ((int)blockIdx.x < n_bblocks) {
    // ---- "b" workgroups: dC.  item = (b, 4-column chunk); wave w walks the bins w, w + 4, ... ----
    const int it = (int)blockIdx.x * 64 + (tid & 63), wv = tid >> 6;
    const bool valid = it < B * H4;
    const int itc = valid ? it : B * H4 - 1;
    const int b = itc / H4, k = itc - b * H4;
    const float4 cv = ld4(a.c + (size_t)b * H + 4 * k);
    const float* dd = a.ddos + (size_t)b * S;
    float4 g = f4zero();
#pragma unroll 4
    for (int s = wv; s < S; s += 4) {
      const float4 ev = ld4(a.e1 + (size_t)s * H + 4 * k);
      const float d = dd[s], ds = d * slope;
      g.x += ev.x + cv.x > 0.f ? d : ds;
      g.y += ev.y + cv.y > 0.f ? d : ds;
      g.z += ev.z + cv.z > 0.f ? d : ds;
      g.w += ev.w + cv.w > 0.f ? d : ds;
    }
    st4(red + (wv * 64 + (tid & 63)) * 4, g);
    __syncthreads();
    if (wv == 0 && valid) {
      const float4 g0 = ld4(red + tid * 4), g1 = ld4(red + (64 + tid) * 4), g2 = ld4(red + (128 + tid) * 4), g3 = ld4(red + (192 + tid) * 4);
      const float4 w = ld4(a.w2 + 4 * k);
      st4(a.dc + (size_t)b * H + 4 * k, make_float4(w.x * ((g0.x + g1.x) + (g2.x + g3.x)), w.y * ((g0.y + g1.y) + (g2.y + g3.y)),
                                                     w.z * ((g0.z + g1.z) + (g2.z + g3.z)), w.w * ((g0.w + g1.w) + (g2.w + g3.w))));
    }
    return;
  }
  // ---- "s" workgroups: dE1 and the parameter partials.  item = (s, 4-column chunk), all B crystals in order ----
  const int it = ((int)blockIdx.x - n_bblocks) * 256 + tid;
  if (it >= S * H4) return;
  const int s = it / H4, k = it - s * H4;
  const float4 ev = ld4(a.e1 + (size_t)s * H + 4 * k);
  float4 g = f4zero(), lw = f4zero();
  float sd = 0.f;
#pragma unroll 4
  for (int b = 0; b < B; ++b) {
    const float4 cv = ld4(a.c + (size_t)b * H + 4 * k);
    const float d = a.ddos[(size_t)b * S + s], ds = d * slope;
    const float px = ev.x + cv.x, py = ev.y + cv.y, pz = ev.z + cv.z, pw = ev.w + cv.w;
    g.x += px > 0.f ? d : ds;
    g.y += py > 0.f ? d : ds;
    g.z += pz > 0.f ? d : ds;
    g.w += pw > 0.f ? d : ds;
    lw.x = fmaf(d, leaky(px, slope), lw.x);
    lw.y = fmaf(d, leaky(py, slope), lw.y);
    lw.z = fmaf(d, leaky(pz, slope), lw.z);
    lw.w = fmaf(d, leaky(pw, slope), lw.w);
    sd += d;
  }
  const float4 w = ld4(a.w2 + 4 * k);
  st4(a.de1 + (size_t)s * H + 4 * k, make_float4(w.x * g.x, w.y * g.y, w.z * g.z, w.w * g.w));
  float* prow = a.partials + (size_t)s * (H + 1) + 4 * k;       // (rows of H + 1 floats: not 16-byte aligned)
  prow[0] = lw.x; prow[1] = lw.y; prow[2] = lw.z; prow[3] = lw.w;
  if (k == 0) a.partials[(size_t)s * (H + 1) + H] = sd;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// what both entries check; `who` names the entry in the message
int check_common(const DosxPairHead* ap, const char* who) {
  DOSX_CHECK_ARG(ap != nullptr, "%s: null descriptor", who);
  const DosxPairHead& a = *ap;
  DOSX_CHECK_ARG(a.S > 0 && a.B > 0 && a.H > 0, "%s: sizes must be positive, got S=%d B=%d H=%d", who, a.S, a.B, a.H);
  DOSX_CHECK_ARG(a.H % 8 == 0 && a.H <= 512, "%s: hidden %d unsupported (a multiple of 8, at most 512)", who, a.H);
  DOSX_CHECK_ARG((long long)a.S * a.B * a.H < (1LL << 31), "%s: S*B*H = %lld is past the 32-bit index range", who,
                 (long long)a.S * a.B * a.H);
  DOSX_CHECK_ARG(a.e1 && a.c && a.w2, "%s: null operand (e1 / c / w2)", who);
  DOSX_CHECK_ARG(aligned16(a.e1) && aligned16(a.c) && aligned16(a.w2), "%s: e1 / c / w2 must be 16-byte aligned", who);
  return 0;
}

}  // namespace

extern "C" int dosx_pair_head_partial_rows(int S, int B) { return (S > 0 && B > 0) ? S : 0; }

extern "C" int dosx_pair_head_fwd(const DosxPairHead* ap, dosx_stream_t stream) {
  if (const int rc = check_common(ap, "dosx_pair_head_fwd")) return rc;
  const DosxPairHead& a = *ap;
  DOSX_CHECK_ARG(a.b2 && a.dos, "dosx_pair_head_fwd: null operand (b2 / dos)");
  const dim3 grid(a.B * ceil_div(a.S, 16));
  hipLaunchKernelGGL(pair_head_fwd_kernel, grid, dim3(256), 0, to_stream(stream), a);
  DOSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int dosx_pair_head_bwd(const DosxPairHead* ap, dosx_stream_t stream) {
  if (const int rc = check_common(ap, "dosx_pair_head_bwd")) return rc;
  const DosxPairHead& a = *ap;
  DOSX_CHECK_ARG(a.ddos && a.de1 && a.dc && a.partials, "dosx_pair_head_bwd: null operand (ddos / de1 / dc / partials)");
  DOSX_CHECK_ARG(aligned16(a.de1) && aligned16(a.dc), "dosx_pair_head_bwd: de1 / dc must be 16-byte aligned");
  const int H4 = a.H / 4;
  const int nb = ceil_div(a.B * H4, 64), ns = ceil_div(a.S * H4, 256);
  hipLaunchKernelGGL(pair_head_bwd_kernel, dim3(nb + ns), dim3(256), 0, to_stream(stream), a, nb);
  DOSX_LAUNCH_CHECK();
  return 0;
}
