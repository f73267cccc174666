// DOS targets of a whole dataset from raw spectra: Gaussian broadening onto a grid (dosx_spectra_broaden) and linear resampling
// onto it (dosx_spectra_interp).  The definition - grid, shift, trapezoid weights, the keep test, the order of every sum, the
// report - is the contract in include/dosx.h (DosxSpectra, DosxSpectraInterp); the numpy twin is dostransformer_amd/spectra.py.
//
// Work decomposition: one workgroup of 256 lanes (4 waves) per crystal; lane t owns the bins t, t + 256, ... (at most 4).
//   broaden   the samples go through LDS in tiles of 256 as (ec_i, w_i * g): shift, trapezoid weight and normalisation are formed
//             once per sample, by the lane that stages it, together with the sample's share of the report.  Every lane then walks
//             the tile in index order and adds the kept terms to its bins' accumulators, so a bin's sum runs in ascending i
//             whatever the tile size.  A lane leaves a tile out for a bin when the tile's range [min ec, max ec] lies further
//             from E_s than cutoff * sigma * (1 + 2^-30): every term of such a tile fails the keep test (the slack covers the
//             three roundings between the two tests), so skipping drops only what the keep test drops.  A wave's bins are
//             contiguous, so on a sorted curve whole waves leave most tiles.
//   interp    a lane finds the last sample at or below each of its bins by bisection in global memory.
//   epilogue  (both) the row is collected in LDS; lane 0 walks it once in ascending s for y_max and area; the report's counts are
//             integer sums over the lanes; then the row, or NaN for a refused crystal, is stored.
// No atomics, no dependence on scheduling; every store is a plain vector store.
#include "common.h"

// sums and decisions are compared with the numpy twin: no fused multiply-adds in this file (see nl_geom.h)
#pragma clang fp contract(off)

namespace {

constexpr int SP_THREADS = 256;
constexpr int SP_WAVES = SP_THREADS / 64;
constexpr int SP_TILE = SP_THREADS;               // one staged sample per lane and tile
constexpr int SP_MAX_BINS = 1024;
constexpr double SP_SQRT_2PI = 2.5066282746310002;
constexpr double SP_SKIP_SLACK = 1.0 + 0x1p-30;

struct SpOut {
  double* y;
  double* y_max;
  double* area;
  double* y_norm;
  int32_t* report;
};

__device__ __forceinline__ double sp_grid(double e0, double de, int s) { return e0 + de * (double)s; }
__device__ __forceinline__ bool sp_finite(double a) { return __builtin_isfinite(a); }
__device__ __forceinline__ double sp_nan() { return __builtin_nan(""); }

// Is [a0, a1) a range of [0, T) with n_min <= a1 - a0 <= n_max?  (ptr is the caller's; nothing outside it is ever read)
__device__ __forceinline__ bool sp_range_ok(int a0, int a1, int T, int n_min, int n_max) {
  return a0 >= 0 && a1 >= a0 && a1 <= T && a1 - a0 >= n_min && a1 - a0 <= n_max;
}

// A crystal whose range is not what the caller stated: NaN everywhere, report (0, 0, -1, 0).
__device__ __forceinline__ void sp_reject(const SpOut& o, int c, int S) {
  for (int s = threadIdx.x; s < S; s += SP_THREADS) {
    o.y[(size_t)c * S + s] = sp_nan();
    if (o.y_norm) o.y_norm[(size_t)c * S + s] = sp_nan();
  }
  if (threadIdx.x == 0) {
    o.y_max[c] = sp_nan(), o.area[c] = sp_nan();
    o.report[c * 4 + 0] = 0, o.report[c * 4 + 1] = 0, o.report[c * 4 + 2] = -1, o.report[c * 4 + 3] = 0;
  }
}

// The shared epilogue.  `row[0..S)` holds the crystal's bins (written by their owners before the call); the three counts are each
// lane's share.  cnt [3][SP_WAVES], stat [1] are LDS.
__device__ __forceinline__ void sp_finish(const SpOut& o, int c, int S, double de, const double* row, int* cnt, double* stat,
                                          int n_inside, int bad, int unsorted, int covered, bool curve) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    n_inside += __shfl_xor(n_inside, s);
    bad += __shfl_xor(bad, s);
    unsorted += __shfl_xor(unsorted, s);
  }
  if (lane == 0) cnt[wave] = n_inside, cnt[SP_WAVES + wave] = bad, cnt[2 * SP_WAVES + wave] = unsorted;
  __syncthreads();                                // the counts, and every owner's row[] entries
  n_inside = bad = unsorted = 0;
#pragma unroll
  for (int w = 0; w < SP_WAVES; ++w) n_inside += cnt[w], bad += cnt[SP_WAVES + w], unsorted += cnt[2 * SP_WAVES + w];
  const bool refused = bad > 0 || (curve && unsorted > 0);
  if (tid == 0) {
    double m = row[0], sum = 0.0;
    for (int s = 0; s < S; ++s) {                 // ascending s: the order of `area` is part of the contract
      const double ys = row[s];
      sum += ys;
      m = ys > m ? ys : m;
    }
    stat[0] = m;
    o.y_max[c] = refused ? sp_nan() : m;
    o.area[c] = refused ? sp_nan() : de * sum;
    o.report[c * 4 + 0] = n_inside, o.report[c * 4 + 1] = covered, o.report[c * 4 + 2] = bad, o.report[c * 4 + 3] = unsorted;
  }
  __syncthreads();
  const double m = stat[0];
  for (int s = tid; s < S; s += SP_THREADS) {
    const double ys = row[s];
    o.y[(size_t)c * S + s] = refused ? sp_nan() : ys;
    if (o.y_norm) o.y_norm[(size_t)c * S + s] = refused ? sp_nan() : (m > 0.0 ? ys / m : 0.0);
  }
}

// NB = bins per lane = ceil(S / 256)
template <int NB>
__global__ __launch_bounds__(SP_THREADS) void spectra_broaden_kernel(const DosxSpectra d) {
  __shared__ double tile_e[SP_TILE], tile_w[SP_TILE];
  __shared__ double row[NB * SP_THREADS];
  __shared__ double range[2][SP_WAVES];
  __shared__ double stat[1];
  __shared__ int cnt[3 * SP_WAVES];
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int S = d.S;
  const SpOut o{d.y, d.y_max, d.area, d.y_norm, d.report};
  const int a0 = d.ptr[c], a1 = d.ptr[c + 1];
  if (!sp_range_ok(a0, a1, d.T, d.n_min, d.n_max)) {
    sp_reject(o, c, S);
    return;
  }
  const int n = a1 - a0;
  const bool curve = d.kind == DOSX_SPECTRA_CURVE;
  const double* e = d.e + a0;
  const double* v = d.v + a0;
  const double sigma = d.sigma[c], shift = d.shift[c], cutoff = d.cutoff;
  const double reach = cutoff * sigma;
  const double E_first = sp_grid(d.e0, d.de, 0), E_last = sp_grid(d.e0, d.de, S - 1);
  const double lo = E_first - reach, hi = E_last + reach;
  const double g = 1.0 / (sigma * SP_SQRT_2PI);
  const double margin = reach * SP_SKIP_SLACK;

  double E[NB], acc[NB];
  bool own[NB];
#pragma unroll
  for (int k = 0; k < NB; ++k) {
    const int s = tid + k * SP_THREADS;
    own[k] = s < S;
    E[k] = sp_grid(d.e0, d.de, own[k] ? s : S - 1);
    acc[k] = 0.0;
  }
  int n_inside = 0, unsorted = 0;
  int bad = tid == 0 ? (int)!(sigma > 0.0 && sp_finite(sigma)) + (int)!sp_finite(shift) : 0;

  for (int base = 0; base < n; base += SP_TILE) {  // workgroup-uniform trip count
    const int i = base + tid;
    double ec = 0.0, wg = 0.0;
    double mn = __builtin_inf(), mx = -__builtin_inf();
    if (i < n) {
      const double ei = e[i], vi = v[i];
      ec = ei - shift;
      double w = vi;
      if (curve) {
        const double el = i > 0 ? e[i - 1] : ei, er = i + 1 < n ? e[i + 1] : ei;
        w = vi * (0.5 * (er - el));
        unsorted += (i + 1 < n && er <= ei) ? 1 : 0;
      }
      wg = w * g;
      bad += (sp_finite(ei) && sp_finite(vi)) ? 0 : 1;
      n_inside += (lo <= ec && ec <= hi) ? 1 : 0;
      mn = mx = ec;
    }
    tile_e[tid] = ec, tile_w[tid] = wg;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      const double a = __shfl_xor(mn, s), b = __shfl_xor(mx, s);
      mn = a < mn ? a : mn;
      mx = b > mx ? b : mx;
    }
    if (lane == 0) range[0][wave] = mn, range[1][wave] = mx;
    __syncthreads();
    mn = range[0][0], mx = range[1][0];
#pragma unroll
    for (int w = 1; w < SP_WAVES; ++w) {
      mn = range[0][w] < mn ? range[0][w] : mn;
      mx = range[1][w] > mx ? range[1][w] : mx;
    }
    const int m = n - base < SP_TILE ? n - base : SP_TILE;
    bool live[NB], any = false;
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      live[k] = own[k] && !(mn - E[k] > margin || E[k] - mx > margin);
      any = any || live[k];
    }
    if (any) {
      for (int j = 0; j < m; ++j) {
        const double ecj = tile_e[j], wj = tile_w[j];
#pragma unroll
        for (int k = 0; k < NB; ++k) {
          if (live[k]) {
            const double x = (E[k] - ecj) / sigma;
            if (fabs(x) <= cutoff) acc[k] += wj * exp(-0.5 * (x * x));
          }
        }
      }
    }
    __syncthreads();                              // the tile and range[] are rewritten by the next round
  }
#pragma unroll
  for (int k = 0; k < NB; ++k)
    if (own[k]) row[tid + k * SP_THREADS] = acc[k];
  const int covered = curve ? (int)(e[0] - shift <= E_first && e[n - 1] - shift >= E_last) : 1;   // (a curve has n >= 2)
  sp_finish(o, c, S, d.de, row, cnt, stat, n_inside, bad, unsorted, covered, curve);
}

__global__ __launch_bounds__(SP_THREADS) void spectra_interp_kernel(const DosxSpectraInterp d) {
  __shared__ double row[SP_MAX_BINS];
  __shared__ double stat[1];
  __shared__ int cnt[3 * SP_WAVES];
  const int c = blockIdx.x, tid = threadIdx.x;
  const int S = d.S;
  const SpOut o{d.y, d.y_max, d.area, d.y_norm, d.report};
  const int a0 = d.ptr[c], a1 = d.ptr[c + 1];
  if (!sp_range_ok(a0, a1, d.T, d.n_min, d.n_max)) {
    sp_reject(o, c, S);
    return;
  }
  const int n = a1 - a0;                          // >= 2: the entry point refuses n_min < 2
  const double* e = d.e + a0;
  const double* v = d.v + a0;
  const double shift = d.shift[c];
  const double E_first = sp_grid(d.e0, d.de, 0), E_last = sp_grid(d.e0, d.de, S - 1);
  int n_inside = 0, unsorted = 0;
  int bad = tid == 0 ? (int)!sp_finite(shift) : 0;
  for (int i = tid; i < n; i += SP_THREADS) {
    const double ei = e[i], vi = v[i], ec = ei - shift;
    bad += (sp_finite(ei) && sp_finite(vi)) ? 0 : 1;
    n_inside += (E_first <= ec && ec <= E_last) ? 1 : 0;
    unsorted += (i + 1 < n && e[i + 1] <= ei) ? 1 : 0;
  }
  const double ec_first = e[0] - shift, ec_last = e[n - 1] - shift;
  for (int s = tid; s < S; s += SP_THREADS) {
    const double Es = sp_grid(d.e0, d.de, s);
    double ys = 0.0;
    if (Es >= ec_first && Es <= ec_last) {
      int jl = 0, jh = n - 1;                     // ec_jl <= Es throughout; both stay inside [0, n-1] whatever the data
      while (jl < jh) {
        const int mid = (jl + jh + 1) >> 1;
        if (e[mid] - shift <= Es) jl = mid;
        else jh = mid - 1;
      }
      if (jl == n - 1) {
        ys = v[n - 1];
      } else {
        const double ecj = e[jl] - shift, ecn = e[jl + 1] - shift;
        ys = v[jl] + (v[jl + 1] - v[jl]) * ((Es - ecj) / (ecn - ecj));
      }
    }
    row[s] = ys;
  }
  const int covered = (int)(ec_first <= E_first && ec_last >= E_last);
  sp_finish(o, c, S, d.de, row, cnt, stat, n_inside, bad, unsorted, covered, true);
}

template <class D>
int sp_validate(const D* d, const char* who, int n_least) {
  DOSX_CHECK_ARG(d, "%s: null descriptor", who);
  DOSX_CHECK_ARG(d->C > 0 && d->T >= 0, "%s: bad sizes C=%d T=%d", who, d->C, d->T);
  DOSX_CHECK_ARG(d->S >= 1 && d->S <= SP_MAX_BINS, "%s: S=%d outside [1, %d]", who, d->S, SP_MAX_BINS);
  DOSX_CHECK_ARG(std::isfinite(d->e0) && std::isfinite(d->de), "%s: the grid must be finite (e0=%g de=%g)", who, d->e0, d->de);
  DOSX_CHECK_ARG(d->de > 0.0 || d->S == 1, "%s: de must be positive (de=%g with S=%d)", who, d->de, d->S);
  DOSX_CHECK_ARG(d->n_min >= 0, "%s: n_min=%d is negative", who, d->n_min);
  DOSX_CHECK_ARG(d->n_min >= n_least, "%s: a curve needs two samples (n_min=%d)", who, d->n_min);
  DOSX_CHECK_ARG(d->n_max >= d->n_min && d->n_max < (1 << 20), "%s: n_max=%d outside [n_min=%d, 2^20)", who, d->n_max, d->n_min);
#define SP_NEED(field) DOSX_CHECK_ARG(d->field, "%s: null %s", who, #field)
  SP_NEED(ptr);
  SP_NEED(shift);
  if (d->T > 0) {
    SP_NEED(e);
    SP_NEED(v);
  }
  SP_NEED(y);
  SP_NEED(y_max);
  SP_NEED(area);
  SP_NEED(report);
  return 0;
}

}  // namespace

extern "C" int dosx_spectra_broaden(const DosxSpectra* d, dosx_stream_t stream) {
  const char* who = "dosx_spectra_broaden";
  DOSX_CHECK_ARG(d, "%s: null descriptor", who);
  DOSX_CHECK_ARG(d->kind == DOSX_SPECTRA_POINTS || d->kind == DOSX_SPECTRA_CURVE, "%s: unknown kind=%d", who, d->kind);
  if (int rc = sp_validate(d, who, d->kind == DOSX_SPECTRA_CURVE ? 2 : 0)) return rc;
  DOSX_CHECK_ARG(d->cutoff > 0.0 && std::isfinite(d->cutoff), "%s: cutoff must be positive and finite (%g)", who, d->cutoff);
  SP_NEED(sigma);
  const dim3 grid((unsigned)d->C), block(SP_THREADS);
  switch ((d->S + SP_THREADS - 1) / SP_THREADS) {
    case 1: spectra_broaden_kernel<1><<<grid, block, 0, to_stream(stream)>>>(*d); break;
    case 2: spectra_broaden_kernel<2><<<grid, block, 0, to_stream(stream)>>>(*d); break;
    case 3: spectra_broaden_kernel<3><<<grid, block, 0, to_stream(stream)>>>(*d); break;
    default: spectra_broaden_kernel<4><<<grid, block, 0, to_stream(stream)>>>(*d); break;
  }
  DOSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int dosx_spectra_interp(const DosxSpectraInterp* d, dosx_stream_t stream) {
  if (int rc = sp_validate(d, "dosx_spectra_interp", 2)) return rc;
  spectra_interp_kernel<<<(unsigned)d->C, SP_THREADS, 0, to_stream(stream)>>>(*d);
  DOSX_LAUNCH_CHECK();
  return 0;
}
