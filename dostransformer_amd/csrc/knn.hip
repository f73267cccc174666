// K nearest periodic neighbours of every atom of a set of crystals, with their Gaussian distance features: the graph-building
// step of the Electron-DOS data path, `data/mat2graph.py:120-243` (pymatgen's `get_all_neighbors(radius)` sorted by distance and
// cut at max_num_nbr = 12, `:193,216-232`, then GaussianDistance.expand, `:162-179`).  pymatgen is not in the tree and not
// pinned; its documented behaviour is restated in include/dosx.h (DosxKnn), where the order inside a distance tie is fixed.
//
// Work decomposition: one wavefront per central atom i.  For every atom j of the crystal the wave walks the minimal integer
// shift box of the pair (the box of neighbors.hip, same arithmetic: nl_geom.h), its 64 lanes striding over the flattened box;
// the three shift digits advance by a mixed-radix add of 64, so the walk has no division.  A candidate is a key
// (r2 bits, j | biased shifts): two unsigned 64-bit words that compare like (r2, j, S0, S1, S2) because r2 >= 0.  Every lane
// keeps the KB <= 16 smallest keys it met as a sorted list in registers (KB is a template bound, insertion is an unrolled
// chain of selects: no runtime-indexed array, no scratch).  K rounds of a wave-wide minimum over the list heads (xor butterfly)
// then pop the winner one by one; lane r keeps the winner of round r and writes rank r.  Nothing depends on how lanes are
// scheduled and there are no atomics: the K keys are the K smallest of a set, whichever lane met them.  Only the N*K kept
// edges (and their G features) are ever written.
#include "common.h"
#include "nl_geom.h"

// membership, ranking and the features are compared bit-for-bit with a numpy restatement: no fused multiply-adds in this file
#pragma clang fp contract(off)

namespace {

constexpr int KNN_WAVES = 4;                      // central atoms per workgroup
constexpr int KNN_BIAS = 1024;                    // shifts are kept as 11-bit biased digits: |S_k| <= 1023
constexpr unsigned long long KNN_EMPTY = ~0ull;   // r2 word of an empty list slot: above the bits of every finite r2

typedef unsigned long long knn_u64;

// (r, t) < (br, bt) as a pair of unsigned words.  Keys travel as two scalars, never as a struct: a select between two struct
// lvalues is a select between addresses and sends the list to scratch.
__device__ __forceinline__ bool knn_lt(knn_u64 r, knn_u64 t, knn_u64 br, knn_u64 bt) { return r < br || (r == br && t < bt); }

template <int KB>
__global__ __launch_bounds__(64 * KNN_WAVES) void knn_graph_kernel(const DosxKnn d) {
  const int lane = threadIdx.x & 63;
  const int ig = (int)blockIdx.x * KNN_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (ig >= d.N) return;                          // the whole wave leaves: no workgroup barrier below
  int c = 0;
  for (int hi = d.C; hi - c > 1;) {               // last c with atom_ptr[c] <= ig (empty crystals own no atom)
    const int mid = (c + hi) >> 1;
    if (d.atom_ptr[mid] <= ig) c = mid; else hi = mid;
  }
  const int a0 = d.atom_ptr[c], n = d.atom_ptr[c + 1] - a0;
  NlGeom q;
  nl_geometry(d.cell + (size_t)c * 9, d.radius, q);
  const double rc2 = d.radius * d.radius, tol2 = d.tol * d.tol;
  double pi[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) pi[a] = d.pos[(size_t)ig * 3 + a];

  knn_u64 br[KB], bt[KB];                         // this lane's KB smallest keys, ascending
#pragma unroll
  for (int t = 0; t < KB; ++t) br[t] = KNN_EMPTY, bt[t] = 0;

  for (int j = 0; j < n; ++j) {
    double dp[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) dp[a] = d.pos[(size_t)(a0 + j) * 3 + a] - pi[a];
    int lo[3], cnt[3];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      lo[k] = 0, cnt[k] = 1;
      if ((d.pbc_mask >> k) & 1) {
        const double f = dp[0] * q.G[k] + dp[1] * q.G[3 + k] + dp[2] * q.G[6 + k];
        // one extra shift either side: the box bound is evaluated in floating point, the membership test below is exact
        const double l = ceil(-f - q.R[k]) - 1.0, h = floor(-f + q.R[k]) + 1.0;
        ok = ok && l >= -(double)(KNN_BIAS - 1) && h <= (double)(KNN_BIAS - 1) && h >= l;   // false for a NaN (singular cell)
        if (ok) lo[k] = (int)l, cnt[k] = (int)h - (int)l + 1;
      }
    }
    if (!ok) continue;                            // wave-uniform: a box past the 11-bit digits holds no candidate
    // lane -> (s0, s1, s2) digits of its first box cell, and the digits of the stride 64
    const int n1 = cnt[1], n2 = cnt[2];
    int t0 = lane / n2;
    int s2 = lane - t0 * n2, s0 = t0 / n1;
    int s1 = t0 - s0 * n1;
    const int u0 = 64 / n2;
    const int a2 = 64 - u0 * n2, a0s = u0 / n1;
    const int a1 = u0 - a0s * n1;
    const unsigned long long jbits = (unsigned long long)j << 33;
    while (s0 < cnt[0]) {
      const int S0 = lo[0] + s0, S1 = lo[1] + s1, S2 = lo[2] + s2;
      double v[3];
      nl_vec(dp, q.L, S0, S1, S2, v);
      const double r2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
      if (r2 > tol2 && r2 <= rc2) {
        const knn_u64 kr = (knn_u64)__double_as_longlong(r2);
        const knn_u64 kt = jbits | (knn_u64)(S0 + KNN_BIAS) << 22 | (knn_u64)(S1 + KNN_BIAS) << 11 | (knn_u64)(S2 + KNN_BIAS);
        if (knn_lt(kr, kt, br[KB - 1], bt[KB - 1])) {
#pragma unroll
          for (int t = KB - 1; t >= 1; --t) {     // slot t-1 still holds its old entry when slot t is rewritten
            const bool up = knn_lt(kr, kt, br[t - 1], bt[t - 1]), here = knn_lt(kr, kt, br[t], bt[t]);
            br[t] = up ? br[t - 1] : (here ? kr : br[t]);
            bt[t] = up ? bt[t - 1] : (here ? kt : bt[t]);
          }
          if (knn_lt(kr, kt, br[0], bt[0])) br[0] = kr, bt[0] = kt;
        }
      }
      s2 += a2;
      if (s2 >= n2) s2 -= n2, ++s1;
      s1 += a1;
      if (s1 >= n1) s1 -= n1, ++s0;
      s0 += a0s;
    }
  }

  // K rounds: the smallest head of the 64 lists wins, its lane pops it.  Keys are distinct (one per (j, S)), so there is one winner.
  const int K = d.K;
  knn_u64 mine_r = KNN_EMPTY, mine_t = 0;
  int count = 0;
  for (int r = 0; r < K; ++r) {
    knn_u64 mr = br[0], mt = bt[0];
#pragma unroll
    for (int x = 32; x >= 1; x >>= 1) {
      const knn_u64 orr = __shfl_xor(mr, x), ot = __shfl_xor(mt, x);
      const bool less = knn_lt(orr, ot, mr, mt);
      mr = less ? orr : mr, mt = less ? ot : mt;
    }
    if ((unsigned)__builtin_amdgcn_readfirstlane((int)(mr >> 32)) == 0xffffffffu) break;   // every list is empty
    if (lane == r) mine_r = mr, mine_t = mt;
    const bool win = br[0] == mr && bt[0] == mt;
#pragma unroll
    for (int t = 0; t < KB - 1; ++t) br[t] = win ? br[t + 1] : br[t], bt[t] = win ? bt[t + 1] : bt[t];
    br[KB - 1] = win ? KNN_EMPTY : br[KB - 1];
    ++count;
  }

  const bool real = lane < count;
  const double dist = real ? sqrt(__longlong_as_double((long long)mine_r)) : d.pad_dist;
  if (lane < K) {
    const size_t o = (size_t)ig * K + lane;
    d.nbr_idx[o] = real ? (int)(mine_t >> 33) : 0;
    d.nbr_shift[o * 3 + 0] = real ? (int)((mine_t >> 22) & 2047) - KNN_BIAS : 0;
    d.nbr_shift[o * 3 + 1] = real ? (int)((mine_t >> 11) & 2047) - KNN_BIAS : 0;
    d.nbr_shift[o * 3 + 2] = real ? (int)(mine_t & 2047) - KNN_BIAS : 0;
    d.nbr_dist[o] = dist;
  }
  if (lane == 0) d.nbr_count[ig] = count;

  if (d.edge_attr) {                              // exp(-(d - mu_g)^2 / var^2) of the K ranks, padded ranks included
    const int G = d.G, tot = K * G;
    const double v2 = d.var * d.var;
    float* out = d.edge_attr + (size_t)ig * K * G;
    for (int e0 = 0; e0 < tot; e0 += 64) {        // every lane stays in the loop: the shuffle reads lanes 0..K-1
      const int e = e0 + lane;
      const int rk = (e < tot ? e : tot - 1) / G;
      const double dd = __shfl(dist, rk);
      if (e < tot) {
        const double t = dd - d.centers[e - rk * G];
        out[e] = (float)exp(-(t * t) / v2);
      }
    }
  }
}

}  // namespace

extern "C" int dosx_knn_graph(const DosxKnn* d, dosx_stream_t stream) {
  DOSX_CHECK_ARG(d, "dosx_knn_graph: null descriptor");
  DOSX_CHECK_ARG(d->C > 0 && d->N >= 0, "dosx_knn_graph: bad sizes C=%d N=%d", d->C, d->N);
  DOSX_CHECK_ARG(d->K >= 1 && d->K <= 16, "dosx_knn_graph: K=%d outside [1, 16]", d->K);
  DOSX_CHECK_ARG((long long)d->N * d->K < (1ll << 31), "dosx_knn_graph: N*K = %lld needs 32-bit edge indices",
                 (long long)d->N * d->K);
  DOSX_CHECK_ARG(d->radius > 0.0, "dosx_knn_graph: radius must be positive (%g)", d->radius);
  DOSX_CHECK_ARG(d->tol >= 0.0, "dosx_knn_graph: tol must not be negative (%g)", d->tol);
  DOSX_CHECK_ARG(d->pos && d->cell && d->atom_ptr, "dosx_knn_graph: null input");
  DOSX_CHECK_ARG(d->nbr_idx && d->nbr_shift && d->nbr_dist && d->nbr_count, "dosx_knn_graph: null output");
  if (d->edge_attr) {
    DOSX_CHECK_ARG(d->G >= 1 && (long long)d->K * d->G < (1ll << 31), "dosx_knn_graph: bad feature width G=%d", d->G);
    DOSX_CHECK_ARG(d->centers, "dosx_knn_graph: null centers");
    DOSX_CHECK_ARG(d->var > 0.0, "dosx_knn_graph: var must be positive (%g)", d->var);
  }
  if (d->N == 0) return 0;
  const unsigned grid = (unsigned)((d->N + KNN_WAVES - 1) / KNN_WAVES);
  hipStream_t s = to_stream(stream);
  if (d->K <= 4) knn_graph_kernel<4><<<grid, 64 * KNN_WAVES, 0, s>>>(*d);
  else if (d->K <= 8) knn_graph_kernel<8><<<grid, 64 * KNN_WAVES, 0, s>>>(*d);
  else if (d->K <= 12) knn_graph_kernel<12><<<grid, 64 * KNN_WAVES, 0, s>>>(*d);
  else knn_graph_kernel<16><<<grid, 64 * KNN_WAVES, 0, s>>>(*d);
  DOSX_LAUNCH_CHECK();
  return 0;
}
