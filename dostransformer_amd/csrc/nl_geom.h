// Lattice geometry shared by the two periodic neighbour searches (neighbors.hip: every pair inside a cutoff; knn.hip: the K
// nearest inside a radius).  Both are compared bit-for-bit with numpy restatements, so the arithmetic lives here once:
// the inverse cell, the per-axis reach of a cutoff in shifts, and the difference vector in the reference's summation order.
#pragma once

// no fused multiply-adds in anything that includes this header (plain operators below, NOT __dmul_rn / __dadd_rn: the HIP
// header versions of those are compiled with contraction allowed and fuse after inlining)
#pragma clang fp contract(off)

namespace {

struct NlGeom {
  double L[9];      // lattice rows
  double G[9];      // inverse (columns g_k = G[.][k])
  double R[3];      // cutoff * |g_k|
};

__device__ __forceinline__ void nl_geometry(const double* __restrict__ cell, double cutoff, NlGeom& q) {
#pragma unroll
  for (int k = 0; k < 9; ++k) q.L[k] = cell[k];
  const double* L = q.L;
  const double c00 = L[4] * L[8] - L[5] * L[7], c01 = L[5] * L[6] - L[3] * L[8], c02 = L[3] * L[7] - L[4] * L[6];
  const double det = L[0] * c00 + L[1] * c01 + L[2] * c02;
  const double id = 1.0 / det;
  q.G[0] = c00 * id; q.G[1] = (L[2] * L[7] - L[1] * L[8]) * id; q.G[2] = (L[1] * L[5] - L[2] * L[4]) * id;
  q.G[3] = c01 * id; q.G[4] = (L[0] * L[8] - L[2] * L[6]) * id; q.G[5] = (L[2] * L[3] - L[0] * L[5]) * id;
  q.G[6] = c02 * id; q.G[7] = (L[1] * L[6] - L[0] * L[7]) * id; q.G[8] = (L[0] * L[4] - L[1] * L[3]) * id;
#pragma unroll
  for (int k = 0; k < 3; ++k)
    q.R[k] = cutoff * sqrt(q.G[k] * q.G[k] + q.G[3 + k] * q.G[3 + k] + q.G[6 + k] * q.G[6 + k]);
}

// d = (pos_j - pos_i) + ((s0*L0 + s1*L1) + s2*L2), no contraction: the reference's (and the oracle's) rounding
__device__ __forceinline__ void nl_vec(const double* dp, const double* L, int s0, int s1, int s2, double* d) {
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double sh = ((double)s0 * L[a] + (double)s1 * L[3 + a]) + (double)s2 * L[6 + a];
    d[a] = dp[a] + sh;
  }
}

}  // namespace
