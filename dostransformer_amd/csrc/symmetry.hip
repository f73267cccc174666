// The crystal system of every crystal of a dataset from its structure: pure translations (dosx_sym_translations) and the point
// group of the reduced primitive cell (dosx_sym_point_group).  The definition - distances, reference atom, lattice and structure
// operations, the trace histogram and its eleven point groups - is the contract in include/dosx.h (DosxSymTranslations,
// DosxSymPointGroup); the numpy twin is dostransformer_amd/symmetry.py.
//
// Work decomposition: one workgroup of 256 lanes (4 waves) per crystal.  Coordinates and species are staged in LDS when the
// crystal has at most SYM_LDS_ATOMS atoms and read from global memory beyond that (same code, a flat pointer either way).
//   translations   the waves stride over the candidate atoms j; a wave's lanes stride over the atoms i, each lane searches its
//                  image k; the wave leaves a candidate at the first 64 atoms with a miss.
//   lattice ops    the 27 candidate rows of each basis vector are filtered by length first (81 lanes), the surviving triples are
//                  walked in lexicographic order 256 at a time, tested for determinant and face diagonals and compacted in that
//                  order by ballots and a per-wave count in LDS.
//   structure ops  the waves stride over the lattice operations; a wave tries the candidate translations in atom order and stops
//                  at the first that maps every atom.
//   classification one wave: ballots over its <= 48 lanes.
// No atomics, no dependence on scheduling; every store is a plain vector store.
#include "common.h"

// decisions are compared with the numpy twin: no fused multiply-adds in this file (see nl_geom.h)
#pragma clang fp contract(off)

namespace {

constexpr int SYM_THREADS = 256;
constexpr int SYM_WAVES = SYM_THREADS / 64;
constexpr int SYM_LDS_ATOMS = 1024;               // staging limit: 28 bytes per atom
constexpr int SYM_MAX_OPS = 48;
constexpr int SYM_INCONSISTENT = 7;
constexpr int SYM_POW3[9] = {1, 3, 9, 27, 81, 243, 729, 2187, 6561};

typedef unsigned long long sym_u64;

// N2, N3, N4, N6, order, crystal-system code of the eleven proper point groups (include/dosx.h)
__constant__ int SYM_GROUPS[11][6] = {
    {0, 0, 0, 0, 1, 6}, {1, 0, 0, 0, 2, 5}, {3, 0, 0, 0, 4, 4}, {1, 0, 2, 0, 4, 2}, {5, 0, 2, 0, 8, 2}, {0, 2, 0, 0, 3, 3},
    {3, 2, 0, 0, 6, 3}, {1, 2, 0, 2, 6, 1}, {7, 2, 0, 2, 12, 1}, {3, 8, 0, 0, 12, 0}, {9, 8, 6, 0, 24, 0}};

struct SymCrystal {
  const double* x;     // [n][3] fractional rows (LDS or global)
  const int* z;        // [n]
  int n;
  double A[9];
  double s2;           // symprec^2
};

extern __shared__ double sym_stage[];             // [cap][3] doubles, then [cap] ints

// Loads crystal c; false (for the whole workgroup) when it is outside [1, n_max].  Ends with a barrier when it staged.
__device__ __forceinline__ bool sym_load(const double* cell, const double* frac, const int* species, const int* atom_ptr, int c,
                                         int n_max, int cap, double symprec, SymCrystal& q) {
  const int a0 = atom_ptr[c];
  q.n = atom_ptr[c + 1] - a0;
  if (q.n < 1 || q.n > n_max) return false;
#pragma unroll
  for (int k = 0; k < 9; ++k) q.A[k] = cell[(size_t)c * 9 + k];
  q.s2 = symprec * symprec;
  q.x = frac + (size_t)a0 * 3;
  q.z = species + a0;
  if (q.n <= cap) {
    int* sz = reinterpret_cast<int*>(sym_stage + (size_t)cap * 3);
    for (int e = threadIdx.x; e < q.n * 3; e += SYM_THREADS) sym_stage[e] = q.x[e];
    for (int e = threadIdx.x; e < q.n; e += SYM_THREADS) sz[e] = q.z[e];
    __syncthreads();
    q.x = sym_stage;
    q.z = sz;
  }
  return true;
}

// First atom of the rarest species, ties to the smallest species number: the minimum of (count, species, atom) over the atoms.
__device__ __forceinline__ int sym_reference(const SymCrystal& q, sym_u64* red) {
  sym_u64 key = ~0ull;
  for (int i = threadIdx.x; i < q.n; i += SYM_THREADS) {
    const int zi = q.z[i];
    int cnt = 0;
    for (int k = 0; k < q.n; ++k) cnt += q.z[k] == zi;
    const sym_u64 mine = (sym_u64)cnt << 42 | (sym_u64)zi << 21 | (sym_u64)i;
    key = mine < key ? mine : key;
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const sym_u64 o = __shfl_xor(key, s);
    key = o < key ? o : key;
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = key;
  __syncthreads();
  key = red[0];
#pragma unroll
  for (int w = 1; w < SYM_WAVES; ++w) key = red[w] < key ? red[w] : key;
  return (int)(key & ((1u << 21) - 1));
}

// Does the moved atom y of species zy land on an atom of its species?
__device__ __forceinline__ bool sym_lands(const SymCrystal& q, double y0, double y1, double y2, int zy) {
  for (int k = 0; k < q.n; ++k) {
    if (q.z[k] != zy) continue;
    double d0 = y0 - q.x[k * 3 + 0], d1 = y1 - q.x[k * 3 + 1], d2 = y2 - q.x[k * 3 + 2];
    d0 -= rint(d0), d1 -= rint(d1), d2 -= rint(d2);
    const double c0 = (d0 * q.A[0] + d1 * q.A[3]) + d2 * q.A[6];
    const double c1 = (d0 * q.A[1] + d1 * q.A[4]) + d2 * q.A[7];
    const double c2 = (d0 * q.A[2] + d1 * q.A[5]) + d2 * q.A[8];
    if ((c0 * c0 + c1 * c1) + c2 * c2 < q.s2) return true;
  }
  return false;
}

// Wave-wide: does y_i = ((x_i0*W0 + x_i1*W1) + x_i2*W2) + t land for every atom i?  (identity: y_i = x_i + t)
template <bool IDENTITY>
__device__ __forceinline__ bool sym_maps_all(const SymCrystal& q, const double* W, const double* t) {
  const int lane = threadIdx.x & 63;
  for (int i0 = 0; i0 < q.n; i0 += 64) {
    const int i = i0 + lane;
    bool miss = false;
    if (i < q.n) {
      const double x0 = q.x[i * 3 + 0], x1 = q.x[i * 3 + 1], x2 = q.x[i * 3 + 2];
      double y[3];
#pragma unroll
      for (int a = 0; a < 3; ++a)
        y[a] = IDENTITY ? (a == 0 ? x0 : a == 1 ? x1 : x2) + t[a] : ((x0 * W[a] + x1 * W[3 + a]) + x2 * W[6 + a]) + t[a];
      miss = !sym_lands(q, y[0], y[1], y[2], q.z[i]);
    }
    if (__ballot(miss) != 0ull) return false;
  }
  return true;
}

__global__ __launch_bounds__(SYM_THREADS) void sym_translations_kernel(const DosxSymTranslations d, int cap) {
  __shared__ sym_u64 red[SYM_WAVES];
  const int c = blockIdx.x;
  SymCrystal q;
  if (!sym_load(d.cell, d.frac, d.species, d.atom_ptr, c, d.n_max, cap, d.symprec, q)) return;
  const int ref = sym_reference(q, red);
  const int zref = q.z[ref];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  unsigned char* flag = static_cast<unsigned char*>(d.flag) + d.atom_ptr[c];
  for (int j = wave; j < q.n; j += SYM_WAVES) {
    bool is = false;
    if (j != ref && q.z[j] == zref) {
      double t[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) t[a] = q.x[j * 3 + a] - q.x[ref * 3 + a];
      is = sym_maps_all<true>(q, nullptr, t);
    }
    if (lane == 0) flag[j] = is ? 1 : 0;
  }
}

__device__ __forceinline__ double sym_len(double v0, double v1, double v2) { return sqrt((v0 * v0 + v1 * v1) + v2 * v2); }

// row r in 0..26 -> digits (w0, w1, w2) in {-1, 0, 1}, first digit slowest: ascending r is lexicographic order
__device__ __forceinline__ void sym_row(int r, int* w) { w[0] = r / 9 - 1, w[1] = (r / 3) % 3 - 1, w[2] = r % 3 - 1; }

__device__ __forceinline__ void sym_image(const double* A, const int* w, double* v) {
#pragma unroll
  for (int a = 0; a < 3; ++a) v[a] = ((double)w[0] * A[a] + (double)w[1] * A[3 + a]) + (double)w[2] * A[6 + a];
}

__global__ __launch_bounds__(SYM_THREADS) void sym_point_group_kernel(const DosxSymPointGroup d, int cap) {
  __shared__ sym_u64 red[SYM_WAVES];
  __shared__ int row_ok[81];
  __shared__ int row_list[3][27], row_cnt[3];
  __shared__ int wave_cnt[SYM_WAVES];
  __shared__ int lat[SYM_MAX_OPS];               // lattice operations as 0..19682 = the nine digits in base 3
  __shared__ int kept[SYM_MAX_OPS];
  const int c = blockIdx.x, tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  SymCrystal q;
  if (!sym_load(d.cell, d.frac, d.species, d.atom_ptr, c, d.n_max, cap, d.symprec, q)) return;
  const int ref = sym_reference(q, red);
  const int zref = q.z[ref];
  const double* A = q.A;

  // (c) rows that keep the length of their basis vector
  if (tid < 81) {
    const int i = tid / 27;
    int w[3];
    double v[3];
    sym_row(tid - i * 27, w);
    sym_image(A, w, v);
    const double own = i == 0 ? sym_len(A[0], A[1], A[2]) : i == 1 ? sym_len(A[3], A[4], A[5]) : sym_len(A[6], A[7], A[8]);
    row_ok[tid] = fabs(sym_len(v[0], v[1], v[2]) - own) < d.symprec;     // (no runtime index into A: it stays in registers)
  }
  __syncthreads();
  if (tid < 3) {
    int m = 0;
    for (int r = 0; r < 27; ++r)
      if (row_ok[tid * 27 + r]) row_list[tid][m++] = r;
    row_cnt[tid] = m;
  }
  __syncthreads();
  const int n0 = row_cnt[0], n1 = row_cnt[1], n2 = row_cnt[2];
  const int total = n0 * n1 * n2;                 // <= 19683
  const double l01 = sym_len(A[0] + A[3], A[1] + A[4], A[2] + A[5]), l02 = sym_len(A[0] + A[6], A[1] + A[7], A[2] + A[8]),
               l12 = sym_len(A[3] + A[6], A[4] + A[7], A[5] + A[8]);
  int n_lat = 0;
  for (int base = 0; base < total; base += SYM_THREADS) {      // workgroup-uniform trip count
    const int t = base + tid;
    bool pass = false;
    int code = 0;
    if (t < total) {
      const int p0 = t / (n1 * n2), p1 = (t / n2) % n1, p2 = t % n2;
      const int r0 = row_list[0][p0], r1 = row_list[1][p1], r2 = row_list[2][p2];
      int w0[3], w1[3], w2[3];
      sym_row(r0, w0), sym_row(r1, w1), sym_row(r2, w2);
      const int det = w0[0] * (w1[1] * w2[2] - w1[2] * w2[1]) - w0[1] * (w1[0] * w2[2] - w1[2] * w2[0]) +
                      w0[2] * (w1[0] * w2[1] - w1[1] * w2[0]);
      if (det == 1 || det == -1) {
        double v0[3], v1[3], v2[3];
        sym_image(A, w0, v0), sym_image(A, w1, v1), sym_image(A, w2, v2);
        pass = fabs(sym_len(v0[0] + v1[0], v0[1] + v1[1], v0[2] + v1[2]) - l01) < d.symprec &&
               fabs(sym_len(v0[0] + v2[0], v0[1] + v2[1], v0[2] + v2[2]) - l02) < d.symprec &&
               fabs(sym_len(v1[0] + v2[0], v1[1] + v2[1], v1[2] + v2[2]) - l12) < d.symprec;
      }
      code = (r0 * 27 + r1) * 27 + r2;
    }
    const sym_u64 b = __ballot(pass);
    if (lane == 0) wave_cnt[wave] = __popcll(b);
    __syncthreads();
    int off = n_lat, all = 0;
#pragma unroll
    for (int w = 0; w < SYM_WAVES; ++w) {
      off += w < wave ? wave_cnt[w] : 0;
      all += wave_cnt[w];
    }
    off += __popcll(b & ((1ull << lane) - 1ull));
    if (pass && off < SYM_MAX_OPS) lat[off] = code;
    n_lat += all;
    __syncthreads();                              // wave_cnt is rewritten by the next round; lat is read below
  }

  signed char* ops = static_cast<signed char*>(d.ops) + (size_t)c * SYM_MAX_OPS * 9;
  if (n_lat > SYM_MAX_OPS) {                      // no lattice has more than 48 operations: nothing is kept
    for (int e = tid; e < SYM_MAX_OPS * 9; e += SYM_THREADS) ops[e] = 0;
    if (tid < 5) d.hist[(size_t)c * 5 + tid] = 0;
    if (tid == 0) d.n_lattice_ops[c] = n_lat, d.n_ops[c] = 0, d.code[c] = SYM_INCONSISTENT;
    return;
  }

  // (d) structure operations: lattice operation o is kept when some candidate translation maps every atom
  for (int o = wave; o < n_lat; o += SYM_WAVES) {
    double W[9], xw[3];
    const int v = lat[o];
#pragma unroll
    for (int e = 0; e < 9; ++e) W[e] = (double)(v / SYM_POW3[8 - e] % 3 - 1);
#pragma unroll
    for (int a = 0; a < 3; ++a) xw[a] = (q.x[ref * 3] * W[a] + q.x[ref * 3 + 1] * W[3 + a]) + q.x[ref * 3 + 2] * W[6 + a];
    bool found = false;
    for (int j = 0; j < q.n && !found; ++j) {
      if (q.z[j] != zref) continue;
      double t[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) t[a] = q.x[j * 3 + a] - xw[a];
      found = sym_maps_all<false>(q, W, t);
    }
    if (lane == 0) kept[o] = found;
  }
  __syncthreads();
  if (tid >= 64) return;

  // (e) one wave: compaction of the kept operations, distinct proper parts, trace histogram, point group
  const bool k = lane < n_lat && kept[lane];
  const sym_u64 kb = __ballot(k);
  const int n_ops = __popcll(kb), pos = __popcll(kb & ((1ull << lane) - 1ull));
  const int v = lane < n_lat ? lat[lane] : 0;
  int W[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) W[e] = v / SYM_POW3[8 - e] % 3 - 1;
  if (k) {
#pragma unroll
    for (int e = 0; e < 9; ++e) ops[pos * 9 + e] = (signed char)W[e];
  }
  if (lane < SYM_MAX_OPS && lane >= n_ops) {
#pragma unroll
    for (int e = 0; e < 9; ++e) ops[lane * 9 + e] = 0;
  }
  const int det = W[0] * (W[4] * W[8] - W[5] * W[7]) - W[1] * (W[3] * W[8] - W[5] * W[6]) + W[2] * (W[3] * W[7] - W[4] * W[6]);
  int pcode = 0;
#pragma unroll
  for (int e = 0; e < 9; ++e) pcode = pcode * 3 + (det * W[e] + 1);
  pcode = k ? pcode : -1;
  bool dup = false;
  for (int l = 0; l < SYM_MAX_OPS; ++l) {         // every lane stays in the loop: the shuffle reads lanes 0..47
    const int other = __shfl(pcode, l);
    dup = dup || (l < lane && other == pcode);
  }
  const bool uniq = k && !dup;
  const int trace = det * (W[0] + W[4] + W[8]);
  int h[5];
#pragma unroll
  for (int b = 0; b < 5; ++b) h[b] = __popcll(__ballot(uniq && trace == b - 1));
  const int n_proper = __popcll(__ballot(uniq));
  if (lane == 0) {
    int code = SYM_INCONSISTENT;
    for (int g = 0; g < 11; ++g) {
      const int* G = SYM_GROUPS[g];
      if (h[0] == G[0] && h[1] == G[1] && h[2] == G[2] && h[3] == G[3] && h[4] == 1 && n_proper == G[4] &&
          (n_ops == G[4] || n_ops == 2 * G[4]))
        code = G[5];
    }
#pragma unroll
    for (int b = 0; b < 5; ++b) d.hist[(size_t)c * 5 + b] = h[b];
    d.n_lattice_ops[c] = n_lat, d.n_ops[c] = n_ops, d.code[c] = code;
  }
}

template <class D>
int sym_validate(const D* d, const char* who) {
  DOSX_CHECK_ARG(d, "%s: null descriptor", who);
  DOSX_CHECK_ARG(d->C > 0 && d->N > 0, "%s: bad sizes C=%d N=%d", who, d->C, d->N);
  DOSX_CHECK_ARG(d->n_min > 0, "%s: an empty crystal (n_min=%d)", who, d->n_min);
  DOSX_CHECK_ARG(d->n_max >= d->n_min && d->n_max < (1 << 21), "%s: n_max=%d outside [n_min=%d, 2^21)", who, d->n_max, d->n_min);
  DOSX_CHECK_ARG(d->symprec > 0.0, "%s: symprec must be positive (%g)", who, d->symprec);
  DOSX_CHECK_ARG(d->cell && d->frac && d->species && d->atom_ptr, "%s: null input", who);
  return 0;
}

inline int sym_cap(int n_max) { return n_max < SYM_LDS_ATOMS ? n_max : SYM_LDS_ATOMS; }
inline size_t sym_lds_bytes(int cap) { return (size_t)cap * (3 * sizeof(double) + sizeof(int)); }

}  // namespace

extern "C" int dosx_sym_translations(const DosxSymTranslations* d, dosx_stream_t stream) {
  if (int rc = sym_validate(d, "dosx_sym_translations")) return rc;
  DOSX_CHECK_ARG(d->flag, "dosx_sym_translations: null output");
  const int cap = sym_cap(d->n_max);
  sym_translations_kernel<<<(unsigned)d->C, SYM_THREADS, sym_lds_bytes(cap), to_stream(stream)>>>(*d, cap);
  DOSX_LAUNCH_CHECK();
  return 0;
}

extern "C" int dosx_sym_point_group(const DosxSymPointGroup* d, dosx_stream_t stream) {
  if (int rc = sym_validate(d, "dosx_sym_point_group")) return rc;
  DOSX_CHECK_ARG(d->n_lattice_ops && d->n_ops && d->ops && d->hist && d->code, "dosx_sym_point_group: null output");
  const int cap = sym_cap(d->n_max);
  sym_point_group_kernel<<<(unsigned)d->C, SYM_THREADS, sym_lds_bytes(cap), to_stream(stream)>>>(*d, cap);
  DOSX_LAUNCH_CHECK();
  return 0;
}
