// Linear functionals of the DOS in the loss and in evaluation (include/dosx.h "linear functionals in the per-crystal losses" and
// "evaluation functionals"): a table fn_w [K,S] of functionals F_k(p) = sum_s fn_w[k,s] p_s - cumulative DOS, moments, windows,
// heat-capacity kernels - whose differences u_k = F_k(p_b) - F_k(t_b) are penalised next to the pointwise term of
// csrc/loss_rows.hip, and which dosx_eval_functionals evaluates in float64.
//
// dosx_loss_rows_fn / _fn_f64.  One wavefront per crystal, four crystals per 256-thread workgroup, as the pointwise kernels; the
// pointwise term is their code (loss_rows.h), summed in their order.  Lane l holds the residuals r_s = p_s - t_s of its elements
// s = l, l + 64, ..., l + 448 of both outputs in registers (S <= 512: eight per output) and, next to them, the eight gradient
// sums of the new term.  Nothing goes through LDS; the table is read from global memory ONCE per crystal, row by row, coalesced,
// four rows per trip of the k loop (their loads go out together, their wave reductions are independent chains).
// SUMMATION ORDER (the fp32 test bars are counted from it, tests/test_gpu_loss_functional.py):
//   phase 1, for k = 0 .. K - 1 in order: lane l forms  sum_j fn_w[k, l + 64 j] r_{l + 64 j}  with j rising (ceil(S / 64) products,
//            one fewer additions), and the 64 lane sums meet in one wave reduction of 6 levels (row_sum): u_k, the same number in
//            every lane.  The crystal's  sum_k e(u_k)  is added up in k order, one addition per k, in every lane alike.
//   phase 2, with the row of the table still in registers: every lane adds  e'(u_k) fn_w[k,s]  to each of its gradient sums - element
//            s receives its K terms in k order, one addition per k.
//   then    dpg[s] = (pointwise gradient) + (coef lam / K) (gradient sum), one product and one addition per element and ONE store:
//            the rows are written once, nothing is read back.  l_b = (pointwise l_b) + (lam / K) (sum_g + beta sum_s).
// Every order above depends on (S, K) alone - not on B, not on the crystal's place in the launch; no atomics.  lam / K is formed
// on the host in the operands' type, so K -> 2 K with lam -> 2 lam is the same number.  fn_kind is a wave-uniform run-time branch;
// the sample and bin weights are read through their pointers (NULL: none), not through template flags as in loss_rows.hip.
//
// dosx_loss_rows_fn_norm / _fn_norm_f64 (and their descriptor forms).  The last K_norm rows of the table are divided by one common
// denominator functional D(x) = sum_s fn_den[s] x_s, floored: u_k = F_k(p) / D+(p) - F_k(t) / D+(t).  A ratio is no function of the
// residual, so lane l holds pg, ps and t THEMSELVES (eight each), the two gradient sums and its eight elements of fn_den; the
// launch shapes, the pointwise term and its order are those above.  Kernels of their own (loss_fnn_*): the ones above are untouched.
// SUMMATION ORDER (tests/test_gpu_loss_normalised.py counts its fp32 bars from it); it depends on (S, K, K_norm) alone:
//   phase 0: lane l forms  sum_j fn_den[l + 64 j] x_{l + 64 j}  with j rising for x = pg, ps, t, one wave reduction each: D(pg),
//            D(ps), D(t);  D+ = D < den_floor ? den_floor : D  (a NaN stays a NaN).
//   plain rows k = 0 .. K - K_norm - 1: phases 1 and 2 above, with r_s = p_s - t_s formed again from the registers (the same bits).
//   normalised rows k = K - K_norm .. K - 1, in order, four per trip: lane sums of fn_w[k,s] x_s with j rising and one wave
//            reduction for each of x = pg, ps, t: F_k(pg), F_k(ps), F_k(t);  q = F_k(x) / D+(x)  (one division each),
//            u_k = q(p) - q(t);  sum_k e(u_k)  goes on in k order (behind the plain rows' terms);  c_k = e'(u_k) / D+(p)  (one
//            division);  A += c_k q_k(p)  in k order, one product and one addition;  every lane adds  c_k fn_w[k,s]  to each of
//            its gradient sums, in k order behind the plain rows' terms.
//   then    dpg[s] = (pointwise gradient) + (coef lam / K) (gradient sum - a fn_den[s]),  a = A where D(p) > den_floor, else 0
//            (a floored denominator is a constant): one product and one subtraction more than above, ONE store.
//
// dosx_eval_functionals / _f64.  One wavefront per row, float64 products and sums: for each k lane l adds the elements l, l + 64,
// ... of the row times the table's in rising order, one wave reduction (xor butterfly), lane 0 writes; any S and K.
#include "loss_rows.h"

namespace {

constexpr int FN_MAX = 512;                 // S and K of the loss entries
constexpr int FN_CHUNKS = FN_MAX / 64;      // elements of a row per lane
constexpr int FN_ROWS = 4;                  // table rows per trip of the k loop

// e(u) and e'(u): DOSX_FN_SQ u^2, 2 u;  DOSX_FN_ABS |u|, sign(u) with sign(0) = 0 (torch.sign) and a NaN staying a NaN
template <typename T>
__device__ __forceinline__ T fn_e(T u, bool abs_kind) { return abs_kind ? abs_of(u) : u * u; }
template <typename T>
__device__ __forceinline__ T fn_de(T u, bool abs_kind) {
  if (!abs_kind) return (T)2 * u;
  return u > (T)0 ? (T)1 : u < (T)0 ? (T)-1 : u == (T)0 ? (T)0 : u;
}

// lane l's elements l, l + 64, ... of one table row; 0 past S
template <typename T>
__device__ __forceinline__ void fn_load_row(T (&wv)[FN_CHUNKS], const T* __restrict__ row, int S, int lane) {
#pragma unroll
  for (int j = 0; j < FN_CHUNKS; ++j) {
    wv[j] = (T)0;
    if (64 * j < S) {                        // wave-uniform
      const int s = lane + 64 * j;
      if (s < S) wv[j] = row[s];             // (under the lane mask: a clamped straight-line load measured 1.8x slower)
    }
  }
}

template <typename T>
struct FnOperands {
  const T* fn_w;       // [K,S]
  int K;
  int abs_kind;        // fn_kind == DOSX_FN_ABS
  T lamk;              // lam / K
};

// One crystal by one wavefront: l_b of the definition, returned in every lane; the crystal's gradient rows written once.
// coef = w_b / B_global; zero: w_b == 0, the rows are +0.0 whatever the crystal holds (l_b is still formed: per_crystal reports it).
template <typename T, int KIND, bool TWO>
__device__ __forceinline__ T fn_row(const T* __restrict__ pg, const T* __restrict__ ps, const T* __restrict__ y, size_t o, int S,
                                    int lane, bool clamp, T beta, T delta, T coef, bool zero, const T* __restrict__ bin_w, T den,
                                    const FnOperands<T>& f, T* __restrict__ dpg, T* __restrict__ dps) {
  T rg[FN_CHUNKS], rs[FN_CHUNKS], gg[FN_CHUNKS], gs[FN_CHUNKS];
  // ---- the pointwise term: loss_row's sums (csrc/loss_rows.hip), the residuals kept ----------------------------------------
  T a = (T)0, c = (T)0;
#pragma unroll
  for (int j = 0; j < FN_CHUNKS; ++j) {
    rg[j] = rs[j] = gg[j] = gs[j] = (T)0;
    const int s = lane + 64 * j;
    if (s < S) {
      const T t = target_of(y[o + s], clamp);
      rg[j] = pg[o + s] - t;
      if constexpr (TWO) rs[j] = ps[o + s] - t;
      if (bin_w) {
        const T v = bin_w[s];
        if (v != (T)0) {
          a += v * elem_loss<T, KIND>(rg[j], delta);
          if constexpr (TWO) c += v * elem_loss<T, KIND>(rs[j], delta);
        }
      } else {
        a += elem_loss<T, KIND>(rg[j], delta);
        if constexpr (TWO) c += elem_loss<T, KIND>(rs[j], delta);
      }
    }
  }
  a = row_sum(a);
  if constexpr (TWO) c = row_sum(c);
  const T r0 = row_term<T, KIND>(a, den);
  const T k0 = row_coef<T, KIND>(coef, r0, den);
  T r1 = (T)0, k1 = (T)0;
  if constexpr (TWO) {
    r1 = row_term<T, KIND>(c, den);
    k1 = row_coef<T, KIND>(beta * coef, r1, den);
  }
  // ---- the functionals: u_k, e(u_k) and the gradient sums, one table row at a time ------------------------------------------
  const bool abs_kind = f.abs_kind != 0;
  T hg = (T)0, hs = (T)0;
  // FN_ROWS rows of the table per trip: their loads are issued together and their 2 FN_ROWS wave reductions are independent
  // chains the scheduler interleaves - one row per trip is one load latency and two dependent reductions per k.  The sums
  // below still receive their terms in k order.
  for (int k0 = 0; k0 < f.K; k0 += FN_ROWS) {
    T wv[FN_ROWS][FN_CHUNKS];
    T ug[FN_ROWS], us[FN_ROWS];
#pragma unroll
    for (int i = 0; i < FN_ROWS; ++i) {
      const int k = k0 + i < f.K ? k0 + i : f.K - 1;           // (past the table: the last row again, read and not used)
      fn_load_row(wv[i], f.fn_w + (size_t)k * S, S, lane);
    }
#pragma unroll
    for (int i = 0; i < FN_ROWS; ++i) {
      ug[i] = us[i] = (T)0;
#pragma unroll
      for (int j = 0; j < FN_CHUNKS; ++j) {
        if (64 * j < S) {                    // wave-uniform: the chunks past S cost a scalar branch
          ug[i] += wv[i][j] * rg[j];         // (idle lanes of the last chunk: 0 * 0)
          if constexpr (TWO) us[i] += wv[i][j] * rs[j];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < FN_ROWS; ++i) {
      ug[i] = row_sum(ug[i]);
      if constexpr (TWO) us[i] = row_sum(us[i]);
    }
#pragma unroll
    for (int i = 0; i < FN_ROWS; ++i) {
      if (k0 + i < f.K) {                    // wave-uniform
        hg += fn_e(ug[i], abs_kind);
        const T eg = fn_de(ug[i], abs_kind);
        T es = (T)0;
        if constexpr (TWO) {
          hs += fn_e(us[i], abs_kind);
          es = fn_de(us[i], abs_kind);
        }
#pragma unroll
        for (int j = 0; j < FN_CHUNKS; ++j) {
          if (64 * j < S) {
            gg[j] += eg * wv[i][j];
            if constexpr (TWO) gs[j] += es * wv[i][j];
          }
        }
      }
    }
  }
  // ---- the rows, written once ----------------------------------------------------------------------------------------------
  const T cg = coef * f.lamk;
  T cs = (T)0;
  if constexpr (TWO) cs = (beta * coef) * f.lamk;
#pragma unroll
  for (int j = 0; j < FN_CHUNKS; ++j) {
    const int s = lane + 64 * j;
    if (s < S) {
      if (zero) {
        dpg[o + s] = (T)0;
        if constexpr (TWO) dps[o + s] = (T)0;
      } else {
        T dg, ds = (T)0;
        if (bin_w) {
          const T v = bin_w[s];
          dg = v != (T)0 ? v * elem_grad<T, KIND>(rg[j], k0, delta) : (T)0;
          if constexpr (TWO) ds = v != (T)0 ? v * elem_grad<T, KIND>(rs[j], k1, delta) : (T)0;
        } else {
          dg = elem_grad<T, KIND>(rg[j], k0, delta);
          if constexpr (TWO) ds = elem_grad<T, KIND>(rs[j], k1, delta);
        }
        dpg[o + s] = dg + cg * gg[j];
        if constexpr (TWO) dps[o + s] = ds + cs * gs[j];
      }
    }
  }
  if constexpr (TWO) return (r0 + beta * r1) + f.lamk * (hg + beta * hs);
  else return r0 + f.lamk * hg;
}

// w_b / B_global and whether w_b == 0; w == NULL: 1 / B_global
template <typename T>
__device__ __forceinline__ T fn_coef(const T* __restrict__ w, const int32_t* __restrict__ w_index, int b, T inv_bglobal, bool* zero) {
  *zero = false;
  if (!w) return inv_bglobal;
  const T wb = weight_of(w, w_index, b);
  *zero = wb == (T)0;
  return wb * inv_bglobal;
}

template <typename T, int KIND, bool TWO>
__global__ __launch_bounds__(ROWS_THREADS) void loss_fn_kernel(const T* __restrict__ pg, const T* __restrict__ ps,
                                                               const T* __restrict__ y, int B, int S, int clamp, T beta, T delta,
                                                               T inv_bglobal, T* __restrict__ dpg, T* __restrict__ dps,
                                                               T* __restrict__ per_crystal, const T* __restrict__ w,
                                                               const int32_t* __restrict__ w_index, const T* __restrict__ bin_w,
                                                               FnOperands<T> f) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * ROWS_WAVES + (threadIdx.x >> 6);
  if (b >= B) return;
  bool zero;
  const T coef = fn_coef(w, w_index, b, inv_bglobal, &zero);
  const T den = bin_w ? bin_total(bin_w, S, lane) : (T)S;
  const T l = fn_row<T, KIND, TWO>(pg, ps, y, (size_t)b * S, S, lane, clamp != 0, beta, delta, coef, zero, bin_w, den, f, dpg, dps);
  if (lane == 0) per_crystal[b] = l;
}

// per_crystal == NULL: one workgroup, the form and the order of loss_rows_solo_kernel (csrc/loss_rows.hip) - the same bits as
// loss_fn_kernel followed by loss_rows_total_kernel
template <typename T, int KIND, bool TWO>
__global__ __launch_bounds__(ROWS_THREADS) void loss_fn_solo_kernel(const T* __restrict__ pg, const T* __restrict__ ps,
                                                                    const T* __restrict__ y, int B, int S, int clamp, T beta,
                                                                    T delta, T inv_bglobal, T* __restrict__ dpg,
                                                                    T* __restrict__ dps, T* __restrict__ loss,
                                                                    const T* __restrict__ w, const int32_t* __restrict__ w_index,
                                                                    const T* __restrict__ bin_w, FnOperands<T> f) {
  __shared__ T share[ROWS_THREADS];
  __shared__ T red[ROWS_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T den = bin_w ? bin_total(bin_w, S, lane) : (T)S;
  T s = (T)0;
  for (int base = 0; base < B; base += ROWS_THREADS) {
    for (int i = wave; i < ROWS_THREADS && base + i < B; i += ROWS_WAVES) {
      bool zero;
      const T coef = fn_coef(w, w_index, base + i, inv_bglobal, &zero);
      const T l = fn_row<T, KIND, TWO>(pg, ps, y, (size_t)(base + i) * S, S, lane, clamp != 0, beta, delta, coef, zero, bin_w, den, f,
                                       dpg, dps);
      if (lane == 0)
        share[i] = w ? share_of<T, true>(l, inv_bglobal, w, w_index, base + i) : share_of<T, false>(l, inv_bglobal, w, w_index, base + i);
    }
    __syncthreads();
    if (base + (int)threadIdx.x < B) s += share[threadIdx.x];
    __syncthreads();
  }
  finish_total(s, red, loss);
}

// ---- normalised rows: the last K_norm rows of the table over D+ = max(sum_s fn_den[s] x_s, den_floor) ------------------------------
template <typename T>
struct FnNormOperands {
  const T* fn_den;     // [S]
  int K_norm;          // 1 .. K: rows K - K_norm .. K - 1 are normalised
  T den_floor;
};

// torch.clamp(min = floor): a NaN stays a NaN
template <typename T>
__device__ __forceinline__ T fn_floored(T d, T floor) { return d < floor ? floor : d; }

// fn_row with normalised rows: the predictions and the target themselves stay in registers, next to the denominator row
template <typename T, int KIND, bool TWO>
__device__ __forceinline__ T fn_norm_row(const T* __restrict__ pg, const T* __restrict__ ps, const T* __restrict__ y, size_t o, int S,
                                         int lane, bool clamp, T beta, T delta, T coef, bool zero, const T* __restrict__ bin_w,
                                         T den, const FnOperands<T>& f, const FnNormOperands<T>& g, T* __restrict__ dpg,
                                         T* __restrict__ dps) {
  T xg[FN_CHUNKS], xs[FN_CHUNKS], tt[FN_CHUNKS], gg[FN_CHUNKS], gs[FN_CHUNKS], dn[FN_CHUNKS];
  // ---- the pointwise term (fn_row's sums) and phase 0: D(pg), D(ps), D(t) -------------------------------------------------------
  T a = (T)0, c = (T)0, Dg = (T)0, Ds = (T)0, Dt = (T)0;
#pragma unroll
  for (int j = 0; j < FN_CHUNKS; ++j) {
    xg[j] = xs[j] = tt[j] = gg[j] = gs[j] = dn[j] = (T)0;
    const int s = lane + 64 * j;
    if (s < S) {
      tt[j] = target_of(y[o + s], clamp);
      xg[j] = pg[o + s];
      if constexpr (TWO) xs[j] = ps[o + s];
      dn[j] = g.fn_den[s];
      const T rg = xg[j] - tt[j], rs = xs[j] - tt[j];
      if (bin_w) {
        const T v = bin_w[s];
        if (v != (T)0) {
          a += v * elem_loss<T, KIND>(rg, delta);
          if constexpr (TWO) c += v * elem_loss<T, KIND>(rs, delta);
        }
      } else {
        a += elem_loss<T, KIND>(rg, delta);
        if constexpr (TWO) c += elem_loss<T, KIND>(rs, delta);
      }
    }
    if (64 * j < S) {                        // wave-uniform (idle lanes of the last chunk: 0 * 0)
      Dg += dn[j] * xg[j];
      if constexpr (TWO) Ds += dn[j] * xs[j];
      Dt += dn[j] * tt[j];
    }
  }
  a = row_sum(a);
  if constexpr (TWO) c = row_sum(c);
  Dg = row_sum(Dg);
  if constexpr (TWO) Ds = row_sum(Ds);
  Dt = row_sum(Dt);
  const T Pg = fn_floored(Dg, g.den_floor), Pt = fn_floored(Dt, g.den_floor);
  T Ps = (T)1;
  if constexpr (TWO) Ps = fn_floored(Ds, g.den_floor);
  const T r0 = row_term<T, KIND>(a, den);
  const T k0 = row_coef<T, KIND>(coef, r0, den);
  T r1 = (T)0, k1 = (T)0;
  if constexpr (TWO) {
    r1 = row_term<T, KIND>(c, den);
    k1 = row_coef<T, KIND>(beta * coef, r1, den);
  }
  const bool abs_kind = f.abs_kind != 0;
  T hg = (T)0, hs = (T)0, Ag = (T)0, As = (T)0;
  // the plain rows come first: two wave-uniform stretches of the k loop, FN_ROWS rows per trip in each (fn_row's reasons)
  const int Kp = f.K - g.K_norm;
  for (int part = 0; part < 2; ++part) {
    const bool norm = part != 0;
    const int kb = norm ? Kp : 0, ke = norm ? f.K : Kp;
    for (int kt = kb; kt < ke; kt += FN_ROWS) {
      T wv[FN_ROWS][FN_CHUNKS];
      T ug[FN_ROWS], us[FN_ROWS], ut[FN_ROWS];
#pragma unroll
      for (int i = 0; i < FN_ROWS; ++i) {
        const int k = kt + i < ke ? kt + i : ke - 1;             // (past the stretch: its last row again, read and not used)
        fn_load_row(wv[i], f.fn_w + (size_t)k * S, S, lane);
      }
      if (!norm) {                           // u_k = sum_s fn_w[k,s] (p_s - t_s): fn_row's numbers
#pragma unroll
        for (int i = 0; i < FN_ROWS; ++i) {
          ug[i] = us[i] = (T)0;
#pragma unroll
          for (int j = 0; j < FN_CHUNKS; ++j) {
            if (64 * j < S) {
              ug[i] += wv[i][j] * (xg[j] - tt[j]);
              if constexpr (TWO) us[i] += wv[i][j] * (xs[j] - tt[j]);
            }
          }
        }
#pragma unroll
        for (int i = 0; i < FN_ROWS; ++i) {
          ug[i] = row_sum(ug[i]);
          if constexpr (TWO) us[i] = row_sum(us[i]);
        }
      } else {                               // F_k(pg), F_k(ps), F_k(t): three reductions per row
#pragma unroll
        for (int i = 0; i < FN_ROWS; ++i) {
          ug[i] = us[i] = ut[i] = (T)0;
#pragma unroll
          for (int j = 0; j < FN_CHUNKS; ++j) {
            if (64 * j < S) {
              ug[i] += wv[i][j] * xg[j];
              if constexpr (TWO) us[i] += wv[i][j] * xs[j];
              ut[i] += wv[i][j] * tt[j];
            }
          }
        }
#pragma unroll
        for (int i = 0; i < FN_ROWS; ++i) {
          ug[i] = row_sum(ug[i]);
          if constexpr (TWO) us[i] = row_sum(us[i]);
          ut[i] = row_sum(ut[i]);
        }
      }
#pragma unroll
      for (int i = 0; i < FN_ROWS; ++i) {
        if (kt + i < ke) {                   // wave-uniform
          T eg, es = (T)0;
          if (!norm) {
            hg += fn_e(ug[i], abs_kind);
            eg = fn_de(ug[i], abs_kind);
            if constexpr (TWO) {
              hs += fn_e(us[i], abs_kind);
              es = fn_de(us[i], abs_kind);
            }
          } else {
            const T qt = ut[i] / Pt, qg = ug[i] / Pg;
            const T vg = qg - qt;
            hg += fn_e(vg, abs_kind);
            eg = fn_de(vg, abs_kind) / Pg;
            Ag += eg * qg;
            if constexpr (TWO) {
              const T qs = us[i] / Ps;
              const T vs = qs - qt;
              hs += fn_e(vs, abs_kind);
              es = fn_de(vs, abs_kind) / Ps;
              As += es * qs;
            }
          }
#pragma unroll
          for (int j = 0; j < FN_CHUNKS; ++j) {
            if (64 * j < S) {
              gg[j] += eg * wv[i][j];
              if constexpr (TWO) gs[j] += es * wv[i][j];
            }
          }
        }
      }
    }
  }
  // ---- the rows, written once ----------------------------------------------------------------------------------------------
  const T cg = coef * f.lamk;
  const T ag = Dg > g.den_floor ? Ag : (T)0;                     // a floored denominator is a constant
  T cs = (T)0, as = (T)0;
  if constexpr (TWO) {
    cs = (beta * coef) * f.lamk;
    as = Ds > g.den_floor ? As : (T)0;
  }
#pragma unroll
  for (int j = 0; j < FN_CHUNKS; ++j) {
    const int s = lane + 64 * j;
    if (s < S) {
      if (zero) {
        dpg[o + s] = (T)0;
        if constexpr (TWO) dps[o + s] = (T)0;
      } else {
        const T rg = xg[j] - tt[j], rs = xs[j] - tt[j];
        T dg, ds = (T)0;
        if (bin_w) {
          const T v = bin_w[s];
          dg = v != (T)0 ? v * elem_grad<T, KIND>(rg, k0, delta) : (T)0;
          if constexpr (TWO) ds = v != (T)0 ? v * elem_grad<T, KIND>(rs, k1, delta) : (T)0;
        } else {
          dg = elem_grad<T, KIND>(rg, k0, delta);
          if constexpr (TWO) ds = elem_grad<T, KIND>(rs, k1, delta);
        }
        dpg[o + s] = dg + cg * (gg[j] - ag * dn[j]);
        if constexpr (TWO) dps[o + s] = ds + cs * (gs[j] - as * dn[j]);
      }
    }
  }
  if constexpr (TWO) return (r0 + beta * r1) + f.lamk * (hg + beta * hs);
  else return r0 + f.lamk * hg;
}

// loss_fn_kernel / loss_fn_solo_kernel with fn_norm_row in place of fn_row
template <typename T, int KIND, bool TWO>
__global__ __launch_bounds__(ROWS_THREADS) void loss_fnn_kernel(const T* __restrict__ pg, const T* __restrict__ ps,
                                                                const T* __restrict__ y, int B, int S, int clamp, T beta, T delta,
                                                                T inv_bglobal, T* __restrict__ dpg, T* __restrict__ dps,
                                                                T* __restrict__ per_crystal, const T* __restrict__ w,
                                                                const int32_t* __restrict__ w_index, const T* __restrict__ bin_w,
                                                                FnOperands<T> f, FnNormOperands<T> g) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * ROWS_WAVES + (threadIdx.x >> 6);
  if (b >= B) return;
  bool zero;
  const T coef = fn_coef(w, w_index, b, inv_bglobal, &zero);
  const T den = bin_w ? bin_total(bin_w, S, lane) : (T)S;
  const T l = fn_norm_row<T, KIND, TWO>(pg, ps, y, (size_t)b * S, S, lane, clamp != 0, beta, delta, coef, zero, bin_w, den, f, g, dpg,
                                        dps);
  if (lane == 0) per_crystal[b] = l;
}

template <typename T, int KIND, bool TWO>
__global__ __launch_bounds__(ROWS_THREADS) void loss_fnn_solo_kernel(const T* __restrict__ pg, const T* __restrict__ ps,
                                                                     const T* __restrict__ y, int B, int S, int clamp, T beta,
                                                                     T delta, T inv_bglobal, T* __restrict__ dpg,
                                                                     T* __restrict__ dps, T* __restrict__ loss,
                                                                     const T* __restrict__ w, const int32_t* __restrict__ w_index,
                                                                     const T* __restrict__ bin_w, FnOperands<T> f,
                                                                     FnNormOperands<T> g) {
  __shared__ T share[ROWS_THREADS];
  __shared__ T red[ROWS_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T den = bin_w ? bin_total(bin_w, S, lane) : (T)S;
  T s = (T)0;
  for (int base = 0; base < B; base += ROWS_THREADS) {
    for (int i = wave; i < ROWS_THREADS && base + i < B; i += ROWS_WAVES) {
      bool zero;
      const T coef = fn_coef(w, w_index, base + i, inv_bglobal, &zero);
      const T l = fn_norm_row<T, KIND, TWO>(pg, ps, y, (size_t)(base + i) * S, S, lane, clamp != 0, beta, delta, coef, zero, bin_w,
                                            den, f, g, dpg, dps);
      if (lane == 0)
        share[i] = w ? share_of<T, true>(l, inv_bglobal, w, w_index, base + i) : share_of<T, false>(l, inv_bglobal, w, w_index, base + i);
    }
    __syncthreads();
    if (base + (int)threadIdx.x < B) s += share[threadIdx.x];
    __syncthreads();
  }
  finish_total(s, red, loss);
}

template <typename T>
struct FnArgs {
  const T *pg, *ps, *y;
  int B, S, B_global, clamp;
  T beta, delta;
  T *dpg, *dps, *per_crystal, *loss;
  const T* w;
  const int32_t* w_index;
  const T* bin_w;
  FnOperands<T> f;
  hipStream_t stream;
};

template <typename T, int KIND, bool TWO>
void launch_fn(const FnArgs<T>& a) {
  const T inv_bglobal = (T)1 / (T)a.B_global;
  if (a.per_crystal) {
    hipLaunchKernelGGL((loss_fn_kernel<T, KIND, TWO>), dim3(ceil_div(a.B, ROWS_WAVES)), dim3(ROWS_THREADS), 0, a.stream, a.pg, a.ps,
                       a.y, a.B, a.S, a.clamp, a.beta, a.delta, inv_bglobal, a.dpg, a.dps, a.per_crystal, a.w, a.w_index, a.bin_w, a.f);
    if (a.w)
      hipLaunchKernelGGL((loss_rows_total_kernel<T, true>), dim3(1), dim3(ROWS_THREADS), 0, a.stream, (const T*)a.per_crystal, a.B,
                         inv_bglobal, a.loss, a.w, a.w_index);
    else
      hipLaunchKernelGGL((loss_rows_total_kernel<T, false>), dim3(1), dim3(ROWS_THREADS), 0, a.stream, (const T*)a.per_crystal, a.B,
                         inv_bglobal, a.loss, a.w, a.w_index);
  } else {
    hipLaunchKernelGGL((loss_fn_solo_kernel<T, KIND, TWO>), dim3(1), dim3(ROWS_THREADS), 0, a.stream, a.pg, a.ps, a.y, a.B, a.S,
                       a.clamp, a.beta, a.delta, inv_bglobal, a.dpg, a.dps, a.loss, a.w, a.w_index, a.bin_w, a.f);
  }
}

template <typename T, int KIND>
void launch_fn_two(const FnArgs<T>& a) {
  if (a.ps) launch_fn<T, KIND, true>(a);
  else launch_fn<T, KIND, false>(a);
}

// the normalised kernels: launch_fn's launches with loss_fnn_* in place of loss_fn_*
template <typename T, int KIND, bool TWO>
void launch_fn_norm(const FnArgs<T>& a, const FnNormOperands<T>& g) {
  const T inv_bglobal = (T)1 / (T)a.B_global;
  if (a.per_crystal) {
    hipLaunchKernelGGL((loss_fnn_kernel<T, KIND, TWO>), dim3(ceil_div(a.B, ROWS_WAVES)), dim3(ROWS_THREADS), 0, a.stream, a.pg, a.ps,
                       a.y, a.B, a.S, a.clamp, a.beta, a.delta, inv_bglobal, a.dpg, a.dps, a.per_crystal, a.w, a.w_index, a.bin_w, a.f,
                       g);
    if (a.w)
      hipLaunchKernelGGL((loss_rows_total_kernel<T, true>), dim3(1), dim3(ROWS_THREADS), 0, a.stream, (const T*)a.per_crystal, a.B,
                         inv_bglobal, a.loss, a.w, a.w_index);
    else
      hipLaunchKernelGGL((loss_rows_total_kernel<T, false>), dim3(1), dim3(ROWS_THREADS), 0, a.stream, (const T*)a.per_crystal, a.B,
                         inv_bglobal, a.loss, a.w, a.w_index);
  } else {
    hipLaunchKernelGGL((loss_fnn_solo_kernel<T, KIND, TWO>), dim3(1), dim3(ROWS_THREADS), 0, a.stream, a.pg, a.ps, a.y, a.B, a.S,
                       a.clamp, a.beta, a.delta, inv_bglobal, a.dpg, a.dps, a.loss, a.w, a.w_index, a.bin_w, a.f, g);
  }
}

template <typename T, int KIND>
void launch_fn_norm_two(const FnArgs<T>& a, const FnNormOperands<T>& g) {
  if (a.ps) launch_fn_norm<T, KIND, true>(a, g);
  else launch_fn_norm<T, KIND, false>(a, g);
}

// what dosx_loss_rows_fn refuses, in its order
template <typename T>
int loss_rows_fn_check(const char* who, const T* pg, const T* ps, const T* y, int B, int S, int B_global, int kind, T delta,
                       const T* dpg, const T* dps, const T* loss, const T* w, const int32_t* w_index, const T* bin_w, const T* fn_w,
                       int K, int fn_kind, T lam) {
  if (const int rc = loss_rows_check<T>(who, pg, ps, y, B, S, B_global, kind, delta, dpg, dps, loss, true, w, w_index, bin_w))
    return rc;
  DOSX_CHECK_ARG(fn_kind == DOSX_FN_SQ || fn_kind == DOSX_FN_ABS, "%s: fn_kind=%d is not DOSX_FN_SQ or DOSX_FN_ABS", who, fn_kind);
  DOSX_CHECK_ARG(std::isfinite((double)lam) && lam >= (T)0, "%s: lam=%g must be finite and >= 0", who, (double)lam);
  if (fn_w) {
    DOSX_CHECK_ARG(K >= 1 && K <= FN_MAX, "%s: K=%d functionals, 1 .. %d with a table", who, K, FN_MAX);
    DOSX_CHECK_ARG(S <= FN_MAX, "%s: S=%d bins, at most %d with a table", who, S, FN_MAX);
    const size_t n = (size_t)B * (size_t)S, bytes = (size_t)K * (size_t)S * sizeof(T);
    DOSX_CHECK_ARG(!inside(fn_w, bytes, pg, n) && !inside(fn_w, bytes, ps, n) && !inside(fn_w, bytes, y, n) &&
                       !inside(fn_w, bytes, (const T*)dpg, n) && !inside(fn_w, bytes, (const T*)dps, n),
                   "%s: fn_w lies inside one of the [B,S] operands pg, ps, y, dpg, dps", who);
  }
  return 0;
}

// dosx_loss_rows_fn's launches behind its checks - also what the normalised entries run, under their names, with nothing to normalise
template <typename T>
int loss_rows_fn_launch(const char* who, const T* pg, const T* ps, const T* y, int B, int S, int B_global, int kind, int clamp_target,
                        T beta, T delta, T* dpg, T* dps, T* per_crystal, T* loss, const T* w, const int32_t* w_index,
                        const T* bin_w, const T* fn_w, int K, int fn_kind, T lam, dosx_stream_t stream) {
  if (!fn_w || lam == (T)0)               // the weighted entries' kernels, bit for bit
    return dosx_loss_rows_weighted_as<T>(who, pg, ps, y, B, S, B_global, kind, clamp_target, beta, delta, dpg, dps, per_crystal, loss,
                                         w, w_index, bin_w, stream);
  const FnArgs<T> a{pg, ps, y, B, S, B_global, clamp_target != 0, beta, delta, dpg, dps, per_crystal, loss, w, w_index, bin_w,
                    {fn_w, K, fn_kind == DOSX_FN_ABS, lam / (T)K}, to_stream(stream)};
  switch (kind) {
    case DOSX_LOSS_RMSE: launch_fn_two<T, DOSX_LOSS_RMSE>(a); break;
    case DOSX_LOSS_MSE: launch_fn_two<T, DOSX_LOSS_MSE>(a); break;
    case DOSX_LOSS_MAE: launch_fn_two<T, DOSX_LOSS_MAE>(a); break;
    default: launch_fn_two<T, DOSX_LOSS_HUBER>(a); break;
  }
  DOSX_LAUNCH_CHECK();
  return 0;
}

template <typename T>
int loss_rows_fn(const char* who, const T* pg, const T* ps, const T* y, int B, int S, int B_global, int kind, int clamp_target,
                 T beta, T delta, T* dpg, T* dps, T* per_crystal, T* loss, const T* w, const int32_t* w_index, const T* bin_w,
                 const T* fn_w, int K, int fn_kind, T lam, dosx_stream_t stream) {
  if (const int rc = loss_rows_fn_check<T>(who, pg, ps, y, B, S, B_global, kind, delta, dpg, dps, loss, w, w_index, bin_w, fn_w, K,
                                           fn_kind, lam))
    return rc;
  return loss_rows_fn_launch<T>(who, pg, ps, y, B, S, B_global, kind, clamp_target, beta, delta, dpg, dps, per_crystal, loss, w,
                                w_index, bin_w, fn_w, K, fn_kind, lam, stream);
}

template <typename T>
int loss_rows_fn_norm(const char* who, const T* pg, const T* ps, const T* y, int B, int S, int B_global, int kind, int clamp_target,
                      T beta, T delta, T* dpg, T* dps, T* per_crystal, T* loss, const T* w, const int32_t* w_index, const T* bin_w,
                      const T* fn_w, int K, int fn_kind, T lam, const T* fn_den, int K_norm, T den_floor, dosx_stream_t stream) {
  if (const int rc = loss_rows_fn_check<T>(who, pg, ps, y, B, S, B_global, kind, delta, dpg, dps, loss, w, w_index, bin_w, fn_w, K,
                                           fn_kind, lam))
    return rc;
  DOSX_CHECK_ARG(K_norm >= 0 && (!fn_w || K_norm <= K), "%s: K_norm=%d normalised rows, 0 .. K=%d (the table's last rows)", who,
                 K_norm, K);
  DOSX_CHECK_ARG(K_norm == 0 || fn_den, "%s: K_norm=%d normalised rows need the denominator row fn_den, which is NULL", who, K_norm);
  DOSX_CHECK_ARG(std::isfinite((double)den_floor) && den_floor > (T)0, "%s: den_floor=%g must be finite and > 0", who,
                 (double)den_floor);
  if (fn_den) {
    const size_t n = (size_t)B * (size_t)S, bytes = (size_t)S * sizeof(T);
    DOSX_CHECK_ARG(!inside(fn_den, bytes, pg, n) && !inside(fn_den, bytes, ps, n) && !inside(fn_den, bytes, y, n) &&
                       !inside(fn_den, bytes, (const T*)dpg, n) && !inside(fn_den, bytes, (const T*)dps, n),
                   "%s: fn_den lies inside one of the [B,S] operands pg, ps, y, dpg, dps", who);
  }
  if (!fn_w || lam == (T)0 || K_norm == 0)               // nothing to normalise: dosx_loss_rows_fn's kernels, bit for bit
    return loss_rows_fn_launch<T>(who, pg, ps, y, B, S, B_global, kind, clamp_target, beta, delta, dpg, dps, per_crystal, loss, w,
                                  w_index, bin_w, fn_w, K, fn_kind, lam, stream);
  const FnArgs<T> a{pg, ps, y, B, S, B_global, clamp_target != 0, beta, delta, dpg, dps, per_crystal, loss, w, w_index, bin_w,
                    {fn_w, K, fn_kind == DOSX_FN_ABS, lam / (T)K}, to_stream(stream)};
  const FnNormOperands<T> g{fn_den, K_norm, den_floor};
  switch (kind) {
    case DOSX_LOSS_RMSE: launch_fn_norm_two<T, DOSX_LOSS_RMSE>(a, g); break;
    case DOSX_LOSS_MSE: launch_fn_norm_two<T, DOSX_LOSS_MSE>(a, g); break;
    case DOSX_LOSS_MAE: launch_fn_norm_two<T, DOSX_LOSS_MAE>(a, g); break;
    default: launch_fn_norm_two<T, DOSX_LOSS_HUBER>(a, g); break;
  }
  DOSX_LAUNCH_CHECK();
  return 0;
}

// the descriptor forms: the same call with the table's side in a DosxFnNorm (a recorded call carries at most 19 integer-class arguments)
template <typename T>
int loss_rows_fn_norm_desc(const char* who, const T* pg, const T* ps, const T* y, int B, int S, int B_global, int kind,
                           int clamp_target, T beta, T delta, T* dpg, T* dps, T* per_crystal, T* loss, const T* w,
                           const int32_t* w_index, const T* bin_w, const DosxFnNorm* fn, dosx_stream_t stream) {
  DOSX_CHECK_ARG(fn, "%s: NULL descriptor fn", who);
  return loss_rows_fn_norm<T>(who, pg, ps, y, B, S, B_global, kind, clamp_target, beta, delta, dpg, dps, per_crystal, loss, w, w_index,
                              bin_w, (const T*)fn->fn_w, fn->K, fn->fn_kind, (T)fn->lam, (const T*)fn->fn_den, fn->K_norm,
                              (T)fn->den_floor, stream);
}

// ---- evaluation -------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(ROWS_THREADS) void eval_functionals_kernel(const T* __restrict__ pred, const T* __restrict__ y, int B,
                                                                        int S, const double* __restrict__ scale,
                                                                        const T* __restrict__ fn_w, int K, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * ROWS_WAVES + (threadIdx.x >> 6);
  if (b >= B) return;
  const size_t o = (size_t)b * S;
  const double sc = scale ? scale[b] : 1.0;
  double* __restrict__ op = out + (size_t)b * 2 * K;
  for (int k = 0; k < K; ++k) {
    const T* __restrict__ row = fn_w + (size_t)k * S;
    double fp = 0.0, fy = 0.0;
    for (int s = lane; s < S; s += 64) {
      const double wv = (double)row[s];
      fp += wv * (double)pred[o + s];
      fy += wv * (double)y[o + s];
    }
    fp = row_sum(fp);
    fy = row_sum(fy);
    if (lane == 0) {
      op[k] = fp * sc;
      op[K + k] = fy * sc;
    }
  }
}

template <typename T>
int eval_functionals(const char* who, const T* pred, const T* y, int B, int S, const double* scale, const T* fn_w, int K,
                     double* out, dosx_stream_t stream) {
  DOSX_CHECK_ARG(B >= 0 && S >= 1 && K >= 1, "%s: B=%d S=%d K=%d (B >= 0, S >= 1 and K >= 1)", who, B, S, K);
  if (B == 0) return 0;
  DOSX_CHECK_ARG(pred && y && fn_w && out, "%s: NULL operand (only scale may be NULL)", who);
  hipLaunchKernelGGL(eval_functionals_kernel<T>, dim3(ceil_div(B, ROWS_WAVES)), dim3(ROWS_THREADS), 0, to_stream(stream), pred, y, B,
                     S, scale, fn_w, K, out);
  DOSX_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int dosx_loss_rows_fn(const float* pg, const float* ps, const float* y, int B, int S, int B_global, int kind,
                                 int clamp_target, float beta, float delta, float* dpg, float* dps, float* per_crystal, float* loss,
                                 const float* w, const int32_t* w_index, const float* bin_w, const float* fn_w, int K, int fn_kind,
                                 float lam, dosx_stream_t stream) {
  return loss_rows_fn<float>("dosx_loss_rows_fn", pg, ps, y, B, S, B_global, kind, clamp_target, beta, delta, dpg, dps, per_crystal,
                             loss, w, w_index, bin_w, fn_w, K, fn_kind, lam, stream);
}

extern "C" int dosx_loss_rows_fn_f64(const double* pg, const double* ps, const double* y, int B, int S, int B_global, int kind,
                                     int clamp_target, double beta, double delta, double* dpg, double* dps, double* per_crystal,
                                     double* loss, const double* w, const int32_t* w_index, const double* bin_w, const double* fn_w,
                                     int K, int fn_kind, double lam, dosx_stream_t stream) {
  return loss_rows_fn<double>("dosx_loss_rows_fn_f64", pg, ps, y, B, S, B_global, kind, clamp_target, beta, delta, dpg, dps,
                              per_crystal, loss, w, w_index, bin_w, fn_w, K, fn_kind, lam, stream);
}

extern "C" int dosx_loss_rows_fn_norm(const float* pg, const float* ps, const float* y, int B, int S, int B_global, int kind,
                                      int clamp_target, float beta, float delta, float* dpg, float* dps, float* per_crystal,
                                      float* loss, const float* w, const int32_t* w_index, const float* bin_w, const float* fn_w,
                                      int K, int fn_kind, float lam, const float* fn_den, int K_norm, float den_floor,
                                      dosx_stream_t stream) {
  return loss_rows_fn_norm<float>("dosx_loss_rows_fn_norm", pg, ps, y, B, S, B_global, kind, clamp_target, beta, delta, dpg, dps,
                                  per_crystal, loss, w, w_index, bin_w, fn_w, K, fn_kind, lam, fn_den, K_norm, den_floor, stream);
}

extern "C" int dosx_loss_rows_fn_norm_f64(const double* pg, const double* ps, const double* y, int B, int S, int B_global, int kind,
                                          int clamp_target, double beta, double delta, double* dpg, double* dps, double* per_crystal,
                                          double* loss, const double* w, const int32_t* w_index, const double* bin_w,
                                          const double* fn_w, int K, int fn_kind, double lam, const double* fn_den, int K_norm,
                                          double den_floor, dosx_stream_t stream) {
  return loss_rows_fn_norm<double>("dosx_loss_rows_fn_norm_f64", pg, ps, y, B, S, B_global, kind, clamp_target, beta, delta, dpg, dps,
                                   per_crystal, loss, w, w_index, bin_w, fn_w, K, fn_kind, lam, fn_den, K_norm, den_floor, stream);
}

extern "C" int dosx_loss_rows_fn_norm_desc(const float* pg, const float* ps, const float* y, int B, int S, int B_global, int kind,
                                           int clamp_target, float beta, float delta, float* dpg, float* dps, float* per_crystal,
                                           float* loss, const float* w, const int32_t* w_index, const float* bin_w,
                                           const DosxFnNorm* fn, dosx_stream_t stream) {
  return loss_rows_fn_norm_desc<float>("dosx_loss_rows_fn_norm_desc", pg, ps, y, B, S, B_global, kind, clamp_target, beta, delta, dpg,
                                       dps, per_crystal, loss, w, w_index, bin_w, fn, stream);
}

extern "C" int dosx_loss_rows_fn_norm_desc_f64(const double* pg, const double* ps, const double* y, int B, int S, int B_global,
                                               int kind, int clamp_target, double beta, double delta, double* dpg, double* dps,
                                               double* per_crystal, double* loss, const double* w, const int32_t* w_index,
                                               const double* bin_w, const DosxFnNorm* fn, dosx_stream_t stream) {
  return loss_rows_fn_norm_desc<double>("dosx_loss_rows_fn_norm_desc_f64", pg, ps, y, B, S, B_global, kind, clamp_target, beta, delta,
                                        dpg, dps, per_crystal, loss, w, w_index, bin_w, fn, stream);
}

extern "C" int dosx_eval_functionals(const float* pred, const float* y, int B, int S, const double* scale, const float* fn_w, int K,
                                     double* out, dosx_stream_t stream) {
  return eval_functionals<float>("dosx_eval_functionals", pred, y, B, S, scale, fn_w, K, out, stream);
}

extern "C" int dosx_eval_functionals_f64(const double* pred, const double* y, int B, int S, const double* scale, const double* fn_w,
                                         int K, double* out, dosx_stream_t stream) {
  return eval_functionals<double>("dosx_eval_functionals_f64", pred, y, B, S, scale, fn_w, K, out, stream);
}
