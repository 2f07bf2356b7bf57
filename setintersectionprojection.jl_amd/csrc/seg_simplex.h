// Simplex sets: { v : v_i >= 0, smin <= sum_i v_i <= smax } on every fiber / slice of a materialised vector (ext_segments.hip,
// SimplexSegProj), 0 <= smin <= smax, smax > 0, both finite and shared by all segments.  smin = smax = 1 is the probability simplex,
// smin = 0 the capped one.  The rule of one segment as __host__ __device__ functions (tests/simplex/rule_driver.cpp runs them on the
// CPU) and the two kernels behind the set; the kernels call nothing else for the arithmetic.  The reference package has no such projector.
//
// RULE.  Pass 1 of a segment of L entries: spos = sum max(v_i, 0) and sall = sum v_i, both in twice the working precision (L21Sum of
// l21.h: the entries are signed and the sums cancel), nneg = #{ v_i < 0 }.  The decision compares in T, as seg_norm.h does:
//   keep    smin <= (T)spos <= smax and nneg == 0: the segment is not written at all, its bits stay (-0.0 included)
//   clip    smin <= (T)spos <= smax and nneg  > 0: only the negative entries are written, as +0
//   shift   otherwise, onto the face sum = b, b = smax if (T)spos > smax, else smin: Michelot's fixed point from theta_0 = (sall - b) / L,
//           A_k = { i : v_i > theta_k }, theta_{k+1} = max(theta_k, (S_k - b) / C_k), until the integer count repeats or is 0.  theta is
//           negative on the lower side; the reference's `rho + 1 < lv` cap of the l1 ball is not used.  (S - b) / C: S - b as an
//           unevaluated sum of two doubles, the quotient and one correction from its exact remainder (simplex_theta), so that theta is
//           the exact threshold of the active set rounded to float64 but for ties within 2^-100; rounded once to T.
//           Apply, all in T: t = v_i - theta, x_i = t > 0 ? t : +0 (an entry on the threshold comes back +0).
// theta only grows, so the count only shrinks: the loops end after at most L + 1 steps for every input.  A NaN in a segment makes spos
// NaN, no comparison holds, theta is NaN and the segment comes back all +0; so does one whose sums overflow.
// No floating-point atomics, no state between calls: two calls give the same bits.
//
// LANE ROUTE (k_simplex_lane).  Fibers whose neighbours along array axis 0 are contiguous (sSa == 1: fiber y, fiber z) and L <=
// SIMPLEX_REG_MAX: one lane owns one segment.  A wave takes 64 neighbouring segments of a row; a lane loads its L values once with stride
// sTa -- 64 consecutive addresses per load across the wave -- keeps them in registers (L is bounded by the template bucket LB, every
// loop over the values is unrolled, the array never goes to scratch) and runs pass 1, Michelot's loop and the apply on its own: no
// LDS, no barrier, no cross-lane reduction.  Sums in index order: the bits of simplex_project_serial.  Lanes past the end of a row do
// nothing.
// TILE ROUTE (k_simplex_tile).  Everything else: the mapping, the LDS residency rule and the plan of seg_norm.h (seg_norm_plan,
// seg_toff, seg_tile_base).  Reductions are fixed trees: serial per thread in t order, l21_sum_merge in a butterfly over the lanes of a
// wave that share a segment (the lowest such lane's result is taken), the four waves' pairs merged in wave order.
// OBSERVATION.  Both kernels with OBS = true are pass 1 alone: out[s] = (T)spos of segment s in SegMap's order, by the route and in the
// order of the projector -- the very number it compares with smin and smax.
#pragma once
#include <cmath>
#include <stdexcept>

#include "l21.h"
#include "seg_norm.h"

namespace sipx {

// Longest fiber of the lane route: the largest bucket of k_simplex_lane.  A bucket of 32 compiles without scratch too (registers)
// but did not beat the tile mapping's time at 256 x 256 x 32 on an MI355X, so fibers of 17 .. 32 entries take the tile route.
constexpr int SIMPLEX_REG_MAX = 16;

// ---- host: what sipx_add_set, sipx_project and sipx_segment_sums refuse (set_config.h, the engine, SimplexSegProj) ----------------------
constexpr const char* SIMPLEX_NEEDS_MODE = "the simplex set (simplex) on the whole array is not built yet: it constrains every fiber or slice -- use a "
                                           "(\"fiber\", d) or (\"slice\", d) mode, or (\"bounds\") together with (\"l1\") on the whole array as a stand-in";
constexpr const char* SIMPLEX_2D_SLICE = "for 2D models, the mode of application for simplex sets needs to be (fiber,x) or (fiber,z)";
constexpr const char* SIMPLEX_ONE_BLOCK = "the simplex set (simplex) constrains the fibers or slices of the range of a one-block operator: TD_OP must "
                                          "be the identity, D_x, D_y or D_z -- for TV or a custom operator use one set per direction";
constexpr const char* SIMPLEX_NO_TRANSFORM = "the simplex set (simplex) takes no transform (DFT, DCT, wavelet): it acts on A x itself -- use it "
                                             "with TD_OP identity, D_x, D_y or D_z";
constexpr const char* SIMPLEX_NO_MINKOWSKI = "the simplex set (simplex) takes no Minkowski component: constrain the sum of the components "
                                             "with a set on the identity instead";
constexpr const char* SIMPLEX_NO_VECTORS = "the simplex set (simplex) takes one pair of scalars (min, max) for all segments for now and no lb / ub "
                                           "vectors: use (\"l1\", op, mode) with one radius per segment beside (\"bounds\")";
constexpr const char* SIMPLEX_SHARDED = "the simplex set (simplex) takes single-process contexts only, this one has a communicator, a slab "
                                        "decomposition or set ownership: use (\"bounds\") with (\"l1\", op, mode), or a single process";
constexpr const char* SIMPLEX_BAD_BOUNDS = "the simplex set (simplex) needs 0 <= min <= max, max > 0, both finite: every segment has entries >= 0 "
                                           "and a sum in [min, max] (min = max = 1: the probability simplex, min = 0: the capped one)";
template <typename T>
void simplex_check_bounds(double smin, double smax) {
  const T lo = (T)smin, hi = (T)smax;
  if (!(lo >= T(0)) || !(lo <= hi) || !(hi > T(0)) || !(hi < (T)INFINITY)) throw std::runtime_error(SIMPLEX_BAD_BOUNDS);
}

// ---- pass 1 ------------------------------------------------------------------------------------------------------------------------------
struct SimplexSums {
  L21Sum spos{0.0, 0.0}, sall{0.0, 0.0};
  double nneg = 0.0;
};
template <typename T>
__host__ __device__ inline void simplex_take(SimplexSums& a, T v) {
  const double x = (double)v;
  l21_sum_add(a.sall, x);
  l21_sum_add(a.spos, v < T(0) ? 0.0 : x);     // (a NaN stays a NaN)
  a.nneg += v < T(0) ? 1.0 : 0.0;
}
// the sum the decision compares and the observer reports
template <typename T>
__host__ __device__ inline T simplex_round(const L21Sum& s) {
  return (T)(s.hi + s.lo);
}
enum { SIMPLEX_KEEP = 0, SIMPLEX_CLIP = 1, SIMPLEX_SHIFT = 2 };
// b: the face a SIMPLEX_SHIFT segment goes to
template <typename T>
__host__ __device__ inline int simplex_decide(T spos, double nneg, T smin, T smax, double& b) {
  b = (double)smin;
  if (smin <= spos && spos <= smax) return nneg > 0.0 ? SIMPLEX_CLIP : SIMPLEX_KEEP;
  if (spos > smax) b = (double)smax;
  return SIMPLEX_SHIFT;
}

// ---- Michelot's iteration ----------------------------------------------------------------------------------------------------------------
// (S - b) / C of a sum in twice the working precision: the remainder of a float64 division is a float64
__host__ __device__ inline double simplex_theta(const L21Sum& S, double C, double b) {
  double d, e;
  l21_two_sum(S.hi, -b, d, e);
  const double q = d / C;
  const double r = fma(-q, C, d);
  return q + (r + (e + S.lo)) / C;
}
struct SimplexState {
  double theta, cprev;
  int done, steps;
};
__host__ __device__ inline SimplexState simplex_start(const L21Sum& sall, double b, long long L) {
  SimplexState st;
  st.theta = simplex_theta(sall, (double)L, b);
  st.cprev = -1.0;
  st.done = 0;
  st.steps = 0;
  return st;
}
template <typename T>
__host__ __device__ inline bool simplex_active(T v, double theta) {
  return (double)v > theta;
}
// S, C: sum and count of the entries above st.theta
__host__ __device__ inline void simplex_step(SimplexState& st, const L21Sum& S, double C, double b) {
  double tn = st.theta;
  if (C > 0.0) tn = simplex_theta(S, C, b);
  st.done = (C == st.cprev || !(C > 0.0)) ? 1 : 0;
  st.theta = tn > st.theta ? tn : st.theta;
  st.cprev = C;
  st.steps += 1;
}
template <typename T>
__host__ __device__ inline T simplex_apply(T v, T theta) {
  const T t = v - theta;
  return t > T(0) ? t : T(0);
}

// The lane route's bucket for a segment mapping (the template parameter LB of k_simplex_lane), 0: the tile route
__host__ __device__ inline int simplex_lane_bucket(const SegMap& m) {
  if (m.LB != 1 || m.sSa != 1 || m.L > SIMPLEX_REG_MAX) return 0;
  return m.L <= 4 ? 4 : (m.L <= 8 ? 8 : 16);
}

// One segment serially, sums in index order: what the lane route computes bit for bit, and the tile route up to the order of its sums.
// Returns the decision; theta (as applied, 0 unless SIMPLEX_SHIFT), (T)spos and the Michelot steps come back.
template <typename T>
__host__ __device__ inline int simplex_project_serial(T* v, long long L, long long stride, T smin, T smax, T& theta_T, T& spos_T, int& steps) {
  SimplexSums a;
  for (long long i = 0; i < L; ++i) simplex_take<T>(a, v[i * stride]);
  spos_T = simplex_round<T>(a.spos);
  theta_T = T(0);
  steps = 0;
  double b;
  const int act = simplex_decide<T>(spos_T, a.nneg, smin, smax, b);
  if (act == SIMPLEX_KEEP) return act;
  if (act == SIMPLEX_CLIP) {
    for (long long i = 0; i < L; ++i)
      if (v[i * stride] < T(0)) v[i * stride] = T(0);
    return act;
  }
  SimplexState st = simplex_start(a.sall, b, L);
  for (long long it = 0; it <= L + 1 && !st.done; ++it) {
    L21Sum S{0.0, 0.0};
    double C = 0.0;
    for (long long i = 0; i < L; ++i)
      if (simplex_active<T>(v[i * stride], st.theta)) {
        l21_sum_add(S, (double)v[i * stride]);
        C += 1.0;
      }
    simplex_step(st, S, C, b);
  }
  steps = st.steps;
  theta_T = (T)st.theta;
  for (long long i = 0; i < L; ++i) v[i * stride] = simplex_apply<T>(v[i * stride], theta_T);
  return act;
}

#if defined(__HIPCC__)
// ---- lane route ----------------------------------------------------------------------------------------------------------------------------
// tile = 64 neighbouring segments of one row (nchunk tiles a row, ntile in all); a workgroup's four waves take four tiles at a time
template <typename T, int LB, bool OBS>
__global__ __launch_bounds__(BLOCK) void k_simplex_lane(SegMap m, long long nchunk, long long ntile, T* __restrict__ v, T smin, T smax,
                                                        T* __restrict__ out) {
  static_assert(LB <= SIMPLEX_REG_MAX, "a bucket above the lane route's bound");
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int L = (int)m.L;
  const long long sTa = m.sTa;
  for (long long tile = (long long)blockIdx.x * (BLOCK / 64) + wave; tile < ntile; tile += (long long)gridDim.x * (BLOCK / 64)) {
    const long long sb = tile / nchunk, sa = (tile - sb * nchunk) * 64 + lane;
    if (sa >= m.SA) continue;
    T* const vs = v + sa + sb * m.sSb;          // (sSa == 1)
    T x[LB];
#pragma unroll
    for (int i = 0; i < LB; ++i) x[i] = i < L ? vs[i * sTa] : T(0);
    SimplexSums a;
#pragma unroll
    for (int i = 0; i < LB; ++i)
      if (i < L) simplex_take<T>(a, x[i]);
    const T sp = simplex_round<T>(a.spos);
    if constexpr (OBS) {
      out[sa + m.SA * sb] = sp;
    } else {
      double b;
      const int act = simplex_decide<T>(sp, a.nneg, smin, smax, b);
      if (act == SIMPLEX_KEEP) continue;
      if (act == SIMPLEX_CLIP) {
#pragma unroll
        for (int i = 0; i < LB; ++i)
          if (i < L && x[i] < T(0)) vs[i * sTa] = T(0);
        continue;
      }
      SimplexState st = simplex_start(a.sall, b, L);
      for (int it = 0; it <= L + 1 && !st.done; ++it) {
        L21Sum S{0.0, 0.0};
        double C = 0.0;
#pragma unroll
        for (int i = 0; i < LB; ++i)
          if (i < L && simplex_active<T>(x[i], st.theta)) {
            l21_sum_add(S, (double)x[i]);
            C += 1.0;
          }
        simplex_step(st, S, C, b);
      }
      const T theta = (T)st.theta;
#pragma unroll
      for (int i = 0; i < LB; ++i)
        if (i < L) vs[i * sTa] = simplex_apply<T>(x[i], theta);
    }
  }
}

// ---- tile route ----------------------------------------------------------------------------------------------------------------------------
// The pairs a (and b when TWO) and the count c over the lanes that share a segment, returned to each of them.  `red`: 5 * BLOCK doubles.
template <bool TWO>
__device__ __forceinline__ void simplex_tile_merge(L21Sum& a, L21Sum& b, double& c, int F, double* red) {
  for (int o = F; o < 64; o <<= 1) {
    const L21Sum pa{__shfl_xor(a.hi, o, 64), __shfl_xor(a.lo, o, 64)};
    l21_sum_merge(a, pa);
    if constexpr (TWO) {
      const L21Sum pb{__shfl_xor(b.hi, o, 64), __shfl_xor(b.lo, o, 64)};
      l21_sum_merge(b, pb);
    }
    c += __shfl_xor(c, o, 64);
  }
  const int tid = (int)threadIdx.x, f = tid & (F - 1);
  red[tid] = a.hi; red[BLOCK + tid] = a.lo; red[2 * BLOCK + tid] = c;
  if constexpr (TWO) { red[3 * BLOCK + tid] = b.hi; red[4 * BLOCK + tid] = b.lo; }
  __syncthreads();
  a = L21Sum{red[f], red[BLOCK + f]};           // the lowest lane of the segment in wave 0, then waves 1 .. 3 in order
  c = red[2 * BLOCK + f];
  if constexpr (TWO) b = L21Sum{red[3 * BLOCK + f], red[4 * BLOCK + f]};
  for (int w = 1; w < BLOCK / 64; ++w) {
    l21_sum_merge(a, L21Sum{red[64 * w + f], red[BLOCK + 64 * w + f]});
    c += red[2 * BLOCK + 64 * w + f];
    if constexpr (TWO) l21_sum_merge(b, L21Sum{red[3 * BLOCK + 64 * w + f], red[4 * BLOCK + 64 * w + f]});
  }
  __syncthreads();
}

template <typename T, bool OBS>
__global__ __launch_bounds__(BLOCK) void k_simplex_tile(SegMap m, SegNormPlan p, T* __restrict__ v, T smin, T smax, T* __restrict__ out) {
  static_assert(BLOCK == 256, "four waves: simplex_tile_merge merges four wave totals");
  extern __shared__ __align__(16) unsigned char simplex_lds[];
  __shared__ double red[5 * BLOCK];
  T* const sm = reinterpret_cast<T*>(simplex_lds);
  const int F = p.F, G = BLOCK >> p.logF;
  const int f = (int)threadIdx.x & (F - 1), r = (int)threadIdx.x >> p.logF;
  const long long L = m.L;
  const bool keep = !OBS && p.lds;
  for (long long tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
    long long base;
    const bool live = seg_tile_base(m, p, tile, f, base);
    T* const vs = v + base;
    // pass 1: the sums; the values go to LDS when they fit
    SimplexSums a;
    if (live)
      for (long long t = r; t < L; t += G) {
        const T x = vs[seg_toff(m, t)];
        if (keep) sm[t * F + f] = x;
        simplex_take<T>(a, x);
      }
    simplex_tile_merge<true>(a.spos, a.sall, a.nneg, F, red);
    const T sp = simplex_round<T>(a.spos);
    if constexpr (OBS) {
      if (live && r == 0) out[seg_tile_index(m, p, tile, f)] = sp;
    } else {
      double b = 0.0;
      const int act = live ? simplex_decide<T>(sp, a.nneg, smin, smax, b) : SIMPLEX_KEEP;
      SimplexState st = simplex_start(a.sall, b, L);
      st.done = act == SIMPLEX_SHIFT ? 0 : 1;
      for (long long it = 0; it <= L + 1; ++it) {
        if (__syncthreads_and(st.done)) break;
        L21Sum S{0.0, 0.0}, none{0.0, 0.0};
        double C = 0.0;
        if (!st.done)
          for (long long t = r; t < L; t += G) {
            const T x = keep ? sm[t * F + f] : vs[seg_toff(m, t)];
            if (simplex_active<T>(x, st.theta)) {
              l21_sum_add(S, (double)x);
              C += 1.0;
            }
          }
        simplex_tile_merge<false>(S, none, C, F, red);
        if (!st.done) simplex_step(st, S, C, b);
      }
      // last pass: a segment inside the set and nonnegative is not written
      if (act != SIMPLEX_KEEP) {
        const T theta = (T)st.theta;
        for (long long t = r; t < L; t += G) {
          const long long o = seg_toff(m, t);
          const T x = keep ? sm[t * F + f] : vs[o];
          if (act == SIMPLEX_SHIFT) vs[o] = simplex_apply<T>(x, theta);
          else if (x < T(0)) vs[o] = T(0);
        }
      }
    }
  }
}
#endif

}  // namespace sipx
