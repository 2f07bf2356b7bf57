// l1 ball, l2 ball and annulus per fiber / per slice of a materialised vector (ext_segments.hip, NormSegProj): the plan of a
// launch and the threshold rule of one segment as __host__ __device__ functions (tests/seg_norms/plan_driver.cpp runs them on
// the CPU), and the one kernel behind all three sets.
//
// Every segment is projected by the rule of the whole-array projector (kernels_proj.hip: decide_body, l1_solve_body):
//   l1       project_l1_Duchi!.jl:21-52: ||v||_1 <= b returns v; otherwise Michelot's fixed point of sum(max(|v| - theta, 0)) = b
//            in float64 from theta_0 = (||v||_1 - b) / L until the active count repeats, the reference's `rho + 1 < lv` cap,
//            theta = max(0, .) rounded once to TF, soft_thr per entry
//   l2       project_l2!.jl:8-13, norm from a float64 sum of squares
//   annulus  project_annulus!.jl:9-18, the constant fill sigma_min / sqrt(L) of an all-zero segment included
// A segment inside its set is not written at all.
//
// MAPPING.  A workgroup owns a TILE of F neighbouring segments along array axis 0 (F a power of two, 1 <= F <= 64) and gives each
// BLOCK / F lanes: thread tid works on segment f = tid % F of the tile and on the elements t = tid / F, tid / F + BLOCK / F, ...
//   F == 1   the segment's own elements are contiguous (sTa == 1: fiber x, slice y, slice z): lanes run along t
//   F  > 1   they are not, but neighbouring segments are (sSa == 1: fiber y, fiber z, slice x): lanes run along the segment
//            index first, so a wave reads runs of F consecutive addresses; the last tile along axis 0 may hold fewer segments
// RESIDENCY.  When the F * L values of a tile fit SEGN_LDS_BYTES they are read from global memory once and kept in LDS (every
// thread re-reads its own entries only: no barrier guards them); otherwise every pass re-reads global memory.
// REDUCTIONS are fixed trees: serial per thread in t order, a butterfly over the lanes of a wave that share a segment, the four
// waves' totals added in wave order.  No floating-point atomics, no state between calls: two calls give the same bits.
// RADII.  All segments share the scalar pmin / pmax, or every segment has its own: rmin[s] / rmax[s], s = seg_tile_index (SegMap's
// order, s = sa + SA * sb).  The lanes of a segment load one address, the F segments of a tile F consecutive ones, once per tile into a
// register.  An l1 radius that is not > 0 can only arrive from device memory (every host path refuses it): the ball is {0} or empty,
// and a segment that is not all zero is set to zero.  The loops end for every radius, NaN included.
// OBSERVATION.  k_seg_observe is pass 1 on its own (segn_pass1, shared with the projector): segment s writes (T)asum or
// (T)sqrt(sumsq), the very numbers k_seg_norm compares with the radii -- radii observed on v make v a point the projector does not write.
#pragma once
#include "ext_family.h"

namespace sipx {

enum { SEGN_L1 = 0, SEGN_L2 = 1, SEGN_ANNULUS = 2 };
// Per-workgroup budget of resident values.  gfx950 has 160 KiB of LDS per compute unit and a kernel may declare 64 KiB; with the
// 4 KiB of reduction scratch a resident workgroup takes at most 36 KiB: four per compute unit.
constexpr int SEGN_LDS_BYTES = 32 * 1024;
constexpr int SEGN_RUN_BYTES = 128;          // run of consecutive addresses a full tile reads per element index: one cache line
constexpr long long SEGN_MAX_GRID = 4ll * NB;

struct SegNormPlan {
  int F, logF;                // segments per tile
  int lds;                    // 1: the tile's values stay in LDS
  long long ntA, ntiles;      // tiles along axis 0, tiles in all
  unsigned grid;
  unsigned lds_bytes;         // dynamic LDS of the launch
  // the four paths, for the tests: 0 segment/LDS, 1 segment/streaming, 2 tile/LDS, 3 tile/streaming
  __host__ __device__ int path() const { return (F > 1 ? 2 : 0) + (lds ? 0 : 1); }
};

__host__ __device__ inline SegNormPlan seg_norm_plan(const SegMap& m, int elem_bytes) {
  SegNormPlan p{};
  p.F = 1;
  if (m.sTa != 1 && m.sSa == 1 && m.SA > 1) {
    const int fmax = SEGN_RUN_BYTES / elem_bytes > 64 ? 64 : SEGN_RUN_BYTES / elem_bytes;
    while (p.F < fmax && p.F < m.SA) p.F <<= 1;
  }
  while ((1 << p.logF) < p.F) ++p.logF;
  p.ntA = (m.SA + p.F - 1) / p.F;
  p.ntiles = p.ntA * (m.nseg / m.SA);
  p.lds = (long long)p.F * m.L * elem_bytes <= (long long)SEGN_LDS_BYTES ? 1 : 0;
  p.lds_bytes = p.lds ? (unsigned)(p.F * m.L * elem_bytes) : 0u;
  p.grid = (unsigned)(p.ntiles < SEGN_MAX_GRID ? (p.ntiles < 1 ? 1 : p.ntiles) : SEGN_MAX_GRID);
  return p;
}

// offset of element t inside its segment (fiber / slice modes: t = ta + LA * tb, see seg_addr; L < 2^31)
__host__ __device__ inline long long seg_toff(const SegMap& m, long long t) {
  if (m.LB == 1) return t * m.sTa;
  const unsigned tb = (unsigned)t / (unsigned)m.LA, ta = (unsigned)t - tb * (unsigned)m.LA;
  return (long long)ta * m.sTa + (long long)tb * m.sTb;
}
// segment `f` of tile `tile`: its index along axis 0 (>= SA: the ragged end of the last tile, no segment) and its first address
__host__ __device__ inline bool seg_tile_base(const SegMap& m, const SegNormPlan& p, long long tile, int f, long long& base) {
  const long long ia = tile % p.ntA, sb = tile / p.ntA, sa = ia * p.F + f;
  base = sa * m.sSa + sb * m.sSb;
  return sa < m.SA;
}

// index of that segment in SegMap's order (what rmin / rmax and the observed norms are indexed by), -1 for a lane of the ragged end
__host__ __device__ inline long long seg_tile_index(const SegMap& m, const SegNormPlan& p, long long tile, int f) {
  const long long ia = tile % p.ntA, sb = tile / p.ntA, sa = ia * p.F + f;
  return sa < m.SA ? sa + m.SA * sb : -1;
}

// Michelot's iteration of one segment.  theta only ever grows, so the active count C(theta) = #{|v| > theta} only shrinks: the
// iteration ends after at most L + 1 steps, when the count repeats (k_l1_solve's rule, no tolerance) or nothing is active.
struct L1SegState {
  double theta, cprev;
  int done;
};
__host__ __device__ inline L1SegState l1_seg_start(double asum, double b, long long L) {
  L1SegState st;
  st.theta = (asum - b) / (double)L;
  st.cprev = -1.0;
  st.done = 0;
  return st;
}
// S, C: sum and count of the magnitudes above st.theta
__host__ __device__ inline void l1_seg_step(L1SegState& st, double S, double C, double b) {
  double tn = st.theta;
  if (C > 0) tn = (S - b) / C;
  st.done = (C == st.cprev || !(C > 0)) ? 1 : 0;
  st.theta = tn > st.theta ? tn : st.theta;
  st.cprev = C;
}
// The reference's scan `while u[rho+1] > (sv[rho+1]-b)/(rho+1) && rho+1 < lv` (project_l1_Duchi!.jl:42) never lets the active set
// reach the whole segment: when every entry would stay active it thresholds with (||v||_1 - min|v| - b) / (lv - 1).
__host__ __device__ inline double l1_seg_finish(const L1SegState& st, double asum, double vmin, double b, long long L) {
  double theta = st.theta;
  if (st.cprev >= (double)L && L > 1) theta = (asum - vmin - b) / (double)(L - 1);
  return theta > 0 ? theta : 0.0;               // theta = max(0, .)   project_l1_Duchi!.jl:46
}

// l2 / annulus of one segment from its float64 sum of squares: 0 inside the set, 1 multiply by `scale`, 2 fill with `scale`
template <typename T>
__host__ __device__ inline int l2_seg_rule(int kind, double sumsq, T pmin, T pmax, long long L, T& scale) {
  const T nl2 = (T)sqrt(sumsq);
  scale = T(1);
  if (kind == SEGN_L2) {                                 // project_l2!.jl:8-13
    if (nl2 <= pmax) return 0;
    scale = pmax / nl2;
    return 1;
  }
  if (pmin <= nl2 && nl2 <= pmax) return 0;              // project_annulus!.jl:9-18
  if (nl2 > pmax) { scale = pmax / nl2; return 1; }
  if (nl2 < pmin && nl2 > T(0)) { scale = pmin / nl2; return 1; }
  if (nl2 < pmin && nl2 == T(0)) {                       // sigma_min ./ sqrt(length(x)): Float64 sqrt of an Int
    scale = (T)((double)pmin / sqrt((double)L));
    return 2;
  }
  return 0;
}

#if defined(__HIPCC__)
// Totals of a and b over the lanes that share a segment, returned to each of them.  `red`: 2 * BLOCK doubles.
__device__ __forceinline__ void segn_sum2(double& a, double& b, int F, double* red) {
  for (int o = F; o < 64; o <<= 1) {
    a += __shfl_xor(a, o, 64);
    b += __shfl_xor(b, o, 64);
  }
  const int lane = threadIdx.x & 63;
  red[threadIdx.x] = a;
  red[BLOCK + threadIdx.x] = b;
  __syncthreads();
  a = ((red[lane] + red[64 + lane]) + red[128 + lane]) + red[192 + lane];
  b = ((red[BLOCK + lane] + red[BLOCK + 64 + lane]) + red[BLOCK + 128 + lane]) + red[BLOCK + 192 + lane];
  __syncthreads();
}
__device__ __forceinline__ double segn_min(double a, int F, double* red) {
  for (int o = F; o < 64; o <<= 1) {
    const double w = __shfl_xor(a, o, 64);
    a = w < a ? w : a;
  }
  const int lane = threadIdx.x & 63;
  red[threadIdx.x] = a;
  __syncthreads();
  for (int w = 0; w < BLOCK / 64; ++w) a = red[64 * w + lane] < a ? red[64 * w + lane] : a;
  __syncthreads();
  return a;
}

// pass 1 of one tile: the sums of segment f over its lanes, returned to each of them; the values go to `sm` when the plan keeps them
template <typename T>
__device__ __forceinline__ void segn_pass1(const SegMap& m, const SegNormPlan& p, const T* vs, T* sm, bool live, int f, int r, int G,
                                           double* red, double& asum, double& sumsq, double& vmin) {
  const int F = p.F;
  const long long L = m.L;
  asum = 0; sumsq = 0; vmin = (double)INFINITY;
  if (live)
    for (long long t = r; t < L; t += G) {
      const T x = vs[seg_toff(m, t)];
      if (p.lds) sm[t * F + f] = x;
      const double a = (double)fabs(x);
      asum += a;
      sumsq += (double)x * (double)x;
      vmin = a < vmin ? a : vmin;
    }
  segn_sum2(asum, sumsq, F, red);
}

// VEC: rmin / rmax hold one radius per segment (rmin is read by the annulus only); otherwise every segment takes pmin / pmax
template <typename T, int KIND, bool VEC>
__global__ __launch_bounds__(BLOCK) void k_seg_norm(SegMap m, SegNormPlan p, T* __restrict__ v, T pmin, T pmax, const T* __restrict__ rmin,
                                                    const T* __restrict__ rmax) {
  static_assert(BLOCK == 256, "four waves: segn_sum2 adds four wave totals");
  extern __shared__ __align__(16) unsigned char segn_lds[];
  __shared__ double red[2 * BLOCK];
  T* const sm = reinterpret_cast<T*>(segn_lds);
  const int F = p.F, G = BLOCK >> p.logF;
  const int f = (int)threadIdx.x & (F - 1), r = (int)threadIdx.x >> p.logF;
  const long long L = m.L;
  for (long long tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
    long long base;
    const bool live = seg_tile_base(m, p, tile, f, base);
    T* const vs = v + base;
    if constexpr (VEC) {
      if (live) {
        const long long s = seg_tile_index(m, p, tile, f);
        pmax = rmax[s];
        if constexpr (KIND == SEGN_ANNULUS) pmin = rmin[s];
      }
    }
    // pass 1: the sums; the values go to LDS when they fit
    double asum, sumsq, vmin;
    segn_pass1<T>(m, p, vs, sm, live, f, r, G, red, asum, sumsq, vmin);
    int act = 0;                        // 0: inside the set, 1: soft threshold / multiply, 2: fill, 3: zero
    T par = T(0);                       // theta or the scale
    if constexpr (KIND == SEGN_L1) {
      vmin = segn_min(vmin, F, red);
      const double b = (double)pmax;
      const bool ball = !VEC || pmax > T(0);                  // a radius from device memory: <= 0 or NaN leaves {0} at most
      const bool need = live && ball && !((T)asum <= pmax);   // norm(v,1) <= b && return v   project_l1_Duchi!.jl:23
      L1SegState st = l1_seg_start(asum, b, L);
      st.done = need ? 0 : 1;
      for (long long it = 0; it <= L + 1; ++it) {
        if (__syncthreads_and(st.done)) break;
        double S = 0, C = 0;
        if (!st.done)
          for (long long t = r; t < L; t += G) {
            const double a = (double)fabs(p.lds ? sm[t * F + f] : vs[seg_toff(m, t)]);
            if (a > st.theta) { S += a; C += 1.0; }
          }
        segn_sum2(S, C, F, red);
        if (!st.done) l1_seg_step(st, S, C, b);
      }
      if (need) {
        act = 1;
        par = (T)l1_seg_finish(st, asum, vmin, b, L);
      } else if (VEC && live && !ball && asum > 0) {
        act = 3;
      }
    } else {
      if (live) act = l2_seg_rule<T>(KIND, sumsq, pmin, pmax, L, par);
    }
    // last pass: only segments outside their set are written
    if (act)
      for (long long t = r; t < L; t += G) {
        const long long o = seg_toff(m, t);
        const T x = p.lds ? sm[t * F + f] : vs[o];
        if constexpr (KIND == SEGN_L1) vs[o] = VEC && act == 3 ? T(0) : soft_thr(x, par);
        else vs[o] = act == 2 ? par : x * par;
      }
  }
}

// The norms of all segments: out[s] = (T)||segment s||_1 (NORM == SEGN_L1) or (T)sqrt(sum of squares) (SEGN_L2), s in SegMap's order.
// `p` is the projector's plan with lds = 0: one read pass, nothing kept.
template <typename T, int NORM>
__global__ __launch_bounds__(BLOCK) void k_seg_observe(SegMap m, SegNormPlan p, const T* __restrict__ v, T* __restrict__ out) {
  static_assert(BLOCK == 256, "four waves: segn_sum2 adds four wave totals");
  __shared__ double red[2 * BLOCK];
  const int F = p.F, G = BLOCK >> p.logF;
  const int f = (int)threadIdx.x & (F - 1), r = (int)threadIdx.x >> p.logF;
  for (long long tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
    long long base;
    const bool live = seg_tile_base(m, p, tile, f, base);
    double asum, sumsq, vmin;
    segn_pass1<T>(m, p, v + base, (T*)nullptr, live, f, r, G, red, asum, sumsq, vmin);
    if (live && r == 0) out[seg_tile_index(m, p, tile, f)] = NORM == SEGN_L1 ? (T)asum : (T)sqrt(sumsq);
  }
}
#endif

}  // namespace sipx
