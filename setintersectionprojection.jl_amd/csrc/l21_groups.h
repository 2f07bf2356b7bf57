// Group sparsity over fibers or slices: the ball { v = A x : sum_s w_s ||v[segment s]||_2 <= tau } on the range of a one-block operator
// (identity, D_x, D_y, D_z), a group being one fiber along a direction or one slice orthogonal to it (ext_group.hip, GroupsProj).  The plan
// of the norms launch and the serial form of the rule as __host__ __device__ functions (tests/l21_groups/rule_driver.cpp runs them on the
// CPU); the threshold and the factor are those of l21_weighted.h, unchanged.  The reference package has no such projector.
//
// SEGMENTS.  make_segmap(spec) on the valid extents TD_n inside the padded grid (ext_family.h): nseg segments of L entries, in the order of
//   sipx_segment_norms and of the per-segment radii.  A pad entry (the far face of a difference operator) enters no sum and is never
//   written, whatever it holds.
// RULE.
//   g_s     = (T) sqrt( sum_t (double)v_{s,t}^2 ), a float64 sum in a fixed order that depends on (grid, op, mode, dir, T) alone, rounded once
//             fibers: segn_pass1's order (seg_norm.h, k_seg_observe<T, SEGN_L2>) -- g is sipx_segment_norms(..., l2) bit for bit
//             slices: the chunked order of PLAN below, every sum an unevaluated pair of doubles (L21Sum of l21.h: the rounding error of
//             every addition kept, for T = double that of every square too), so a slice of 10^6 entries is summed as exactly as one of 10
//   w_s     = the weight as given when it is > 0 and finite, 0 otherwise (l21w_clean); no weights: every w_s = 1, and the bits are those
//             of the set built with a vector of ones
//   theta   = the weighted Michelot iteration of l21_weighted.h on (g, w) with n = nseg: l21w_add, l21w_active, l21w_start, l21w_step, the
//             sums in twice the working precision; (T)asum <= tau leaves v unwritten.  NOT the engine's l1 search: that carries the
//             reference's `rho + 1 < lv` cap, which thresholds with (S - min - tau) / (n - 1) when every entry stays active -- here the
//             common case (g = (3, 4, 5), tau = 6: theta = 2 and (1, 2, 3); the capped rule gives 1.5 and a sum of 7.5, outside the ball)
//   apply   v_{s,t} <- v_{s,t} * f_s in T, f_s = l21w_factor(g_s, w_s, theta): g_s == theta w_s zeroes the group, g_s == 0 multiplies by 0,
//             w_s == 0 leaves the segment unwritten, bits and -0.0 included
// PLAN (slices).  seg_norm.h gives a slice to one workgroup; here every slice is cut into chunks of `chunk` consecutive element indices t
//   (the last one may be shorter), L21G_CHUNK_BYTES of one workgroup's reads.  A workgroup owns one (tile, chunk): the tile is one slice
//   whose elements are contiguous along x (slice y, slice z: F = 1, a thread takes VW = 16 bytes of consecutive t, then strides), or F
//   neighbouring slices along x (slice x: lanes run along the slice index first, as in seg_norm.h).  Its sum: serial per thread in
//   ascending t, then the halving tree of l21_tree_merge restricted to the lanes of one slice; the partial goes to part[2 (s nchunk + c)].
//   A second kernel merges a slice's partials in ascending c and writes g_s.  The 16-byte and the scalar path give every thread the same
//   elements in the same order: the same arithmetic.
// No floating-point atomics, no state between calls: the feasibility estimate and the y update take the same path, two calls give the
// same bits.
#pragma once
#include <stdexcept>
#include <string>

#include "l21_weighted.h"
#include "seg_norm.h"

namespace sipx {

// ---- the refusals of the set, worded once (set_config.h, the engine's stand-alone calls, the projector's own check) --------------------
constexpr const char* L21G_ONE_BLOCK = "the l2,1 ball over fibers or slices (l21_groups) groups the range of a one-block operator: TD_OP must "
                                       "be the identity, D_x, D_y or D_z (on TV use the l21 sets, whose groups are the grid points)";
constexpr const char* L21G_NEEDS_MODE = "the l2,1 ball over fibers or slices (l21_groups) needs a fiber or slice mode: on the whole array it has "
                                        "one group and is the l2 ball -- use the l2 set";
constexpr const char* L21G_2D_SLICE = "for 2D models, the mode of application for l21_groups sets needs to be (fiber,x) or (fiber,z)";
constexpr const char* L21G_NO_TRANSFORM = "the l2,1 ball over fibers or slices (l21_groups) takes no transform: it acts on A x itself";
constexpr const char* L21G_NO_MINKOWSKI = "the l2,1 ball over fibers or slices (l21_groups) takes no Minkowski component";
constexpr const char* L21G_SHARDED = "the l2,1 ball over fibers or slices (l21_groups) takes single-process contexts only, this one has a "
                                     "communicator, a slab decomposition or set ownership: its segments compete for one budget across the "
                                     "whole array -- use a single process";

// the descriptor: lb = one weight per segment or NULL, never ub; `given`: the entries the descriptor says lb holds
inline void l21g_check_desc(bool has_lb, bool has_ub, long long given, long long nseg, bool fiber, int dir, const long long* dims) {
  if (has_ub) throw std::runtime_error("the l2,1 ball over fibers or slices (l21_groups) takes weights in lb and no ub: the radius is pmax");
  if (has_lb && given != nseg)
    throw std::runtime_error("the weighted l2,1 ball (l21_groups): " + std::to_string(given) + " weights given, " + std::to_string(nseg) +
                             " are needed -- one per segment, a segment being a " + (fiber ? "fiber along" : "slice orthogonal to") +
                             " dimension " + std::to_string(dir + 1) + " of the array of shape (" + std::to_string(dims[0]) + ", " +
                             std::to_string(dims[1]) + ", " + std::to_string(dims[2]) + ") (TD_n)");
}

// ---- the plan of the norms launch -------------------------------------------------------------------------------------------------
constexpr int L21G_CHUNK_BYTES = 20 * 1024;      // one workgroup's reads of a chunk: 80 bytes per thread

struct L21GroupsPlan {
  int slices;                 // 0: fibers, one launch of k_seg_observe with `fiber`; 1: the chunked route
  SegNormPlan fiber;          // fibers: seg_norm_plan with nothing resident
  int F, logF;                // slices: slices per tile (slice x), 1 otherwise
  int vw;                     // slices: consecutive t a thread takes before it strides (16 bytes when F == 1, one entry in a tile)
  long long chunk, nchunk;    // slices: element indices per chunk, chunks per slice
  long long ntA;              // slices: tiles
  long long grid;             // workgroups of the norms launch: ntA * nchunk (slices), fiber.grid (fibers)
  __host__ __device__ long long t0(long long c) const { return c * chunk; }
  __host__ __device__ long long t1(long long c, long long L) const { return (c + 1) * chunk < L ? (c + 1) * chunk : L; }
};

__host__ __device__ inline L21GroupsPlan l21_groups_plan(const SegMap& m, int mode, int elem_bytes) {
  L21GroupsPlan p{};
  if (mode != SIPX_MODE_SLICE) {
    p.fiber = seg_norm_plan(m, elem_bytes);
    p.fiber.lds = 0;
    p.fiber.lds_bytes = 0;
    p.F = 1; p.vw = 1; p.chunk = m.L; p.nchunk = 1; p.ntA = m.nseg;
    p.grid = p.fiber.grid;
    return p;
  }
  p.slices = 1;
  const SegNormPlan t = seg_norm_plan(m, elem_bytes);      // (the tile of seg_norm.h: F > 1 where neighbouring slices are contiguous)
  p.F = t.F; p.logF = t.logF;
  p.vw = p.F == 1 ? 16 / elem_bytes : 1;
  p.chunk = (long long)L21G_CHUNK_BYTES / elem_bytes / p.F;
  p.nchunk = (m.L + p.chunk - 1) / p.chunk;
  if (p.nchunk < 1) p.nchunk = 1;
  p.ntA = (m.nseg + p.F - 1) / p.F;
  p.grid = p.ntA * p.nchunk;
  return p;
}

// one entry enters a slice's sum of squares (T = double: with the rounding error of the square)
template <typename T>
__host__ __device__ inline void l21g_add_square(L21Sum& acc, T x) {
  l21w_add_product<T>(acc, (double)x, (double)x);
}
// g_s from the merged partials of a slice
template <typename T>
__host__ __device__ inline T l21g_norm_of(const L21Sum& s) {
  return (T)sqrt(s.hi + s.lo);
}

// The whole rule serially on the segment norms: the search of l21_weighted.h on (g, w) -- w == nullptr: every weight 1 -- and the factors.
// Returns need as l21w_search_serial does; f[s] (nseg entries) is the factor of segment s, 1 where need == 0 or the weight is 0.
template <typename T>
inline int l21g_rule_serial(const T* g, const T* w, long long nseg, T tau, T& theta_T, double& asum, int& passes, T* f) {
  const T* ww = w;
  T* ones = nullptr;
  if (!w) {
    ones = new T[(size_t)(nseg > 0 ? nseg : 1)];
    for (long long s = 0; s < nseg; ++s) ones[s] = T(1);
    ww = ones;
  }
  const int need = l21w_search_serial<T>(g, ww, nseg, tau, theta_T, asum, passes);
  for (long long s = 0; s < nseg; ++s) {
    const T ws = l21w_clean<T>(ww[s]);
    f[s] = (need == 1 && ws > T(0)) ? l21w_factor<T>(g[s], ws, theta_T) : T(1);
  }
  delete[] ones;
  return need;
}

}  // namespace sipx
