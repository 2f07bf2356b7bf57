// Group cardinality: the set { v = A x : at most k segments of v are non-zero } on the range of a one-block operator (identity, D_x, D_y,
// D_z), a segment being one fiber along a direction or one slice orthogonal to it (ext_group.hip, CardGroupsProj).  The non-convex
// counterpart of the l2,1 ball of l21_groups.h, as cardinality is that of the l1 ball.  The serial forms of the rule as __host__ __device__
// functions (tests/card_groups/rule_driver.cpp runs them on the CPU).  The reference package has no such projector.
//
// SEGMENTS.  make_segmap(spec) on the valid extents TD_n inside the padded grid (ext_family.h): nseg segments of L entries, in the order of
//   sipx_segment_norms and of l21_groups.  A pad entry (the far face of a difference operator) belongs to no segment: never read, never
//   written.
// RULE.
//   g_s     = the l2 norm of segment s as GroupNorms forms it for l21_groups, bit for bit (fibers: k_seg_observe<T, SEGN_L2>, the bits of
//             sipx_segment_norms; slices: the chunked compensated sums of l21_groups.h).  sipx_group_norms returns this array.
//   need    = #{s : g_s > 0} > k.  Without need nothing is written: v keeps its bits, -0.0 included.  k >= nseg is this case, and then
//             not one kernel is launched.
//   (tau, cut) = the k-th place of the stable descending order of g: magnitude descending, ties to the lower segment index.  tau = g at
//             that place (> 0 whenever need holds), cut = its segment index.  Segment s is kept iff cardg_keeps(g_s, s, tau, cut):
//             g_s > tau || (g_s == tau && s <= cut) -- card_keeps of ext_transform.hip, PX_CARD's rule of sipx_device.h.
//             Without need: tau = 0, cut = CARDG_NO_CUT, as the engine's search leaves them.
//   apply   a kept segment is not touched, neither read nor written; every entry of a dropped segment is written +0 without a read of v.
// SELECTION.  Two routes, one result (need, tau, cut), held in the need / tau / quota of a ProjScalars<T>:
//   search  the engine's cardinality search on g (K<T>::proj_scalars_arr, PX_CARD, len = true_len = nseg) with a SearchState of the
//           projector's own: exact, stable and tie-safe for any nseg (tests/card_exact.py states the contract)
//   small   k_cardg_rank, nseg <= CARDG_SMALL_MAX: one workgroup stages g in LDS, the thread of segment s counts
//           r_s = #{t : g_t > g_s || (g_t == g_s && t < s)} -- the place of s in the stable order, a permutation of 0 .. nseg - 1 -- and
//           the one segment with r_s == k - 1 writes tau = g_s, cut = s.  cardg_rank_of / cardg_select_by_rank below are its serial form.
//           One launch where the search is a dozen dependent ones; its nseg^2 comparisons bound it from above (measured
//           0.04 against 0.39 ms at 8 and 64 segments, 0.07 against 0.25 at 1024, 0.67 against 0.22 at 4096 with four segments a thread).
// No floating-point atomics, no state that changes the result: two calls give the same bits.
#pragma once
#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>

#ifndef __host__      // a plain host compiler (the rule driver); the library's units include the HIP headers first
#define __host__
#define __device__
#endif

namespace sipx {

// ---- the refusals of the set, worded once (set_config.h, the engine's stand-alone calls, the projector's own check; host.py repeats them) ----
constexpr const char* CARDG_NEEDS_MODE = "group cardinality (card_groups) needs a fiber or slice mode: on the whole array it has one group, which "
                                         "every k >= 1 keeps -- drop the set, or count entries with the cardinality set";
constexpr const char* CARDG_2D_SLICE = "for 2D models, the mode of application for card_groups sets needs to be (fiber,x) or (fiber,z)";
constexpr const char* CARDG_ONE_BLOCK = "group cardinality (card_groups) counts the fibers or slices of the range of a one-block operator: TD_OP "
                                        "must be the identity, D_x, D_y or D_z (on TV or a custom operator use the cardinality set, which counts "
                                        "entries)";
constexpr const char* CARDG_NO_TRANSFORM = "group cardinality (card_groups) takes no transform (DFT, DCT, wavelet): it acts on A x itself -- use "
                                           "the cardinality set behind the transform, which counts coefficients";
constexpr const char* CARDG_NO_MINKOWSKI = "group cardinality (card_groups) takes no Minkowski component: constrain the sum of the components";
constexpr const char* CARDG_NO_VECTORS = "group cardinality (card_groups) takes one k for the whole array and no lb / ub / weights: a segment is kept "
                                         "or dropped whole -- for weights per segment use the l21_groups set";
constexpr const char* CARDG_NO_SET_DATA = "group cardinality (card_groups) holds no vectors to replace: k is fixed when the set is added -- build a "
                                          "new context for another k";
constexpr const char* CARDG_SHARDED = "group cardinality (card_groups) takes single-process contexts only, this one has a communicator, a slab "
                                      "decomposition or set ownership: its segments compete for k places across the whole array -- use a "
                                      "single process";
constexpr const char* CARDG_BAD_K = "group cardinality (card_groups) needs an integer k >= 1, the number of fibers or slices kept (k = 0 is the "
                                    "zero array: use bounds)";
constexpr const char* CARDG_K_INEXACT = "group cardinality (card_groups): a k below the number of segments must be exactly representable in the "
                                        "working precision, since the search reads k from it -- Float32: k <= 2^24; use Float64";
constexpr const char* CARDG_TOO_LARGE = "group cardinality (card_groups): the grid needs fewer than 2^31 points -- split the array";

constexpr int CARDG_SMALL_MAX = 1024;                      // most segments of the small route: one a thread, T[CARDG_SMALL_MAX] of LDS, nseg comparisons each
constexpr long long CARDG_NO_CUT = 0x7fffffffffffffffll;   // the cut where nothing is dropped (ProjScalars::quota as k_card_decide leaves it)

// k as the descriptor carries it (pmax, a double) for a set of nseg segments in precision T
template <typename T>
inline void cardg_check_k(double k, long long nseg) {
  if (!(k >= 1.0) || !(k < INFINITY) || k != std::floor(k)) throw std::runtime_error(CARDG_BAD_K);
  if (k < (double)nseg && (double)(T)k != k) throw std::runtime_error(CARDG_K_INEXACT);
}

template <typename T>
struct CardGSel {
  int need;
  T tau;
  long long cut;
};

template <typename T>
__host__ __device__ inline bool cardg_keeps(T g, long long s, T tau, long long cut) { return g > tau || (g == tau && s <= cut); }

// The serial rule: need, then tau = the largest value with #{g_s >= tau} >= k by bisection on the bit pattern (monotone for the
// non-negative numbers g holds), then the cut among the segments equal to tau, lowest indices first.
template <typename T>
__host__ __device__ inline CardGSel<T> cardg_select_serial(const T* g, long long nseg, long long k) {
  CardGSel<T> r{0, T(0), CARDG_NO_CUT};
  long long nnz = 0;
  for (long long s = 0; s < nseg; ++s) nnz += g[s] > T(0) ? 1 : 0;
  if (k >= nseg || nnz <= k) return r;
  r.need = 1;
  unsigned long long ans = 0;
  const int bits = (int)sizeof(T) * 8;
  for (int bit = bits - 2; bit >= 0; --bit) {                // (the sign bit is 0)
    const unsigned long long cand = ans | (1ull << bit);
    long long c = 0;
    for (long long s = 0; s < nseg; ++s) {
      unsigned long long key = 0;
      memcpy(&key, &g[s], sizeof(T));                        // (little endian: the low bytes)
      c += (g[s] == g[s] && key >= cand && !(key >> (bits - 1))) ? 1 : 0;
    }
    if (c >= k) ans = cand;
  }
  memcpy(&r.tau, &ans, sizeof(T));
  long long above = 0;
  for (long long s = 0; s < nseg; ++s) above += g[s] > r.tau ? 1 : 0;
  long long quota = k - above;                               // segments equal to tau that stay (>= 1)
  for (long long s = 0; s < nseg; ++s)
    if (g[s] == r.tau && --quota == 0) { r.cut = s; break; }
  return r;
}

// The small route's rule: the place of segment s in the stable descending order
template <typename T>
__host__ __device__ inline long long cardg_rank_of(const T* g, long long nseg, long long s) {
  const T gs = g[s];
  long long r = 0;
  for (long long t = 0; t < nseg; ++t) r += (g[t] > gs || (g[t] == gs && t < s)) ? 1 : 0;
  return r;
}
template <typename T>
__host__ __device__ inline CardGSel<T> cardg_select_by_rank(const T* g, long long nseg, long long k) {
  CardGSel<T> r{0, T(0), CARDG_NO_CUT};
  long long nnz = 0;
  for (long long s = 0; s < nseg; ++s) nnz += g[s] > T(0) ? 1 : 0;
  if (k >= nseg || nnz <= k) return r;
  for (long long s = 0; s < nseg; ++s)
    if (cardg_rank_of<T>(g, nseg, s) == k - 1) { r.need = 1; r.tau = g[s]; r.cut = s; }
  return r;
}

// keep[s] (nseg entries) <- 1 where segment s stays
template <typename T>
__host__ __device__ inline void cardg_kept(const T* g, long long nseg, const CardGSel<T>& sel, unsigned char* keep) {
  for (long long s = 0; s < nseg; ++s) keep[s] = (!sel.need || cardg_keeps<T>(g[s], s, sel.tau, sel.cut)) ? 1 : 0;
}

}  // namespace sipx
