// The l2,0 sets on total variation: { v = TV x : at most k grid points p carry a non-zero gradient vector v_p } on the range of the TV /
// TV_xy operator (ext_group.hip, L20Proj and L20FrameProj) -- L0 gradient smoothing, a piecewise-constant model with at most k edge points
// whose edges keep their contrast.  The non-convex counterpart of the l2,1 balls of l21.h / l21_seg.h / l21_joint.h, as card_groups.h is that
// of l21_groups.h.  ("cardinality", "TV") is another set: it counts differences, so a diagonal edge costs two and it prefers staircases.
// The serial forms of the rule as __host__ __device__ functions of a header that needs no HIP header (tests/l20/rule_driver.cpp runs them
// on the CPU).  The reference package has no such projector.
//
// GROUPS.  Those of l21.h -- the group of grid point p holds the forward differences that START at p, 0 to ndim members, none at the last
//   corner -- and, for the joint set, those of l21_joint.h: the group of pixel (i, j) holds the differences that start at (i, j, k) in every
//   frame k.  A row a block does not have is a pad: never read for its value, never written (l20_member is l21_member).
// FORMS.   EXT_L20        ("l20", TV | TV_xy), whole array: one budget k over the N grid points, index = the column-major point index
//          EXT_L20_SEG    ("l20", TV_xy, ("slice", "z")): every frame has its own budget k or k[frame] over its L = n1 n2 pixels,
//                         index = the in-frame pixel index
//          EXT_L20_JOINT  ("l20_joint", TV_xy): one budget k over the L pixels, index = the pixel index; one common edge set for all frames
// RULE.
//   g_p     = the key: the group norm formed by the launch the convex set uses, bit for bit -- k_l21_norms (l20_key below is its serial
//             form, l21_group_norm), k_l21j_norms / k_l21j_finish with the chunk plan of l21_joint.h for the joint set.
//             sipx_tv_group_norms returns this array.
//   need    = #{p : g_p > 0} > k.  Without need nothing is written: v keeps its bits, -0.0 included.  k >= the number of groups is this
//             case, and then not one kernel is launched.
//   (tau, cut) = the k-th place of the stable descending order of g: magnitude descending, ties to the lower group index.  Group p is
//             kept iff cardg_keeps(g_p, p, tau, cut): g_p > tau || (g_p == tau && p <= cut), PX_CARD's rule.  tau > 0 whenever need holds,
//             so a group of norm 0 counts as dropped (it is written +0, which it is already up to the sign of a zero).
//   apply   a kept group is neither read nor written; every member of a dropped group is written +0 without a read of v.
// SELECTION.  Whole array and joint: CardgSelect of ext_group.hip, the very selection of card_groups.h (k_cardg_rank up to CARDG_SMALL_MAX
//   groups, the engine's cardinality search above).  Per frame: k_l20_frames, one workgroup per frame -- the count of the non-zero keys, a
//   radix select on the bit pattern of g (g >= 0, so the pattern is monotone), 8 bits a pass, then the cut among the keys equal to tau:
//   the last of them where all of them stay, otherwise one ordered pass; l20_frame_select below is its serial form.
// No floating-point atomics, nothing kept between calls that changes the result: two calls give the same bits.
#pragma once
#include "card_groups.h"

namespace sipx {

// ---- the refusals of the sets, worded once (set_config.h, the engine's stand-alone calls, the projectors' own checks; host.py repeats them) ----
constexpr const char* L20_NEEDS_TV = "the l2,0 set (l20) counts the gradient vectors of the TV operator: TD_OP must be TV (D2D, D3D) or TV_xy, not a "
                                     "one-block or custom operator (there use the cardinality set, which counts entries, or card_groups)";
constexpr const char* L20_JOINT_ROUTE = "the joint l2,0 set (l20_joint) needs the TV_xy operator of a 3-D grid in tensor mode: its groups span "
                                        "the frames -- for one budget over all grid points use (\"l20\", \"TV_xy\"), per frame (\"l20\", \"TV_xy\", "
                                        "(\"slice\", \"z\"))";
constexpr const char* L20_MODES = "the l2,0 set (l20) applies to the whole array (matrix / tensor mode), or per frame as (\"slice\", \"z\") on TV_xy: "
                                  "fiber modes and other slices have no gradient groups -- use card_groups on D_x, D_y or D_z there";
constexpr const char* L20_NO_TRANSFORM = "the l2,0 set (l20, l20_joint) takes no transform (DFT, DCT, wavelet): it acts on TV x itself -- use the "
                                         "cardinality set behind the transform, which counts coefficients";
constexpr const char* L20_NO_MINKOWSKI = "the l2,0 set (l20, l20_joint) takes no Minkowski component: constrain the sum of the components";
constexpr const char* L20_NO_WEIGHTS = "the l2,0 set (l20, l20_joint) takes no weights and no lb: a group is kept or dropped whole by its plain "
                                       "norm -- for weighted groups use the l21 set with weights";
constexpr const char* L20_K_VECTOR = "the l2,0 set (l20) takes one k, or per frame -- (\"slice\", \"z\") on TV_xy -- a vector of n3 integers in max; "
                                     "every other form has one budget: pass a scalar";
constexpr const char* L20_NO_SET_DATA = "the l2,0 set (l20, l20_joint) built with a scalar k holds no vectors to replace -- build the per-frame "
                                        "set with a vector of n3 budgets to replace them, or a new context for another k";
constexpr const char* L20_SET_DATA_UB = "the l2,0 set (l20) per frame: the budgets are its ub, n3 integers >= 1; it has no lb";
constexpr const char* L20_SHARDED = "the l2,0 set (l20, l20_joint) takes single-process contexts only, this one has a communicator, a slab "
                                    "decomposition or set ownership: its groups span the blocks of TV and compete for k places across the "
                                    "whole array -- use a single process";
constexpr const char* L20_NO_COARSE = "multilevel: the l2,0 set (l20, l20_joint) has no rule that takes k to a grid with another number of "
                                      "points -- solve on one level";
constexpr const char* L20_BAD_K = "the l2,0 set (l20, l20_joint) needs an integer k >= 1, the number of grid points that may carry a gradient "
                                  "(k = 0 is the constant array: use bounds on TV)";
constexpr const char* L20_K_INEXACT = "the l2,0 set (l20, l20_joint): a k below the number of groups must be exactly representable in the "
                                      "working precision, since the search reads k from it -- Float32: k <= 2^24; use Float64";
constexpr const char* L20_TOO_LARGE = "the l2,0 set (l20, l20_joint): the grid needs fewer than 2^31 points -- split the array";

// k as the descriptor carries it (pmax, a double, or one entry of the per-frame vector) for a set of ngroups groups in precision T
template <typename T>
inline void l20_check_k(double k, long long ngroups) {
  if (!(k >= 1.0) || !(k < INFINITY) || k != std::floor(k)) throw std::runtime_error(L20_BAD_K);
  if (k < (double)ngroups && (double)(T)k != k) throw std::runtime_error(L20_K_INEXACT);
}
// the per-frame budgets, T[nframes] (sipx_add_set, sipx_set_data from host memory)
template <typename T>
inline void l20_check_k_vector(const T* k, long long nframes, long long L) {
  for (long long f = 0; f < nframes; ++f) l20_check_k<T>((double)k[f], L);
}

// ---- membership and the key of one group: l21_member / l21_group_norm of l21.h, which the kernels call -------------------------------------
__host__ __device__ inline bool l20_member(int cd, int nd) { return cd < nd - 1; }
template <typename T>
__host__ __device__ inline T l20_key(const T* v, const bool* member, int nblk) {
  double ss = 0.0;
  for (int q = 0; q < nblk; ++q) ss += member[q] ? (double)v[q] * (double)v[q] : 0.0;
  return (T)std::sqrt(ss);
}

// ---- need / tau / cut over an array of keys: the whole-array and the joint form -------------------------------------------------------------
template <typename T>
__host__ __device__ inline CardGSel<T> l20_select_serial(const T* g, long long n, long long k) { return cardg_select_serial<T>(g, n, k); }

// ---- one frame, as k_l20_frames selects: count, radix select on the bit pattern (8 bits a pass, most significant first), ordered cut --------
template <typename T>
__host__ __device__ inline unsigned long long l20_bits(T g) {
  unsigned long long key = 0;
  memcpy(&key, &g, sizeof(T));                               // (little endian: the low bytes; g >= 0: the pattern is monotone)
  return key;
}
template <typename T>
__host__ __device__ inline CardGSel<T> l20_frame_select(const T* g, long long L, long long k) {
  CardGSel<T> r{0, T(0), CARDG_NO_CUT};
  long long nnz = 0;
  for (long long t = 0; t < L; ++t) nnz += g[t] > T(0) ? 1 : 0;
  if (k >= L || nnz <= k) return r;
  r.need = 1;
  unsigned long long prefix = 0, mask = 0;
  long long kk = k;
  for (int shift = (int)sizeof(T) * 8 - 8; shift >= 0; shift -= 8) {
    long long hist[256];
    for (int b = 0; b < 256; ++b) hist[b] = 0;
    for (long long t = 0; t < L; ++t) {
      const unsigned long long key = l20_bits<T>(g[t]);
      if ((key & mask) == prefix) ++hist[(key >> shift) & 255ull];
    }
    long long cum = 0;
    int b = 255;
    for (; b > 0; --b) {
      if (cum + hist[b] >= kk) break;
      cum += hist[b];
    }
    prefix |= (unsigned long long)b << shift;
    kk -= cum;
    mask |= 255ull << shift;
  }
  memcpy(&r.tau, &prefix, sizeof(T));                        // the k-th largest key; kk of the keys equal to it stay, the earliest ones
  for (long long t = 0; t < L; ++t)
    if (l20_bits<T>(g[t]) == prefix && --kk == 0) { r.cut = t; break; }
  return r;
}

// keep[p] (n entries) <- 1 where group p stays
template <typename T>
__host__ __device__ inline void l20_kept(const T* g, long long n, const CardGSel<T>& sel, unsigned char* keep) { cardg_kept<T>(g, n, sel, keep); }

}  // namespace sipx
