// The l2,1 ball whose groups run across the equal-sized blocks of a stacked operator: { v : sum_p ||v_p||_2 <= tau } on the range of a
// caller-supplied sparse operator A = [A_0; A_1; ...; A_{B-1}] (SIPX_OP_CSC) whose B blocks have G rows each (ext_group.hip, BallProj,
// EXT_L21_STACKED).  With A the Hessian -- the named operator "Hessian" of the front end, B = 3 on a 2-D and B = 6 on a 3-D grid -- it
// is second-order isotropic total variation (TV^2, the bounded-Hessian regulariser): sum_p ||H x(p)||_F <= tau, whose null space is
// the affine functions.  Other stacked operators -- a projected gradient, [grad; alpha H] -- take the caller-supplied form.
// The rule of one group as __host__ __device__ functions (tests/l21_stacked/rule_driver.cpp runs them on the CPU); the kernels in
// ext_group.hip call nothing else for the arithmetic.  The reference package has no such projector.
//
// GROUPS.  The operator has M = B G rows, block q holding rows q G .. q G + G - 1, 1 <= B <= L21S_MAX_BLOCKS; M % B != 0 is refused.
//   Group p (p < G) is { v[q G + p] : q < B }.  Every position is a member: there are no grid coordinates and no pads (l21.h has both).
//   A zero row of A simply holds v = 0 and contributes nothing.
// RULE.  That of l21.h with these groups:
//   g_p     = (T) sqrt( sum_q (double)v[q G + p]^2 ), the float64 sum of squares taken in block order q = 0 .. B - 1 and rounded once to T
//             (l21s_group_norm, through l21_norm_of)
//   theta   = the threshold of the l1 ball of radius tau on the array g (G entries): the engine's own search (K<T>::proj_scalars_arr,
//             PX_L1)
//   the search's own decision ||g||_1 <= tau (ProjScalars::need == 0) leaves v unwritten: its bits stay, -0.0 included
//   otherwise v[q G + p] <- v[q G + p] * l21_weight(g_p, theta), in T
//   Float64: theta is re-evaluated on the search's active set in twice the working precision (l21_theta_refined through l21_tree_merge,
//   the kernels EXT_L21 runs: l21.h THRESHOLD IN FLOAT64).  Unlike a TV grid, whose last corner has g = 0, every group of a stacked
//   operator can be above theta; l21_theta_refined then returns the search's threshold, as l21.h says.
// No floating-point atomics, and no state but the warm start of the search: two calls give the same bits.
#pragma once
#include <stdexcept>
#include <string>

#include "l21.h"

namespace sipx {

constexpr int L21S_MAX_BLOCKS = 8;

// ---- the refusals of the set, worded once (set_config.h, the engine's stand-alone calls, the projector's own check; host.py repeats them) ----
constexpr const char* L21S_NEEDS_CSC = "the stacked l2,1 ball (l21_stacked) groups the rows of a caller-supplied sparse operator across its blocks: "
                                       "the operator must be SIPX_OP_CSC (custom_TD_OP, or the named \"Hessian\") -- on the built-in TV operator "
                                       "the set is (\"l21\", \"TV\")";
constexpr const char* L21S_WHOLE_ONLY = "the stacked l2,1 ball (l21_stacked) applies to the whole array (matrix / tensor mode): its groups are the "
                                        "rows p, G + p, 2 G + p, ... of the operator, fibers and slices have no meaning there";
constexpr const char* L21S_NO_TRANSFORM = "the stacked l2,1 ball (l21_stacked) takes no transform (DFT, DCT, wavelet): it acts on A x itself";
constexpr const char* L21S_NO_MINKOWSKI = "the stacked l2,1 ball (l21_stacked) takes no Minkowski component: custom operators have none";
constexpr const char* L21S_NO_VECTORS = "the stacked l2,1 ball (l21_stacked) takes no weights and no vectors (lb, ub): weights per group are not built";
constexpr const char* L21S_SHARDED = "the stacked l2,1 ball (l21_stacked) takes single-process contexts only, this one has a communicator, a slab "
                                     "decomposition or set ownership: its groups span the blocks of a caller-supplied operator -- use a single process";
constexpr const char* L21S_NO_COARSE = "multilevel: the stacked l2,1 ball (l21_stacked, (\"l21\", \"Hessian\")) is not built for PARSDMM_multi_level: "
                                       "solve on one level";
inline std::string l21s_bad_blocks(long long B) {
  return "the stacked l2,1 ball (l21_stacked): blocks = " + std::to_string(B) + ", the number of equal-sized blocks of the operator must be 1 .. " +
         std::to_string(L21S_MAX_BLOCKS);
}
inline std::string l21s_bad_rows(long long M, long long B) {
  return "the stacked l2,1 ball (l21_stacked): the operator has M = " + std::to_string(M) + " rows, not a multiple of blocks = " + std::to_string(B) +
         " -- every block needs the same number of rows (pad a shorter block with zero rows)";
}
// B and M of a descriptor; returns G, the number of groups
inline long long l21s_check_shape(long long M, long long B) {
  if (B < 1 || B > L21S_MAX_BLOCKS) throw std::runtime_error(l21s_bad_blocks(B));
  if (M < 1 || M % B != 0) throw std::runtime_error(l21s_bad_rows(M, B));
  if (M >= (1ll << 31)) throw std::runtime_error("the stacked l2,1 ball (l21_stacked): the operator needs fewer than 2^31 rows");
  return M / B;
}

// ---- the rule of one group ----------------------------------------------------------------------------------------------------------------
// where member q of group p lives
__host__ __device__ inline unsigned l21s_index(unsigned q, unsigned G, unsigned p) { return q * G + p; }
// one more member in the float64 sum of squares (block order)
template <typename T>
__host__ __device__ inline double l21s_add_square(double ss, T v) {
  return ss + l21_square<T>(v, true);
}
// g_p of group p of v (B blocks of G entries)
template <typename T>
__host__ __device__ inline T l21s_group_norm(const T* v, int B, unsigned G, unsigned p) {
  double ss = 0.0;
  for (int q = 0; q < B; ++q) ss = l21s_add_square<T>(ss, v[l21s_index((unsigned)q, G, p)]);
  return l21_norm_of<T>(ss);
}
// every member of a group is multiplied by l21_weight(g_p, theta) (l21.h)
template <typename T>
__host__ __device__ inline T l21s_scaled(T v, T f) { return v * f; }

}  // namespace sipx
