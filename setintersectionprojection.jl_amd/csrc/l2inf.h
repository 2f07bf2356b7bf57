// Pointwise bounds on the group norms: the l2,inf ball { v : ||v_p||_2 <= c_p for every group p } on the range of the TV / TV_xy operator
// (an isotropic slope constraint: nowhere steeper than c_p, whatever the direction of the edge), across the frames of TV_xy, or across
// the equal-sized blocks of a caller-supplied stacked operator such as the Hessian (a pointwise curvature bound).  It is the isotropic
// counterpart of ("bounds", "TV"), which bounds every difference direction on its own, and the dual ball of the l2,1 ball of l21.h.
// The rule of one group as __host__ __device__ functions (tests/l2inf/rule_driver.cpp runs them on the CPU); the kernels in
// ext_group.hip (L2InfProj) call nothing else for the arithmetic.  The reference package has no such projector.
//
// GROUPS.  EXT_L2INF on TV / TV_xy: those of l21.h, one per grid point (l21_member).  EXT_L2INF_JOINT on TV_xy: those of l21_joint.h, one per
//   pixel across all frames, summed by its plan.  EXT_L2INF_STACKED: those of l21_stacked.h, group p < G = M / B being { v[q G + p] : q < B }.
// BOUND.  c is one positive number (pmax), or one number >= 0 per group in ub, in group order: N grid points (the order of
//   sipx_tv_group_norms), n1 n2 pixels, or G rows.  +inf leaves a group free, 0 flattens it.  The entry of a group without a member (the
//   last corner of a grid) is never looked at by the host check and changes nothing on the device.  A NaN that reaches the device in a
//   vector handed over in device memory leaves its group free.
// RULE.
//   g_p     = l21_norm_of of the float64 sum of squares of the members in block order (l21.h, l21_joint.h, l21_stacked.h), bit for bit
//             what the norms kernel of the l2,1 ball on the same operator writes
//   g_p <= c_p, compared in T (l2inf_clipped false): the group keeps its bits, -0.0 included; a thread none of whose groups is
//             clipped stores nothing
//   otherwise every member is multiplied by f_p = c_p / g_p, the quotient and the products in T (l2inf_factor, l2inf_scaled)
//   rows a block does not have are never written
// There is no threshold and no search: nothing is kept between calls, there are no floating-point atomics, two calls give the same bits.
//
// HOW FAR THE OUTPUT MAY EXCEED THE BOUND.  u = eps / 2 the unit roundoff of T, m the members of a group.  Barring overflow and underflow:
//   g = ||v|| (1 + dg), |dg| <= kg u, with kg = 1 + m 2^-28 for Float32 (the squares are exact in float64, its sum and square root round
//       at 2^-53, the one rounding to T counts) and kg = 1 + m / 2 for Float64 (m roundings of the sum of squares, halved by the root,
//       and the root's own)
//   f = (c / g)(1 + df), |df| <= u;   every product v_q f rounds once more, |dq| <= u
//   so the exact norm of the output is at most c (1 + u)^2 / (1 - kg u) <= c (1 + (kg + 2) u) to first order, and the norm the
//   projector's own norms kernel OBSERVES on it (sipx_l2inf_norm) carries kg u once more:
//       g(P v) <= c (1 + l2inf_excess_units(m) u),   l2inf_excess_units(m) = 2 kg + 2 (+ 0.01 for the second-order terms)
//   -- 4 u c, at most 4 ulps of c, for Float32; (m + 4) u c for Float64.  An entry of the output differs from c v_q / ||v|| by at most
//   (kg + 2) u |P v|_q: 1.5 eps for Float32, (m / 4 + 1.5) eps for Float64, within the 4 eps the l2,1 family is held to up to m = 8.
//   An unclipped group is observed at its own g <= c exactly.
#pragma once
#include <cmath>
#include <stdexcept>
#include <string>

#include "l21.h"

namespace sipx {

// ---- the refusals of the sets, worded once (set_config.h, the engine's stand-alone calls, the projector's own check; host.py repeats them) ----
constexpr const char* L2INF_NEEDS_TV = "the l2,inf ball (l2inf) bounds the gradient magnitude at every grid point: TD_OP must be TV (D2D, D3D), TV_xy "
                                       "or the named \"Hessian\" -- a bound on one difference direction is (\"bounds\", \"D_z\"), a caller-supplied "
                                       "stacked operator takes (\"l2inf_stacked\", name, 0, c, mode, custom_TD_OP=(A, False), blocks=B)";
constexpr const char* L2INF_JOINT_ROUTE = "the joint l2,inf ball (l2inf_joint) groups the frames of TV_xy: TD_OP must be TV_xy, mode tensor -- per "
                                          "frame bounds are (\"l2inf\", \"TV_xy\")";
constexpr const char* L2INF_STACKED_NEEDS_CSC = "the stacked l2,inf ball (l2inf_stacked) groups the rows of a caller-supplied sparse operator across its "
                                                "blocks: the operator must be SIPX_OP_CSC (custom_TD_OP, or the named \"Hessian\") -- on the built-in TV "
                                                "operator the set is (\"l2inf\", \"TV\")";
constexpr const char* L2INF_MIN = "the l2,inf ball (l2inf, l2inf_joint, l2inf_stacked) bounds the group norms from above only: min must be 0 -- a lower "
                                  "bound on the gradient magnitude is not convex and not built";
constexpr const char* L2INF_BAD_C = "the l2,inf ball (l2inf, l2inf_joint, l2inf_stacked) needs a bound c > 0 as a scalar (c = 0 is the constant array: "
                                    "use bounds on TV, or a vector of zeros to flatten chosen points)";
constexpr const char* L2INF_MODES = "the l2,inf ball (l2inf, l2inf_joint, l2inf_stacked) applies to the whole array (matrix / tensor mode), fibers and "
                                    "slices are not built: (\"slice\", \"z\") on TV_xy is the vector form with c constant within every frame -- pass "
                                    "max = np.repeat(c_frames, n1 * n2)";
constexpr const char* L2INF_NO_TRANSFORM = "the l2,inf ball (l2inf, l2inf_joint, l2inf_stacked) takes no transform (DFT, DCT, wavelet): it acts on the "
                                           "differences of x themselves";
constexpr const char* L2INF_NO_WEIGHTS = "the l2,inf ball (l2inf, l2inf_joint, l2inf_stacked) takes no weights (lb): a weight per group is its bound, pass "
                                         "the vector of bounds as max (ub)";
constexpr const char* L2INF_NO_MINKOWSKI = "the l2,inf ball (l2inf, l2inf_joint, l2inf_stacked) takes no Minkowski component: bound the sum itself";
constexpr const char* L2INF_SHARDED = "the l2,inf ball (l2inf, l2inf_joint, l2inf_stacked) takes single-process contexts only, this one has a "
                                      "communicator, a slab decomposition or set ownership: its groups span the blocks of the operator -- use "
                                      "(\"bounds\", \"TV\"), or a single process";
constexpr const char* L2INF_NO_COARSE = "multilevel: the l2,inf ball (l2inf, l2inf_joint, l2inf_stacked) is not built for PARSDMM_multi_level: a bound on "
                                        "the gradient magnitude does not carry over to a coarser grid unchanged -- solve on one level";
constexpr const char* L2INF_NO_SET_DATA = "this l2,inf set was built with a scalar bound, which is fixed at sipx_add_set: build it with a vector of bounds "
                                          "(ub) to replace them in a live context";
inline std::string l2inf_bad_length(long long given, long long groups) {
  return "the l2,inf ball (l2inf, l2inf_joint, l2inf_stacked): the vector of bounds has " + std::to_string(given) + " entries, the set has " +
         std::to_string(groups) + " groups (one bound per grid point, per pixel of the joint set, or per row of one block)";
}
inline std::string l2inf_bad_entry(long long p) {
  return "the l2,inf ball (l2inf, l2inf_joint, l2inf_stacked): bound " + std::to_string(p) +
         " is negative or NaN -- every bound must be >= 0 (+inf leaves a point free, 0 flattens it)";
}

inline std::string l2inf_bad_blocks(long long B) {
  return "the stacked l2,inf ball (l2inf_stacked): blocks = " + std::to_string(B) + ", the number of equal-sized blocks of the operator must be 1 .. 8";
}
inline std::string l2inf_bad_rows(long long M, long long B) {
  return "the stacked l2,inf ball (l2inf_stacked): the operator has M = " + std::to_string(M) + " rows, not a multiple of blocks = " + std::to_string(B) +
         " -- every block needs the same number of rows (pad a shorter block with zero rows)";
}
// B and M of a stacked descriptor, the limits of l21_stacked.h (L21S_MAX_BLOCKS = 8); returns G, the number of groups
inline long long l2infs_check_shape(long long M, long long B) {
  if (B < 1 || B > 8) throw std::runtime_error(l2inf_bad_blocks(B));
  if (M < 1 || M % B != 0) throw std::runtime_error(l2inf_bad_rows(M, B));
  if (M >= (1ll << 31)) throw std::runtime_error("the stacked l2,inf ball (l2inf_stacked): the operator needs fewer than 2^31 rows");
  return M / B;
}

// the scalar bound of a descriptor
inline void l2inf_check_c(double c) {
  if (!(c > 0)) throw std::runtime_error(L2INF_BAD_C);
}
// a host vector of bounds, `groups` entries; has_member(p): false for the groups whose entry is not looked at
template <typename T, typename F>
void l2inf_check_vector(const T* c, long long groups, F has_member) {
  for (long long p = 0; p < groups; ++p)
    if (!(c[p] >= T(0)) && has_member(p)) throw std::runtime_error(l2inf_bad_entry(p));
}

// ---- the rule of one group ----------------------------------------------------------------------------------------------------------------
// is the group scaled?  (false: it keeps its bits)
template <typename T>
__host__ __device__ inline bool l2inf_clipped(T g, T c) { return g > c; }
// f_p of a clipped group
template <typename T>
__host__ __device__ inline T l2inf_factor(T g, T c) { return c / g; }
template <typename T>
__host__ __device__ inline T l2inf_scaled(T v, T f) { return v * f; }
// the group of up to `n` members v[0 .. n - 1] (member[q] false: a row the block does not have), in place; returns g
template <typename T>
__host__ __device__ inline T l2inf_group(T* v, const bool* member, int n, T c) {
  double ss = 0.0;
  for (int q = 0; q < n; ++q) ss += l21_square<T>(v[q], member[q]);
  const T g = l21_norm_of<T>(ss);
  if (!l2inf_clipped<T>(g, c)) return g;
  const T f = l2inf_factor<T>(g, c);
  for (int q = 0; q < n; ++q)
    if (member[q]) v[q] = l2inf_scaled<T>(v[q], f);
  return g;
}
// what the observed norm of a projected group of m members may exceed c by, in units of u c, u = eps / 2 (derivation above)
template <typename T>
__host__ __device__ inline double l2inf_excess_units(long long m) {
  const double kg = sizeof(T) == 4 ? 1.0 + (double)m / 268435456.0 : 1.0 + 0.5 * (double)m;
  return 2.0 * kg + 2.0 + 0.01;
}

}  // namespace sipx
