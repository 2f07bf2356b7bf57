// The weighted l1 ball: { v : sum_i w_i |v_i| <= tau } on the rows of A x, one weight w_i >= 0 per row of the operator (identity, D_x, D_y,
// D_z, TV, TV_xy), in the reference's row order (ext_group.hip, L1WProj).  The set of iteratively reweighted l1, of anisotropic TV with a
// weight per direction, of masks (w_i = 0 leaves a row free).  The rule as __host__ __device__ functions (tests/l1_weighted/rule_driver.cpp
// runs them on the CPU); the kernels in ext_group.hip call nothing else for the arithmetic.  The reference package has no such projector.
//
// RULE.  With a_i = |v_i| the search is the rule of l21_weighted.h on the pairs (a, w): l21w_clean, L21WSums, l21w_add, l21w_active,
// l21w_theta_of, L21WState, l21w_start and l21w_step as they stand there.
//   asum    = sum_i (double)w_i (double)a_i (an L21Sum, the order of l21_weighted.h SUMS); (T)asum <= tau: v is not written at all,
//             its bits stay (-0.0 included)
//   otherwise theta_0 = (S_all - tau) / C_all, A_k = { i : (double)a_i > theta_k (double)w_i }, theta_{k+1} = max(theta_k, (S_k - tau) / C_k),
//             stop when the integer count repeats or is 0, theta = (T) max(theta_k, 0), rounded once
//   weight 0  an entry whose cleaned weight is 0 adds nothing to S or C whatever v_i holds: it is not multiplied by 0 (l1w_take).  Every row
//             a block of the operator does not have carries weight 0 in the padded layout, and kernels do not rely on what pads hold
//             (l21.h): a NaN or an infinity there does not reach the sums.  Such an entry is counted as l21w_search_serial counts it (in
//             the first pass, and later when a_i > 0), so that for finite v need, theta, asum AND the passes are those of
//             l21w_search_serial(|v|, w); the count of entries that never move only shifts the stop test by a constant.
//   apply   for w_i > 0, all in T:  p = theta w_i (rounded in T; -ffp-contract=off),  t = a_i - p,
//             y_i = t > 0 ? copysign(t, v_i) : copysign(0, v_i)            (an entry on the threshold is zeroed)
//           w_i == 0: y_i = v_i, not written (beside a weighted entry in one 16-byte store its own bits go back)
// No floating-point atomics, no state between calls: the feasibility estimate and the y update take the same path, two calls give the
// same bits.
#pragma once
#include <cmath>
#include <stdexcept>
#include <string>

#include "l21_weighted.h"

namespace sipx {

// ---- host: what sipx_add_set, sipx_set_data, sipx_project and sipx_l1_weighted_norm refuse (called from set_config.h and the engine) --------
constexpr const char* L1W_NO_MODE = "the weighted l1 ball (l1_weighted) applies to the whole array (matrix / tensor mode): per fiber or slice use "
                                    "(\"l1\", op, mode) with segment_norms=True, which takes one radius per segment";
constexpr const char* L1W_NO_TRANSFORM = "the weighted l1 ball (l1_weighted) takes no transform (DFT, DCT, wavelet): its weights are one per row of "
                                         "identity, D_x, D_y, D_z, TV or TV_xy -- behind a transform use the plain (\"l1\", transform)";
constexpr const char* L1W_NO_CUSTOM = "the weighted l1 ball (l1_weighted) takes no custom operator: its weights follow the rows of identity, D_x, "
                                      "D_y, D_z, TV or TV_xy -- scale the rows of the operator and use the plain (\"l1\", op)";
constexpr const char* L1W_NO_MINKOWSKI = "the weighted l1 ball (l1_weighted) takes no Minkowski component: use the plain (\"l1\", op) there";
constexpr const char* L1W_SHARDED = "the weighted l1 ball (l1_weighted) takes single-process contexts only, this one has a communicator, a slab "
                                    "decomposition or set ownership: use the plain (\"l1\", op), or a single process";
constexpr const char* L1W_NEEDS_WEIGHTS = "the weighted l1 ball (l1_weighted) needs its weights in lb, one per row of the operator: without "
                                          "weights the set is the plain (\"l1\", op)";
constexpr const char* L1W_NO_UB = "the weighted l1 ball (l1_weighted) takes weights in lb and no ub: the radius is pmax";
constexpr const char* L1W_SET_DATA_UB = "the weights of the weighted l1 ball are its lb; it has no ub (the radius is fixed at sipx_add_set)";

// the descriptor: lb = one weight per row or NULL (sipx_set_data brings them), never ub; `given`: the entries the descriptor says lb holds
inline void l1w_check_desc(bool has_ub, long long given, long long rows) {
  if (has_ub) throw std::runtime_error(L1W_NO_UB);
  if (given != rows)
    throw std::runtime_error("the weighted l1 ball (l1_weighted): " + std::to_string(given) + " weights given, " + std::to_string(rows) +
                             " are needed -- one per row of the operator, in the order of A x");
}
// every host path refuses a weight that is negative, NaN or infinite, naming the first offender (the rule of check_l21_weights)
template <typename T>
void check_l1w_weights(const T* w, long long n) {
  for (long long k = 0; k < n; ++k)
    if (!(w[k] >= T(0)) || !(w[k] < (T)INFINITY))
      throw std::runtime_error("the weighted l1 ball (l1_weighted): weight " + std::to_string(k) +
                               " is negative, NaN or infinite -- every weight must be finite and >= 0 (0 leaves its row free)");
}

// ---- the search: one entry (v, w) enters the sums of a pass (w: cleaned; FIRST: the pass over every entry, theta is not looked at) ----------
template <typename T, bool FIRST>
__host__ __device__ inline void l1w_take(L21WSums& a, T v, T w, double theta) {
  if (!(w > T(0))) {                 // nothing of v reaches S or C; counted as l21w_active(|v|, 0, theta) counts a finite entry
    if (FIRST || fabs(v) > T(0)) a.cnt += 1.0;
    return;
  }
  const T av = fabs(v);
  if (FIRST || l21w_active<T>(av, w, theta)) l21w_add<T>(a, av, w);
}
// ---- the apply: y of an entry whose cleaned weight is > 0 ----------------------------------------------------------------------------------
template <typename T>
__host__ __device__ inline T l1w_shrink(T v, T w, T theta) {
  const T p = theta * w;
  const T t = fabs(v) - p;
  return t > T(0) ? copysign(t, v) : copysign(T(0), v);
}

// The whole projection serially, one L21WSums per pass added in index order: what the kernels compute up to the order of their sums.
// Returns need (-1 when the bound of n + 1 passes of the host loop is exceeded, v is then not written); theta_T, asum, the passes come back.
template <typename T>
__host__ __device__ inline int l1w_project_serial(T* v, const T* w, long long n, T tau, T& theta_T, double& asum, int& passes) {
  L21WState st{};
  L21WSums all;
  for (long long i = 0; i < n; ++i) l1w_take<T, true>(all, v[i], l21w_clean<T>(w[i]), 0.0);
  l21w_start<T>(st, theta_T, all, tau);
  for (long long it = 0; !st.done; ++it) {
    if (it > n) { passes = st.passes; asum = st.asum; return -1; }
    L21WSums act;
    for (long long i = 0; i < n; ++i) l1w_take<T, false>(act, v[i], l21w_clean<T>(w[i]), st.theta);
    l21w_step<T>(st, theta_T, act, tau);
  }
  asum = st.asum;
  passes = st.passes;
  if (st.need)                       // (all weights 0: asum = 0 <= tau, need = 0)
    for (long long i = 0; i < n; ++i) {
      const T wi = l21w_clean<T>(w[i]);
      if (wi > T(0)) v[i] = l1w_shrink<T>(v[i], wi, theta_T);
    }
  return st.need;
}

}  // namespace sipx
