// Weighted isotropic total variation: the ball { v : sum_p w_p ||v_p||_2 <= tau } on the groups of l21.h (the N grid points of TV / TV_xy)
// or of l21_joint.h (the L = n1 n2 pixels across the frames), every group with a weight w_p >= 0 (ext_group.hip, BallProj's weighted
// route).  The rule as __host__ __device__ functions (tests/l21_weighted/rule_driver.cpp runs them on the CPU); the kernels in
// ext_group.hip call nothing else for the arithmetic.  The reference package has no such projector.
//
// RULE.
//   g_p     = exactly as in the unweighted sets (l21_group_norm; the z-march of l21_joint.h), n entries
//   w_p     = the weight as given when it is >= 0 and finite, 0 otherwise (l21w_clean: every host path refuses such a weight, one that
//             arrives from device memory cannot be checked and leaves its group unconstrained)
//   asum    = sum_p (double)w_p (double)g_p in the fixed order of SUMS below; (T)asum <= tau: v is not written at all, its bits stay
//   otherwise theta is the fixed point of the weighted Michelot iteration,
//             theta_0     = (S_all - tau) / C_all,  S = sum w g and C = sum w^2 over all groups
//             A_k         = { p : g_p > theta_k w_p }, compared in float64 as written: (double)g_p > theta_k * (double)w_p
//             theta_{k+1} = max(theta_k, (S_k - tau) / C_k) over A_k; an empty A_k keeps theta_k
//             stop        when the integer count |A_k| repeats (|A_{-1}| = n) or is 0
//             theta       = (T) max(theta_k, 0), rounded once
//             (the reference's `rho + 1 < lv` cap of the l1 search is not carried over: on a grid the last corner has g = 0)
//   apply   v_q[p] <- v_q[p] * f_p,  t = g_p - theta * w_p (the product rounded in T); t = t > 0 ? t : 0; f_p = g_p > 0 ? t / g_p : 0,
//             all in T (l21w_factor).  g_p == theta w_p zeroes the group; w_p == 0 gives f_p = 1 exactly and the group is not stored.
// SUMS.  Both precisions carry S and C as unevaluated sums of two doubles (L21Sum of l21.h: every addition's rounding error kept).
// T = float: the products w g and w w are exact in float64.  T = double: the product's own rounding error, fma(w, g, -p), is kept in
// the low word -- every pass, not only the last, evaluates (S - tau) / C in twice the working precision (l21w_theta_of).  Order: a
// thread adds its entries in ascending index, the threads of a workgroup are merged by l21w_tree (the halving order of l21_tree_merge),
// the workgroups by the same tree in the finish kernel.  The bits depend on the launch geometry, which depends on (n, T, the 16-byte
// path) alone.  The count is an integer held in a double (n < 2^31).
// No floating-point atomics, no state between calls: the feasibility estimate and the y update take the same path, two calls give
// the same bits.
#pragma once
#include <stdexcept>
#include <string>

#include "l21.h"

namespace sipx {

// ---- host: what sipx_add_set, sipx_set_data and sipx_l21_weighted_norm refuse (called from set_config.h and the engine) ----------------------
// every host path refuses a weight that is negative, NaN or infinite, naming the set and the first offender
template <typename T>
void check_l21_weights(const T* w, long long n, const char* set) {
  for (long long k = 0; k < n; ++k)
    if (!(w[k] >= T(0)) || !(w[k] < (T)INFINITY))
      throw std::runtime_error(std::string("the weighted l2,1 ball (") + set + "): weight " + std::to_string(k) +
                               " is negative, NaN or infinite -- every weight must be finite and >= 0 (0 leaves its group unconstrained)");
}
// the descriptor of a whole-array l2,1 set: lb = one weight per group or NULL, never ub; `given`: the entries the descriptor says lb holds
inline void l21w_check_desc(const char* set, bool has_lb, bool has_ub, long long given, long long groups, bool joint) {
  if (has_ub)
    throw std::runtime_error(std::string("the l2,1 ball (") + set + ") on the whole array takes weights in lb and no ub: the radius is pmax");
  if (has_lb && given != groups)
    throw std::runtime_error(std::string("the weighted l2,1 ball (") + set + "): " + std::to_string(given) + " weights given, " +
                             std::to_string(groups) + " are needed -- one per " + (joint ? "pixel (n1 n2)" : "grid point"));
}
inline void l21w_refuse_frames() {
  throw std::runtime_error("the l2,1 ball per frame takes no weights (lb): use the whole-array set on TV_xy or the joint set, "
                           "which take one weight per group");
}

// the weight the rule uses: a weight that is not >= 0 and finite counts as 0
template <typename T>
__host__ __device__ inline T l21w_clean(T w) {
  return (w > T(0) && w < (T)INFINITY) ? w : T(0);
}

// the sums of one pass: S = sum w g, C = sum w^2, cnt = |A|
struct L21WSums {
  L21Sum S{0.0, 0.0}, C{0.0, 0.0};
  double cnt = 0.0;
};
// x * y into acc with the product's rounding error kept (T = float: the product is exact and the fma is not needed)
template <typename T>
__host__ __device__ inline void l21w_add_product(L21Sum& acc, double x, double y) {
  const double p = x * y;
  l21_sum_add(acc, p);
  if (sizeof(T) == 8) acc.lo += fma(x, y, -p);
}
// one group enters the sums of a pass (w: cleaned)
template <typename T>
__host__ __device__ inline void l21w_add(L21WSums& a, T g, T w) {
  l21w_add_product<T>(a.S, (double)w, (double)g);
  l21w_add_product<T>(a.C, (double)w, (double)w);
  a.cnt += 1.0;
}
__host__ __device__ inline void l21w_merge(L21WSums& a, const L21WSums& o) {
  l21_sum_merge(a.S, o.S);
  l21_sum_merge(a.C, o.C);
  a.cnt += o.cnt;
}
// is group (g, w) in the active set of theta?  (w: cleaned)
template <typename T>
__host__ __device__ inline bool l21w_active(T g, T w, double theta) {
  return (double)g > theta * (double)w;
}
// (S - tau) / C with S and C in twice the working precision: the quotient of the leading words corrected once by the remainder
__host__ __device__ inline double l21w_theta_of(const L21Sum& S, const L21Sum& C, double tau) {
  double d, e;
  l21_two_sum(S.hi, -tau, d, e);
  const double nlo = e + S.lo;
  const double q = (d + nlo) / C.hi;
  const double r = (fma(-q, C.hi, d) + nlo) - q * C.lo;
  return q + r / C.hi;
}

// The state of the iteration: on the device one of these per projector call (k_l21w_finish alone writes it).
struct L21WState {
  double theta;        // theta_k
  double asum;         // S_all of the first pass, as a float64
  double prev;         // |A_{k-1}|
  int done;            // 1: theta_T / need hold
  int need;            // 0: inside the ball, v is not written
  int passes;          // evaluations of (S, C) so far, the first included
  int pad;
};
// the first pass (every group): asum, the decision, theta_0
template <typename T>
__host__ __device__ inline void l21w_start(L21WState& st, T& theta_T, const L21WSums& all, T tau) {
  st.asum = all.S.hi + all.S.lo;
  st.prev = all.cnt;
  st.passes = 1;
  st.theta = 0.0;
  theta_T = T(0);
  if ((T)st.asum <= tau) { st.need = 0; st.done = 1; return; }
  st.need = 1;
  st.done = 0;
  st.theta = l21w_theta_of(all.S, all.C, (double)tau);
}
// a pass over A_k
template <typename T>
__host__ __device__ inline void l21w_step(L21WState& st, T& theta_T, const L21WSums& act, T tau) {
  st.passes += 1;
  if (act.cnt > 0.0) {
    const double th = l21w_theta_of(act.S, act.C, (double)tau);
    st.theta = th > st.theta ? th : st.theta;
  }
  if (!(act.cnt > 0.0) || act.cnt == st.prev) {
    st.done = 1;
    theta_T = (T)(st.theta > 0.0 ? st.theta : 0.0);
  }
  st.prev = act.cnt;
}
// f_p: the factor every member of the group is multiplied by (w: cleaned)
template <typename T>
__host__ __device__ inline T l21w_factor(T g, T w, T theta) {
  T t = g - theta * w;
  t = t > T(0) ? t : T(0);
  return g > T(0) ? t / g : T(0);
}

// The whole search serially, one L21WSums per pass added in index order: what the kernels compute up to the order of their sums.
// Returns need (-1 when the bound of n + 1 passes of the host loop is exceeded); theta_T, asum and the passes come back.
template <typename T>
__host__ __device__ inline int l21w_search_serial(const T* g, const T* w, long long n, T tau, T& theta_T, double& asum, int& passes) {
  L21WState st{};
  L21WSums all;
  for (long long p = 0; p < n; ++p) l21w_add<T>(all, g[p], l21w_clean<T>(w[p]));
  l21w_start<T>(st, theta_T, all, tau);
  for (long long it = 0; !st.done; ++it) {
    if (it > n) { passes = st.passes; asum = st.asum; return -1; }
    L21WSums act;
    for (long long p = 0; p < n; ++p) {
      const T wp = l21w_clean<T>(w[p]);
      if (l21w_active<T>(g[p], wp, st.theta)) l21w_add<T>(act, g[p], wp);
    }
    l21w_step<T>(st, theta_T, act, tau);
  }
  asum = st.asum;
  passes = st.passes;
  return st.need;
}

#if defined(__HIPCC__)
// The fixed tree of a pass' sums across the NT threads of a workgroup, in the halving order of l21_tree_merge: thread t merges its
// sums with those of thread t + w for w = NT / 2 .. 1.  `red`: 5 * NT doubles of LDS.  The total comes back in thread 0 alone.
template <int NT>
__device__ __forceinline__ void l21w_tree(L21WSums& a, double* red) {
  double *r0 = red, *r1 = red + NT, *r2 = red + 2 * NT, *r3 = red + 3 * NT, *r4 = red + 4 * NT;
  const int t = threadIdx.x;
  r0[t] = a.S.hi; r1[t] = a.S.lo; r2[t] = a.C.hi; r3[t] = a.C.lo; r4[t] = a.cnt;
  __syncthreads();
  for (int w = NT / 2; w > 0; w >>= 1) {
    if (t < w) {
      L21WSums x, y;
      x.S = L21Sum{r0[t], r1[t]}; x.C = L21Sum{r2[t], r3[t]}; x.cnt = r4[t];
      y.S = L21Sum{r0[t + w], r1[t + w]}; y.C = L21Sum{r2[t + w], r3[t + w]}; y.cnt = r4[t + w];
      l21w_merge(x, y);
      r0[t] = x.S.hi; r1[t] = x.S.lo; r2[t] = x.C.hi; r3[t] = x.C.lo; r4[t] = x.cnt;
    }
    __syncthreads();
  }
  if (t == 0) { a.S = L21Sum{r0[0], r1[0]}; a.C = L21Sum{r2[0], r3[0]}; a.cnt = r4[0]; }
  __syncthreads();
}
#endif

}  // namespace sipx
