// Isotropic total variation: the l2,1 ball { v : sum_p ||v_p||_2 <= tau } on the range of the TV operator (ext_group.hip,
// BallProj).  The rule of one group as __host__ __device__ functions (tests/l21/rule_driver.cpp runs them on the CPU); the
// kernels in ext_group.hip call nothing else for the arithmetic.
//
// GROUPS.  The TV operator lays its nblk = 2 (2-D) or 3 (3-D) difference blocks side by side as full padded grids with block
// stride N = prod(n): block q holds the forward differences along direction dir[q].  The group of grid point p is the set of
// differences that START at p, { v[q * N + p] : q < nblk and p has a successor along dir[q] } -- 0 to ndim members; the last
// corner of the grid has none.  A row a block does not have (p on the far face along dir[q]) is a pad of the layout: it
// contributes nothing to the norm, is never written, and what it holds is never looked at (l21_member).
//
// RULE.
//   g_p     = (T) sqrt( sum_q (double)v_q[p]^2 ), the float64 sum of squares taken in block order q = 0, 1, 2 and rounded once to T
//             (seg_norm.h's l2 convention)
//   theta   = the threshold of the l1 ball of radius tau on the array g (N entries): the engine's own search (K<T>::proj_scalars_arr,
//             PX_L1), exact in float64 and rounded once to T
//   the search's own decision ||g||_1 <= tau (ProjScalars::need == 0) leaves v unwritten: its bits stay, -0.0 included
//   otherwise v_q[p] <- v_q[p] * f_p,  t = g_p - theta; t = t > 0 ? t : 0; f_p = g_p > 0 ? t / g_p : 0, all in T
//             (ext_transform.hip, k_csoft: the groups (re, im) of the l1 ball behind the DFT)
// THRESHOLD IN FLOAT64.  The search evaluates theta = (S - tau) / C, S and C the sum and count of the g_p above theta, in float64.
// For T = float that is exact to far below half an ulp of T.  For T = double it is a float64 sum: off by a few ulp of S / C, which
// for a group barely above a small theta is many ulp of g_p - theta.  The Float64 projector therefore takes the search's active set
// { g_p > theta_search } and evaluates (S - tau) / C once more with S as an unevaluated sum of two doubles (every addition's rounding
// error kept, fixed order: l21_sum_add / l21_sum_merge / l21_theta_refined below); that theta is applied.  The active set of the
// search is the set of the exact fixed point unless a g_p lies within the search's error of theta, and such a group changes
// (S - tau) / C by less than that error over C.  The search's state is not touched.  When no g_p or every g_p is above
// theta_search (the reference's `rho + 1 < lv` cap; impossible on a grid, whose last corner has g = 0) theta_search is applied.
// Float64 inputs whose squares leave the float64 range (|v| above about 1e154, or squares that underflow) are outside the
// contract: the sum of squares is taken as it is, without rescaling.
// No floating-point atomics, and no state but the warm start of the search: two calls give the same bits.
#pragma once
#include <cmath>

#include <hip/hip_runtime.h>

namespace sipx {

// does point p have a member in the block along a direction of extent nd, where its coordinate is cd?
__host__ __device__ inline bool l21_member(int cd, int nd) { return cd < nd - 1; }

// one term of the sum of squares; a row the block does not have contributes exactly nothing, whatever it holds
template <typename T>
__host__ __device__ inline double l21_square(T v, bool member) {
  return member ? (double)v * (double)v : 0.0;
}
// g_p of a group from its float64 sum of squares (added in block order)
template <typename T>
__host__ __device__ inline T l21_norm_of(double sumsq) {
  return (T)sqrt(sumsq);
}
// g_p of up to three members
template <typename T>
__host__ __device__ inline T l21_group_norm(const T* v, const bool* member, int nblk) {
  double ss = 0.0;
  for (int q = 0; q < nblk; ++q) ss += l21_square<T>(v[q], member[q]);
  return l21_norm_of<T>(ss);
}
// f_p: the factor every member of the group is multiplied by
template <typename T>
__host__ __device__ inline T l21_weight(T g, T theta) {
  T t = g - theta;
  t = t > T(0) ? t : T(0);
  return g > T(0) ? t / g : T(0);
}

// ---- Float64: (S - tau) / C with S in twice the working precision ---------------------------------------------------------------------
// hi + lo is the sum so far: hi the float64 sum, lo the rounding errors of its additions (Knuth's two-sum; needs -ffp-contract=off
// and no value-changing optimisation, as all of csrc/ is built)
struct L21Sum {
  double hi, lo;
};
__host__ __device__ inline void l21_two_sum(double a, double b, double& s, double& e) {
  s = a + b;
  const double bb = s - a;
  e = (a - (s - bb)) + (b - bb);
}
__host__ __device__ inline void l21_sum_add(L21Sum& acc, double x) {
  double s, e;
  l21_two_sum(acc.hi, x, s, e);
  acc.hi = s;
  acc.lo += e;
}
__host__ __device__ inline void l21_sum_merge(L21Sum& acc, const L21Sum& o) {
  double s, e;
  l21_two_sum(acc.hi, o.hi, s, e);
  acc.hi = s;
  acc.lo += e + o.lo;
}
// theta of the active set (sum S, count C of N entries) for radius tau; theta_search where the set is empty or everything
__host__ __device__ inline double l21_theta_refined(const L21Sum& S, double C, double tau, double N, double theta_search) {
  if (!(C > 0.0) || !(C < N)) return theta_search;
  double d, e;
  l21_two_sum(S.hi, -tau, d, e);
  const double th = (d + (e + S.lo)) / C;
  return th > 0.0 ? th : 0.0;
}

#if defined(__HIPCC__)
// The fixed tree of the sums in twice the working precision, across the NT threads of a workgroup: the four-wave layout of segn_sum2
// does not apply to a pair that is merged, not added, so the pairs are merged in halves -- thread t merges (sh[t], sl[t]) with
// (sh[t + w], sl[t + w]) for w = NT / 2 .. 1, the counts are added alongside.  `red`: 3 * NT doubles of LDS.  Returned to every thread.
// Every Float64 threshold (k_l21_theta_part, k_l21_theta_final, k_l21_frames) goes through this one order.
template <int NT>
__device__ __forceinline__ void l21_tree_merge(L21Sum& a, double& c, double* red) {
  double *sh = red, *sl = red + NT, *sc = red + 2 * NT;
  sh[threadIdx.x] = a.hi; sl[threadIdx.x] = a.lo; sc[threadIdx.x] = c;
  __syncthreads();
  for (int w = NT / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      L21Sum x{sh[threadIdx.x], sl[threadIdx.x]};
      l21_sum_merge(x, L21Sum{sh[threadIdx.x + w], sl[threadIdx.x + w]});
      sh[threadIdx.x] = x.hi; sl[threadIdx.x] = x.lo; sc[threadIdx.x] += sc[threadIdx.x + w];
    }
    __syncthreads();
  }
  a.hi = sh[0]; a.lo = sl[0]; c = sc[0];
  __syncthreads();
}
#endif

}  // namespace sipx
