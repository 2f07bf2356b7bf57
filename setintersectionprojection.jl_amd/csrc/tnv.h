// Total nuclear variation: the nuclear-norm ball on the frame Jacobians of the in-plane gradient TV_xy = vcat(D_y, D_x) of a 3-D grid,
//     { v = TV_xy x : sum over pixels p of ||J_p||_* <= tau },   J_p = the 2 x n3 matrix whose column k is (D_y x, D_x x) at pixel p in frame k
// (ext_group.hip, TnvProj).  The Schatten-1 member of the family whose Frobenius member is l21_joint.h: the frames share not only where
// their edges are but the direction of their gradients.  The rule of one pixel as __host__ __device__ functions
// (tests/tnv/rule_driver.cpp runs them on the CPU); the kernels in ext_group.hip call nothing else for the arithmetic.  The reference
// package has no such projector.
//
// GROUPS.  Those of l21_joint.h: pixel (i, j) has a D_y member in every frame if j < n2 - 1 and a D_x member in every frame if
// i < n1 - 1 (l21_member); L = n1 n2 pixels, pixel p = i + n1 j of frame k is grid point p + k L.  A block a pixel does not have is a
// row of zeros of J_p: its pad entries are never used for arithmetic (tnv_gram_add, tnv_apply_pair replace them by 0) and never written.
//
// RULE, per pixel p.
//   Gram     G_p = J_p J_p' = [[a, c], [c, b]], a = sum_k vy^2, b = sum_k vx^2, c = sum_k vy vx.  Frames ascend; the z range is cut into
//            the chunks of l21_joint_plan(L, n3, sizeof(T)), every chunk sum starts from zero, the chunk sums are added in ascending
//            order starting from zero (tnv_gram_add, tnv_gram_merge): the order rule of l21_joint.h for three sums.
//            T = float: plain float64 sums, the products are exact.  T = double: every sum is an unevaluated pair of doubles (L21Sum) whose
//            low word keeps the rounding error of every addition and, by fma, of every product (l21w_add_product<double>).
//   Decomp.  d = (a - b) / 2, r = hypot(d, c), lambda1 = (a + b) / 2 + r, lambda2 = max(a b - c^2, 0) / lambda1 -- never (a + b) / 2 - r,
//            which cancels.  T = double: a b - c^2 and the quotient are evaluated in twice the working precision from the hi / lo words
//            (tnv_lambda2_wide): in plain float64 the cancellation in a b - c^2 costs sigma2 half its digits on a pixel that is nearly
//            rank 1.  sigma1 = (T) sqrt(lambda1), sigma2 = (T) sqrt(lambda2), each rounded once.  The left singular vector is
//            u1 = (cs, sn), normalised from (d + r, c) if d >= 0, else from (c, r - d); hypot(d, c) == 0 gives u1 = (1, 0).  (cs, sn) are
//            kept in T.  A pixel with no members, or all zeros, gives sigma = 0.
//   Thresh.  theta = the threshold of the l1 ball of radius tau on the 2 L numbers s = [sigma1 of all pixels; sigma2 of all pixels]: the
//            engine's own search (K<T>::proj_scalars_arr, PX_L1) with a state of its own; Float64: re-evaluated on the search's active
//            set in twice the working precision (l21.h).  The search's own decision ||s||_1 <= tau (ProjScalars::need == 0) leaves v
//            unwritten: its bits stay, -0.0 included.
//   Scaling  f_i = l21_weight(sigma_i, theta) in T, M_p = f2 I + (f1 - f2) u1 u1' in float64 (tnv_matrix); every frame's (vy, vx) at p
//            becomes M_p (vy, vx), the two products and their sum in float64, rounded once to T (tnv_apply_pair).  Only existing members
//            are written.
// PLAN.  l21_joint_plan: it depends on (L, n3, bytes per entry) alone, so the bits of s do not depend on the launch either.
// No floating-point atomics, and no state but the warm start of the search: two calls give the same bits.
#pragma once
#include "l21_joint.h"
#include "l21_weighted.h"

namespace sipx {

// the three sums of one pixel (one chunk, or all of them); T = float uses the hi words alone
struct TnvGram {
  L21Sum a, b, c;
};
// doubles a chunk leaves per pixel: part[(chunk * tnv_words + word) * L + pixel]
template <typename T>
constexpr int tnv_words() { return sizeof(T) == 8 ? 6 : 3; }

// what one frame adds to a pixel's sums
template <typename T>
__host__ __device__ inline void tnv_gram_add(TnvGram& g, T vy, T vx, bool my, bool mx) {
  const double y = my ? (double)vy : 0.0, x = mx ? (double)vx : 0.0;
  if (sizeof(T) == 8) {
    l21w_add_product<T>(g.a, y, y);
    l21w_add_product<T>(g.b, x, x);
    l21w_add_product<T>(g.c, y, x);
  } else {
    g.a.hi += y * y;
    g.b.hi += x * x;
    g.c.hi += y * x;
  }
}
// a chunk's sums enter the total
template <typename T>
__host__ __device__ inline void tnv_gram_merge(TnvGram& g, const TnvGram& o) {
  if (sizeof(T) == 8) {
    l21_sum_merge(g.a, o.a);
    l21_sum_merge(g.b, o.b);
    l21_sum_merge(g.c, o.c);
  } else {
    g.a.hi += o.a.hi;
    g.b.hi += o.b.hi;
    g.c.hi += o.c.hi;
  }
}
template <typename T>
__host__ __device__ inline void tnv_gram_store(const TnvGram& g, double* part, long long L, long long p, int c) {
  double* const o = part + (long long)c * tnv_words<T>() * L + p;
  if (sizeof(T) == 8) {
    o[0] = g.a.hi; o[L] = g.a.lo; o[2 * L] = g.b.hi; o[3 * L] = g.b.lo; o[4 * L] = g.c.hi; o[5 * L] = g.c.lo;
  } else {
    o[0] = g.a.hi; o[L] = g.b.hi; o[2 * L] = g.c.hi;
  }
}
// the sums of pixel p from the chunk sums, ascending c from zero
template <typename T>
__host__ __device__ inline TnvGram tnv_gram_total(const double* part, long long L, long long p, int nchunk) {
  TnvGram g{};
  for (int c = 0; c < nchunk; ++c) {
    const double* const o = part + (long long)c * tnv_words<T>() * L + p;
    TnvGram x{};
    if (sizeof(T) == 8) {
      x.a = L21Sum{o[0], o[L]}; x.b = L21Sum{o[2 * L], o[3 * L]}; x.c = L21Sum{o[4 * L], o[5 * L]};
    } else {
      x.a.hi = o[0]; x.b.hi = o[L]; x.c.hi = o[2 * L];
    }
    tnv_gram_merge<T>(g, x);
  }
  return g;
}

// max(a b - c^2, 0) / lambda1 from the hi / lo words of the sums, in twice the working precision: the products with their fma errors
// and the cross terms of the low words, their difference as a pair, the quotient corrected once by its remainder
__host__ __device__ inline double tnv_lambda2_wide(const TnvGram& g, double lambda1) {
  double ah, al, bh, bl, ch, cl;
  l21_two_sum(g.a.hi, g.a.lo, ah, al);
  l21_two_sum(g.b.hi, g.b.lo, bh, bl);
  l21_two_sum(g.c.hi, g.c.lo, ch, cl);
  const double p = ah * bh, pe = fma(ah, bh, -p) + (ah * bl + al * bh);
  const double q = ch * ch, qe = fma(ch, ch, -q) + 2.0 * (ch * cl);
  double s, se, dh, dl;
  l21_two_sum(p, -q, s, se);
  l21_two_sum(s, se + (pe - qe), dh, dl);
  if (!(dh > 0.0)) return 0.0;
  const double q1 = dh / lambda1;
  return q1 + (fma(-q1, lambda1, dh) + dl) / lambda1;
}

// what a pixel's sums decompose to: the two singular values and the left singular vector of the larger
template <typename T>
struct TnvPixel {
  T s1, s2, cs, sn;
};
template <typename T>
__host__ __device__ inline TnvPixel<T> tnv_decompose(const TnvGram& g) {
  const double a = sizeof(T) == 8 ? g.a.hi + g.a.lo : g.a.hi, b = sizeof(T) == 8 ? g.b.hi + g.b.lo : g.b.hi,
               c = sizeof(T) == 8 ? g.c.hi + g.c.lo : g.c.hi;
  const double d = 0.5 * (a - b), r = hypot(d, c), lambda1 = 0.5 * (a + b) + r;
  double lambda2 = 0.0;
  if (lambda1 > 0.0) {
    if (sizeof(T) == 8) {
      lambda2 = tnv_lambda2_wide(g, lambda1);
    } else {
      const double det = a * b - c * c;
      lambda2 = (det > 0.0 ? det : 0.0) / lambda1;
    }
  }
  TnvPixel<T> o;
  o.s1 = (T)sqrt(lambda1);
  o.s2 = (T)sqrt(lambda2);
  const double x = d >= 0.0 ? d + r : c, y = d >= 0.0 ? c : r - d, nn = hypot(x, y);
  o.cs = nn > 0.0 ? (T)(x / nn) : T(1);
  o.sn = nn > 0.0 ? (T)(y / nn) : T(0);
  return o;
}

// M_p = f2 I + (f1 - f2) u1 u1' = [[m00, m01], [m01, m11]]
template <typename T>
__host__ __device__ inline void tnv_matrix(T s1, T s2, T cs, T sn, T theta, double& m00, double& m01, double& m11) {
  const double f1 = (double)l21_weight<T>(s1, theta), f2 = (double)l21_weight<T>(s2, theta), df = f1 - f2;
  const double c = (double)cs, s = (double)sn;
  m00 = f2 + df * c * c;
  m01 = df * c * s;
  m11 = f2 + df * s * s;
}
// (oy, ox) = M_p (vy, vx); a member the pixel does not have enters as 0 and its output is not to be stored
template <typename T>
__host__ __device__ inline void tnv_apply_pair(double m00, double m01, double m11, T vy, T vx, bool my, bool mx, T& oy, T& ox) {
  const double y = my ? (double)vy : 0.0, x = mx ? (double)vx : 0.0;
  oy = (T)(m00 * y + m01 * x);
  ox = (T)(m01 * y + m11 * x);
}

// The whole rule serially: what the kernels compute.  vy, vx: the padded blocks of D_y and D_x (N = L n3 entries each); s: 2 L entries
// [sigma1; sigma2], rot: 2 L entries [cs; sn].
template <typename T>
__host__ __device__ inline void tnv_decompose_serial(const L21JointPlan& plan, long long n1, long long n2, long long n3, const T* vy,
                                                      const T* vx, T* s, T* rot) {
  const long long L = n1 * n2;
  for (long long p = 0; p < L; ++p) {
    const bool my = l21_member((int)(p / n1), (int)n2), mx = l21_member((int)(p % n1), (int)n1);
    TnvGram g{};
    for (int c = 0; c < plan.nchunk; ++c) {
      TnvGram gc{};
      for (long long k = plan.z0(c); k < plan.z1(c, (int)n3); ++k) tnv_gram_add<T>(gc, vy[p + k * L], vx[p + k * L], my, mx);
      tnv_gram_merge<T>(g, gc);
    }
    const TnvPixel<T> o = tnv_decompose<T>(g);
    s[p] = o.s1; s[L + p] = o.s2; rot[p] = o.cs; rot[L + p] = o.sn;
  }
}
template <typename T>
__host__ __device__ inline void tnv_apply_serial(long long n1, long long n2, long long n3, T* vy, T* vx, const T* s, const T* rot, T theta) {
  const long long L = n1 * n2;
  for (long long p = 0; p < L; ++p) {
    const bool my = l21_member((int)(p / n1), (int)n2), mx = l21_member((int)(p % n1), (int)n1);
    double m00, m01, m11;
    tnv_matrix<T>(s[p], s[L + p], rot[p], rot[L + p], theta, m00, m01, m11);
    for (long long k = 0; k < n3; ++k) {
      T oy, ox;
      tnv_apply_pair<T>(m00, m01, m11, vy[p + k * L], vx[p + k * L], my, mx, oy, ox);
      if (my) vy[p + k * L] = oy;
      if (mx) vx[p + k * L] = ox;
    }
  }
}

}  // namespace sipx
