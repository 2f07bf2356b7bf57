// Joint (vectorial) isotropic total variation: the l2,1 ball whose groups span the frames, on the range of the in-plane gradient
// TV_xy = vcat(D_y, D_x) of a 3-D grid, { v : sum_{(i,j)} g_ij <= tau } (ext_group.hip, BallProj).  The launch plan of the z-march
// and the rule of one pixel as __host__ __device__ functions (tests/l21_joint/rule_driver.cpp runs them on the CPU); the kernels in
// ext_group.hip call nothing else for the arithmetic.
//
// GROUPS.  l21.h with the two blocks dir = {1, 0} on an (n1, n2, n3) grid.  The group of PIXEL (i, j) holds, for every frame k, the D_y
// difference that starts at (i, j, k) if j < n2 - 1 and the D_x difference if i < n1 - 1 (l21_member): 0 to 2 n3 members, the last
// corner pixel has none.  There are L = n1 n2 groups; pixel p = i + n1 j of frame k is grid point p + k L.  Rows a block does not have
// are pads of the layout: they contribute nothing, are never written, and what they hold is never looked at.
//
// RULE.
//   ss_ij   = the float64 sum of l21_square over the members, frames ascending and within a frame D_y then D_x (l21_joint_add).  The
//             z range may be cut into chunks (l21_joint_plan): chunk c covers the frames [c zc, min((c + 1) zc, n3)), every chunk sum
//             starts from 0.0, the chunk sums are added in ascending c starting from 0.0 (l21_joint_total).  One chunk: the plain
//             serial sum.
//   g_ij    = (T) sqrt(ss_ij), rounded once (l21_norm_of)
//   theta   = the threshold of the l1 ball of radius tau on the L numbers g: the engine's own search (K<T>::proj_scalars_arr, PX_L1) with a
//             state of its own; Float64: re-evaluated on the search's active set in twice the working precision (l21.h)
//   the search's own decision ||g||_1 <= tau (ProjScalars::need == 0) leaves v unwritten: its bits stay, -0.0 included
//   otherwise every member of group (i, j), in every frame, is multiplied by l21_weight(g_ij, theta) in T
// PLAN.  A thread of the z-march owns the pixels of 16 bytes (or one pixel) and walks the frames of its chunk; L / VW threads alone
// underfill the device at frame sizes like 256 x 256, so the frames are cut into as many chunks as it takes to reach L21J_FILL_THREADS
// threads, none shorter than L21J_MIN_CHUNK frames.  The plan depends on (L, n3, bytes per entry) and on nothing else -- no device
// property, no launch geometry, not the path (16 bytes or one pixel) the launch takes -- so the bits of g do not either.
// No floating-point atomics, and no state but the warm start of the search: two calls give the same bits.
#pragma once
#include "l21.h"

// (the two constants of the plan; a variant library with others: tools/build_variant.sh, EXTRA='-DL21J_FILL_THREADS=...')
#ifndef L21J_FILL_THREADS
#define L21J_FILL_THREADS 131072
#endif
#ifndef L21J_MIN_CHUNK
#define L21J_MIN_CHUNK 8
#endif

namespace sipx {

struct L21JointPlan {
  int nchunk;                 // chunks of the z range; 1: k_l21j_norms writes g itself
  int zc;                     // frames per chunk (the last one may be shorter)
  __host__ __device__ int z0(int c) const { return c * zc; }
  __host__ __device__ int z1(int c, int n3) const { return (c + 1) * zc < n3 ? (c + 1) * zc : n3; }
};
__host__ __device__ inline L21JointPlan l21_joint_plan(long long L, long long n3, int elem_bytes) {
  long long threads = L * elem_bytes / 16;                    // of one chunk on the 16-byte path
  if (threads < 1) threads = 1;
  const long long want = ((long long)L21J_FILL_THREADS + threads - 1) / threads, most = n3 / (long long)L21J_MIN_CHUNK;
  long long nc = want < most ? want : most;
  if (nc < 1) nc = 1;
  L21JointPlan p;
  p.zc = (int)((n3 + nc - 1) / nc);
  if (p.zc < 1) p.zc = 1;
  p.nchunk = (int)((n3 + p.zc - 1) / p.zc);
  if (p.nchunk < 1) p.nchunk = 1;
  return p;
}

// the two members a frame adds to a pixel's sum of squares, in contract order
template <typename T>
__host__ __device__ inline void l21_joint_add(double& ss, T vy, T vx, bool my, bool mx) {
  ss += l21_square<T>(vy, my);
  ss += l21_square<T>(vx, mx);
}
// ss_ij from the chunk sums part[c L + p]
__host__ __device__ inline double l21_joint_total(const double* part, long long L, long long p, int nchunk) {
  double ss = 0.0;
  for (int c = 0; c < nchunk; ++c) ss += part[(long long)c * L + p];
  return ss;
}

// The whole rule serially: what the kernels compute.  vy, vx: the padded blocks of D_y and D_x (N = L n3 entries each), g: L entries.
template <typename T>
__host__ __device__ inline void l21_joint_norms_serial(const L21JointPlan& plan, long long n1, long long n2, long long n3, const T* vy,
                                                        const T* vx, T* g) {
  const long long L = n1 * n2;
  for (long long p = 0; p < L; ++p) {
    const bool my = l21_member((int)(p / n1), (int)n2), mx = l21_member((int)(p % n1), (int)n1);
    double ss = 0.0;
    for (int c = 0; c < plan.nchunk; ++c) {
      double sc = 0.0;
      for (long long k = plan.z0(c); k < plan.z1(c, (int)n3); ++k) l21_joint_add<T>(sc, vy[p + k * L], vx[p + k * L], my, mx);
      ss += sc;
    }
    g[p] = l21_norm_of<T>(ss);
  }
}
template <typename T>
__host__ __device__ inline void l21_joint_scale_serial(long long n1, long long n2, long long n3, T* vy, T* vx, const T* g, T theta) {
  const long long L = n1 * n2;
  for (long long p = 0; p < L; ++p) {
    const bool my = l21_member((int)(p / n1), (int)n2), mx = l21_member((int)(p % n1), (int)n1);
    const T f = l21_weight<T>(g[p], theta);
    for (long long k = 0; k < n3; ++k) {
      if (my) vy[p + k * L] = vy[p + k * L] * f;
      if (mx) vx[p + k * L] = vx[p + k * L] * f;
    }
  }
}

}  // namespace sipx
