// Per-frame isotropic total variation: the l2,1 ball of every z-slice on the range of the in-plane gradient TV_xy = vcat(D_y, D_x)
// of a 3-D grid, { v : sum_{p in frame k} ||v_p||_2 <= tau_k for every k } (ext_group.hip, FrameProj).  The plan of the threshold
// launch and the rule of one frame as __host__ __device__ functions (tests/l21_frames/rule_driver.cpp runs them on the CPU).
//
// GROUPS.  l21.h with the two blocks dir = {1, 0} on an (n1, n2, n3) grid: the group of point p = (i, j, k) holds the D_y difference
// that starts at p (j < n2 - 1) and the D_x difference (i < n1 - 1); the last corner of every frame has none.  Frame k is the L = n1 n2
// points (., ., k); no group reaches into another frame.
//
// RULE.
//   g_p      = l21_group_norm (l21.h): the float64 sum of squares in block order, rounded once to T
//   asum_k   = the float64 sum of the frame's g in the kernel's fixed order (seg_norm.h REDUCTIONS)
//   (T)asum_k <= tau_k: the frame is not written at all, its bits stay, -0.0 included (l21_seg_decide == 0)
//   otherwise Michelot's iteration of seg_norm.h on the L values g_p (l1_seg_start / l1_seg_step / l1_seg_finish), theta_k rounded
//   once to T, and every member of every group of the frame is multiplied by l21_weight(g_p, theta_k) in T
// THRESHOLD IN FLOAT64 (l21.h).  T = double: the last evaluation of (S - tau_k) / C over the converged active set { g_p > theta_k }
// carries S in twice the working precision (L21Sum, l21_sum_add / l21_sum_merge in the kernel's fixed order, l21_theta_refined);
// when that set is empty or the whole frame (the reference's `rho + 1 < lv` cap) the iteration's theta_k stays.
// RADII (seg_norm.h).  One scalar for every frame, or tau[k].  A radius that is not > 0 can only arrive from device memory (every
// host path refuses it): a frame that is not all zero is set to zero (l21_seg_decide == 3).
// No floating-point atomics, no state between calls: the y update and the feasibility estimate take the same path, two calls give
// the same bits.
#pragma once
#include "l21.h"
#include "seg_norm.h"

namespace sipx {

// Launch plan of the threshold kernel: one workgroup per frame, grid-stride over the frames; the frame's L group norms stay in LDS
// when they fit seg_norm.h's budget, otherwise every pass re-reads them from global memory.
struct L21SegPlan {
  int lds;                    // 1: the frame's g stay in LDS
  unsigned grid;
  unsigned lds_bytes;         // dynamic LDS of the launch
  __host__ __device__ int path() const { return lds ? 0 : 1; }      // 0 frame/LDS, 1 frame/streaming
};
__host__ __device__ inline L21SegPlan l21_seg_plan(long long L, long long nframes, int elem_bytes) {
  L21SegPlan p{};
  p.lds = L * elem_bytes <= (long long)SEGN_LDS_BYTES ? 1 : 0;
  p.lds_bytes = p.lds ? (unsigned)(L * elem_bytes) : 0u;
  p.grid = (unsigned)(nframes < SEGN_MAX_GRID ? (nframes < 1 ? 1 : nframes) : SEGN_MAX_GRID);
  return p;
}

// what happens to a frame: 0 not written, 1 scaled by the weights of its theta, 3 set to zero (a device radius that is not > 0)
template <typename T>
__host__ __device__ inline int l21_seg_decide(double asum, T tau, bool vec) {
  const bool ball = !vec || tau > T(0);
  if (!ball) return asum > 0 ? 3 : 0;
  return (T)asum <= tau ? 0 : 1;
}

// theta_k of a frame outside its ball from the end of Michelot's iteration; T = double: S, C are the sum (twice the working precision)
// and the count of the g_p above the iteration's theta (l21_seg_theta_search), T = float: not looked at
template <typename T>
__host__ __device__ inline T l21_seg_theta_search(const L1SegState& st, double asum, double gmin, T tau, long long L) {
  return (T)l1_seg_finish(st, asum, gmin, (double)tau, L);
}
__host__ __device__ inline double l21_seg_theta_final(double theta_search, const L21Sum& S, double C, double tau, long long L) {
  return l21_theta_refined(S, C, tau, (double)L, theta_search);
}

// One frame, serially in index order: what the kernel computes up to the order of its sums.  Returns l21_seg_decide; theta and the
// number of Michelot passes (evaluations of S, C) come back for a frame that is scaled.
template <typename T>
__host__ __device__ inline int l21_seg_frame(const T* g, long long L, T tau, bool vec, T& asum_T, T& theta, int& passes) {
  double asum = 0, gmin = (double)INFINITY;
  for (long long t = 0; t < L; ++t) {
    const double a = (double)g[t];
    asum += a;
    gmin = a < gmin ? a : gmin;
  }
  asum_T = (T)asum;
  theta = T(0);
  passes = 0;
  const int act = l21_seg_decide<T>(asum, tau, vec);
  if (act != 1) return act;
  L1SegState st = l1_seg_start(asum, (double)tau, L);
  for (long long it = 0; it <= L + 1 && !st.done; ++it) {
    double S = 0, C = 0;
    for (long long t = 0; t < L; ++t) {
      const double a = (double)g[t];
      if (a > st.theta) { S += a; C += 1.0; }
    }
    l1_seg_step(st, S, C, (double)tau);
    ++passes;
  }
  theta = l21_seg_theta_search<T>(st, asum, gmin, tau, L);
  if (sizeof(T) == 8) {
    L21Sum S{0.0, 0.0};
    double C = 0;
    for (long long t = 0; t < L; ++t) {
      const double a = (double)g[t];
      if (a > (double)theta) { l21_sum_add(S, a); C += 1.0; }
    }
    theta = (T)l21_seg_theta_final((double)theta, S, C, (double)tau, L);
  }
  return act;
}

#if defined(__HIPCC__)
// f(t, src[t]) for the thread's entries t = tid, tid + BLOCK, ... in that order, L21_SEG_LOADS loads issued before the first is used:
// one workgroup streams a whole frame, and with one load in flight per lane a pass is a chain of L / BLOCK exposed memory latencies
// (the weak case of k_seg_norm).  The order of the visits, hence every sum, is that of the plain loop.
constexpr int L21_SEG_LOADS = 8;
template <typename T, typename F>
__device__ __forceinline__ void l21_seg_each(const T* __restrict__ src, unsigned L, F&& f) {
  unsigned t = threadIdx.x;
  for (; t + (L21_SEG_LOADS - 1) * BLOCK < L; t += L21_SEG_LOADS * BLOCK) {
    T x[L21_SEG_LOADS];
#pragma unroll
    for (int u = 0; u < L21_SEG_LOADS; ++u) x[u] = src[t + u * BLOCK];
#pragma unroll
    for (int u = 0; u < L21_SEG_LOADS; ++u) f(t + u * BLOCK, x[u]);
  }
  for (; t < L; t += BLOCK) f(t, src[t]);
}

// Thresholds of all frames from the group norms g (frame k at g + k L, contiguous): theta[k], need[k] (l21_seg_decide) and
// asum_out[k] = (T)asum_k.  OBSERVE: pass 1 only, asum_out alone is written.  Every thread of the workgroup holds the same totals after
// a reduction, so the iteration's state is uniform and the loop needs no vote.  A thread re-reads from LDS only what it wrote itself.
template <typename T, bool VEC, bool OBSERVE>
__global__ __launch_bounds__(BLOCK) void k_l21_frames(L21SegPlan p, unsigned L, unsigned nframes, const T* __restrict__ g, T tau,
                                                      const T* __restrict__ rmax, T* __restrict__ theta, int* __restrict__ need,
                                                      T* __restrict__ asum_out, int* __restrict__ passes) {
  static_assert(BLOCK == 256, "four waves: segn_sum2 adds four wave totals");
  extern __shared__ __align__(16) unsigned char l21_seg_lds[];
  __shared__ double red[3 * BLOCK];
  T* const sm = reinterpret_cast<T*>(l21_seg_lds);
  for (unsigned k = blockIdx.x; k < nframes; k += gridDim.x) {
    const T* const gk = g + (size_t)k * L;
    if constexpr (VEC) tau = rmax[k];
    double asum = 0, unused = 0, gmin = (double)INFINITY;
    l21_seg_each<T>(gk, L, [&](unsigned t, T x) {
      if (!OBSERVE && p.lds) sm[t] = x;
      const double a = (double)x;
      asum += a;
      gmin = a < gmin ? a : gmin;
    });
    segn_sum2(asum, unused, 1, red);
    if (threadIdx.x == 0) asum_out[k] = (T)asum;
    if constexpr (OBSERVE) continue;
    gmin = segn_min(gmin, 1, red);
    const int act = l21_seg_decide<T>(asum, tau, VEC);
    auto each = [&](auto&& f) {        // (two calls, so that the loads keep their address space)
      if (p.lds) l21_seg_each<T>(sm, L, f);
      else l21_seg_each<T>(gk, L, f);
    };
    T th = T(0);
    int np = 0;
    if (act == 1) {
      L1SegState st = l1_seg_start(asum, (double)tau, (long long)L);
      for (unsigned it = 0; it <= L + 1 && !st.done; ++it) {
        double S = 0, C = 0;
        each([&](unsigned, T x) {
          const double a = (double)x;
          if (a > st.theta) { S += a; C += 1.0; }
        });
        segn_sum2(S, C, 1, red);
        l1_seg_step(st, S, C, (double)tau);
        ++np;
      }
      th = l21_seg_theta_search<T>(st, asum, gmin, tau, (long long)L);
      if constexpr (sizeof(T) == 8) {
        L21Sum S{0.0, 0.0};
        double C = 0;
        each([&](unsigned, T x) {
          const double a = (double)x;
          if (a > (double)th) { l21_sum_add(S, a); C += 1.0; }
        });
        l21_tree_merge<BLOCK>(S, C, red);
        th = (T)l21_seg_theta_final((double)th, S, C, (double)tau, (long long)L);
      }
    }
    if (threadIdx.x == 0) {
      theta[k] = th;
      need[k] = act;
      passes[k] = np;
    }
  }
}
#endif

}  // namespace sipx
