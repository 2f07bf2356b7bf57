// Group norms across the blocks of a multi-block operator: the l2,1 ball on the range of the TV operator (isotropic total
// variation, EXT_L21).  The rule is written down in l21.h; here are the two streaming kernels and the projector (BallProj)
//     k_l21_norms    g[p] <- the l2 norm of the group of grid point p              reads nblk N words, writes N
//     the engine's l1 threshold search on the array g (K<T>::proj_scalars_arr)     its passes over N words
//     k_l21_scale     v_q[p] <- v_q[p] * f_p unless the search found v inside     reads (nblk + 1) N words, writes nblk N
// -- (2 nblk + 2) N words plus the search per projection outside the set.  The reference package has no such projector.
// Float64 only: between the search and k_l21_scale, k_l21_theta_part / k_l21_theta_final re-evaluate the threshold on the search's
// active set in twice the working precision (one more pass over g, N words; l21.h THRESHOLD IN FLOAT64).
//
// Both kernels are grid-stride over the N grid points with 32-bit index arithmetic (N < 2^31 is checked when the projector is
// built), use no LDS, and take VW points per thread: 16 bytes of every array when n1 % 4 == 0 (then N and every block base
// are 16-byte aligned and the VW points lie on one grid line), one point otherwise.  g lives in the projector's own memory.
// The ball whose groups span the frames (EXT_L21_JOINT, l21_joint.h) is the same projector with norms kernels of its own and L = n1 n2
// entries of g; the ball of every z-slice of TV_xy (EXT_L21_SEG, l21_seg.h, FrameProj) has k_l21_frames in place of the search.
// Built with one weight per group (ExtSpec::weighted, l21_weighted.h) BallProj takes a route of its own after the norms launch: Michelot
// passes k_l21w_part / k_l21w_finish in batches gated on a device flag, then k_l21w_scale; without weights not one launch differs.
// The ball whose groups are the fibers or slices of a one-block operator's range (EXT_L21_GROUPS, l21_groups.h, GroupsProj) shares only the
// weighted iteration (L21WSearch): its norms and its scale kernel are its own.
// Group cardinality on the same fibers or slices (EXT_CARD_GROUPS, card_groups.h, CardGroupsProj) shares that norms launch (GroupNorms) and
// the coordinate -> segment arithmetic of the scale kernel; it selects by rank counting in one workgroup (k_cardg_rank) or by the engine's
// cardinality search, and its apply kernel (k_cardg_zero) only stores.
// The l2,0 sets on the groups of the TV / TV_xy operator (EXT_L20, EXT_L20_SEG, EXT_L20_JOINT, l20.h, L20Proj and L20FrameProj) take the norms
// launch of the l2,1 balls as their key, the selection of group cardinality (CardgSelect, which CardGroupsProj holds too) or, per frame, a
// radix select in one workgroup per frame (k_l20_frames), and a store-only apply across the blocks (k_l20_zero).
// Total nuclear variation (EXT_TNV, tnv.h, TnvProj) has the groups and the z-march of the joint ball, two numbers per pixel in the search
// and a 2 x 2 matrix per pixel in place of the weight.
// The weighted l1 ball on the rows of an operator (EXT_L1_WEIGHTED, l1_weighted.h, L1WProj) is the weighted iteration once more, on the pairs
// (|v_i|, w_i) of the flat padded array: a pass kernel that reads v itself (k_l1w_part) and a soft-threshold apply (k_l1w_apply).
// The ball whose groups run across the equal-sized blocks of a caller-supplied stacked operator (EXT_L21_STACKED, l21_stacked.h: the Hessian
// of second-order TV) is BallProj once more with k_l21s_norms / k_l21s_scale in place of the TV kernels: no coordinates, no pads.
// The l2,inf ball on the same groups (EXT_L2INF, EXT_L2INF_JOINT, EXT_L2INF_STACKED, l2inf.h, L2InfProj) bounds every group norm on its own:
// no search at all, one sweep that takes the norm, decides and scales (k_l2inf_clip / k_l2infs_clip), the joint set the z-march and
// k_l2inf_scale.
// Order of the file: the kernels, the checks of a spec, one launcher per kernel (l21_norms, l21_scale, l21_frames), the projectors.
// A projector's observe() runs the norms launch and the first sum of its own project(): what it reports is what project() decides on.
#include <atomic>

#include "ext_family.h"
#include "l21.h"
#include "l21_joint.h"
#include "l21_seg.h"
#include "l21_stacked.h"
#include "l2inf.h"
#include "l21_groups.h"
#include "card_groups.h"
#include "l20.h"
#include "l21_weighted.h"
#include "l1_weighted.h"
#include "tnv.h"

namespace sipx {

struct L21Args {
  Grid G;
  int dir[3];             // direction of block q
  long long bstride;      // block q starts at v + q * bstride
};

template <typename T>
constexpr int l21_vec_width() { return 16 / (int)sizeof(T); }

// membership of the VW points p .. p + VW - 1 (one grid line) in block q: along axis 0 it differs from point to point
template <int VW>
__device__ __forceinline__ void l21_members(const L21Args& a, const Coord& c, int q, bool (&mem)[VW]) {
  const int d = a.dir[q];
  const int cd = coord_of(c, d), nd = (int)a.G.n[d];
#pragma unroll
  for (int k = 0; k < VW; ++k) mem[k] = l21_member(cd + (d == 0 ? k : 0), nd);
}

template <typename T, int NBLK, int VW>
__global__ __launch_bounds__(BLOCK) void k_l21_norms(L21Args a, const T* __restrict__ v, T* __restrict__ g) {
  const unsigned nvec = (unsigned)(a.G.N / VW), step = gridDim.x * BLOCK;
  for (unsigned vi = blockIdx.x * BLOCK + threadIdx.x; vi < nvec; vi += step) {
    const unsigned p = vi * VW;
    const Coord c = coords(a.G, (long long)p);
    double ss[VW];
#pragma unroll
    for (int k = 0; k < VW; ++k) ss[k] = 0.0;
#pragma unroll
    for (int q = 0; q < NBLK; ++q) {
      bool mem[VW];
      l21_members<VW>(a, c, q, mem);
      const Vec<T, VW> x = ldv<T, VW>(v + (size_t)q * (size_t)a.bstride + p);
#pragma unroll
      for (int k = 0; k < VW; ++k) ss[k] += l21_square<T>(x.v[k], mem[k]);
    }
    Vec<T, VW> out;
#pragma unroll
    for (int k = 0; k < VW; ++k) out.v[k] = l21_norm_of<T>(ss[k]);
    stv<T, VW>(g + p, out);
  }
}

// FRAMES (EXT_L21_SEG, l21_seg.h): every z-slice has its own threshold and decision, theta[k] / need[k] of k_l21_frames at the z
// coordinate of the VW points (one grid line: one frame); a frame with need == 0 is skipped without a store, need == 3 is zeroed
// JOINT (EXT_L21_JOINT, l21_joint.h): g holds one norm per pixel, the weight of grid point p is read at its pixel index p - k L
template <typename T, int NBLK, int VW, bool FRAMES, bool JOINT = false>
__global__ __launch_bounds__(BLOCK) void k_l21_scale(L21Args a, T* __restrict__ v, const T* __restrict__ g,
                                                     const ProjScalars<T>* __restrict__ ps, const T* __restrict__ theta,
                                                     const int* __restrict__ need) {
  T th = T(0);
  if constexpr (!FRAMES) {
    if (!ps->need) return;
    th = theta ? theta[0] : ps->theta;                // (Float64: the threshold k_l21_theta_final left)
  }
  const unsigned nvec = (unsigned)(a.G.N / VW), step = gridDim.x * BLOCK;
  for (unsigned vi = blockIdx.x * BLOCK + threadIdx.x; vi < nvec; vi += step) {
    const unsigned p = vi * VW;
    const Coord c = coords(a.G, (long long)p);
    bool zero = false;
    if constexpr (FRAMES) {
      const int act = need[c.k];
      if (!act) continue;
      th = theta[c.k];
      zero = act == 3;
    }
    const Vec<T, VW> gv = ldv<T, VW>(g + (JOINT ? p - (unsigned)c.k * (unsigned)a.G.st[2] : p));
    T f[VW];
#pragma unroll
    for (int k = 0; k < VW; ++k) f[k] = l21_weight<T>(gv.v[k], th);
#pragma unroll
    for (int q = 0; q < NBLK; ++q) {
      bool mem[VW];
      l21_members<VW>(a, c, q, mem);
      T* vq = v + (size_t)q * (size_t)a.bstride + p;
      Vec<T, VW> x = ldv<T, VW>(vq);
#pragma unroll
      for (int k = 0; k < VW; ++k) x.v[k] = FRAMES && zero ? T(0) : x.v[k] * f[k];
      bool all = true;
#pragma unroll
      for (int k = 0; k < VW; ++k) all = all && mem[k];
      if (all) {
        stv<T, VW>(vq, x);
      } else {            // the far face along dir[q]: rows the block does not have are not written
#pragma unroll
        for (int k = 0; k < VW; ++k)
          if (mem[k]) vq[k] = x.v[k];
      }
    }
  }
}

// ---- Float64: the threshold of the search's active set, correctly rounded (l21.h) ---------------------------------------------------
// k_l21_theta_part: every thread adds the g[p] > theta of its grid-stride share with the error term of every addition kept, the
// workgroup adds its threads' pairs in a fixed tree: part[3 b .. 3 b + 2] = (sum, error term, count) of workgroup b.
// k_l21_theta_final (one workgroup): the same tree over the workgroups' pairs, then theta = (S - tau) / C from the pair.
constexpr int L21_THETA_GRID = 512;
__global__ __launch_bounds__(BLOCK) void k_l21_theta_part(unsigned N, const double* __restrict__ g, const ProjScalars<double>* __restrict__ ps,
                                                          double* __restrict__ part) {
  if (!ps->need) return;
  __shared__ double red[3 * BLOCK];
  const double th = ps->theta;
  L21Sum acc{0.0, 0.0};
  double cnt = 0.0;
  for (unsigned p = blockIdx.x * BLOCK + threadIdx.x; p < N; p += gridDim.x * BLOCK) {
    const double a = g[p];
    if (a > th) { l21_sum_add(acc, a); cnt += 1.0; }
  }
  l21_tree_merge<BLOCK>(acc, cnt, red);
  if (threadIdx.x == 0) { part[3 * blockIdx.x] = acc.hi; part[3 * blockIdx.x + 1] = acc.lo; part[3 * blockIdx.x + 2] = cnt; }
}
__global__ __launch_bounds__(BLOCK) void k_l21_theta_final(int nparts, unsigned N, double tau, const double* __restrict__ part,
                                                           const ProjScalars<double>* __restrict__ ps, double* __restrict__ theta) {
  __shared__ double red[3 * BLOCK];
  if (!ps->need) {
    if (threadIdx.x == 0) theta[0] = ps->theta;
    return;
  }
  L21Sum acc{0.0, 0.0};
  double cnt = 0.0;
  for (int b = threadIdx.x; b < nparts; b += BLOCK) {
    l21_sum_merge(acc, L21Sum{part[3 * b], part[3 * b + 1]});
    cnt += part[3 * b + 2];
  }
  l21_tree_merge<BLOCK>(acc, cnt, red);
  if (threadIdx.x == 0) theta[0] = l21_theta_refined(acc, cnt, tau, (double)N, ps->theta);
}

// out[0] <- (T) ||g||_1 as the search's first pass summed it: the number its decision compares with the radius
template <typename T>
__global__ void k_l21_pick(const ProjScalars<T>* __restrict__ ps, T* __restrict__ out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) out[0] = (T)ps->asum;
}

// ---- the ball across the blocks of a stacked operator (l21_stacked.h, EXT_L21_STACKED) ----------------------------------------------------
//     k_l21s_norms    g[p] <- the l2 norm of { v[q G + p] : q < B }                          reads B G words, writes G
//     k_l21s_scale    v[q G + p] <- v[q G + p] * f_p unless the search found v inside         reads (B + 1) G words, writes B G
// Grid-stride over the G groups with 32-bit indices (B G < 2^31 is checked when the projector is built), no LDS, VW consecutive groups per
// thread: 16 bytes of every block and of g when G % VW == 0 (then every block base q G is 16-byte aligned), one group otherwise.  Every
// position is a member, so there is no coordinate arithmetic and no partial store.  NBLK = 3 and 6 (the Hessian of a 2-D / 3-D grid) are
// compiled as constants, NBLK = 0 loops over the runtime B.
template <typename T, int NBLK, int VW>
__global__ __launch_bounds__(BLOCK) void k_l21s_norms(unsigned G, int B, const T* __restrict__ v, T* __restrict__ g) {
  const int nb = NBLK > 0 ? NBLK : B;
  const unsigned nvec = G / VW, step = gridDim.x * BLOCK;
  for (unsigned vi = blockIdx.x * BLOCK + threadIdx.x; vi < nvec; vi += step) {
    const unsigned p = vi * VW;
    double ss[VW];
#pragma unroll
    for (int k = 0; k < VW; ++k) ss[k] = 0.0;
#pragma unroll
    for (int q = 0; q < nb; ++q) {
      const Vec<T, VW> x = ldv<T, VW>(v + l21s_index((unsigned)q, G, p));
#pragma unroll
      for (int k = 0; k < VW; ++k) ss[k] = l21s_add_square<T>(ss[k], x.v[k]);
    }
    Vec<T, VW> out;
#pragma unroll
    for (int k = 0; k < VW; ++k) out.v[k] = l21_norm_of<T>(ss[k]);
    stv<T, VW>(g + p, out);
  }
}
template <typename T, int NBLK, int VW>
__global__ __launch_bounds__(BLOCK) void k_l21s_scale(unsigned G, int B, T* __restrict__ v, const T* __restrict__ g,
                                                      const ProjScalars<T>* __restrict__ ps, const T* __restrict__ theta) {
  if (!ps->need) return;
  const T th = theta ? theta[0] : ps->theta;          // (Float64: the threshold k_l21_theta_final left)
  const int nb = NBLK > 0 ? NBLK : B;
  const unsigned nvec = G / VW, step = gridDim.x * BLOCK;
  for (unsigned vi = blockIdx.x * BLOCK + threadIdx.x; vi < nvec; vi += step) {
    const unsigned p = vi * VW;
    const Vec<T, VW> gv = ldv<T, VW>(g + p);
    T f[VW];
#pragma unroll
    for (int k = 0; k < VW; ++k) f[k] = l21_weight<T>(gv.v[k], th);
#pragma unroll
    for (int q = 0; q < nb; ++q) {
      T* vq = v + l21s_index((unsigned)q, G, p);
      Vec<T, VW> x = ldv<T, VW>(vq);
#pragma unroll
      for (int k = 0; k < VW; ++k) x.v[k] = l21s_scaled<T>(x.v[k], f[k]);
      stv<T, VW>(vq, x);
    }
  }
}

// ---- the l2,inf ball (l2inf.h): ||v_p||_2 <= c_p for every group, EXT_L2INF, EXT_L2INF_JOINT, EXT_L2INF_STACKED ----------------------------
//     k_l2inf_clip     TV / TV_xy: norm, decision and scaling of VW grid points in one sweep      reads nblk N (+ N) words, writes <= nblk N
//     k_l2infs_clip    the same across the B blocks of a stacked operator                          reads B G (+ G) words, writes <= B G
//     k_l2inf_scale    the joint set: g per pixel from the z-march of the l2,1 ball (l21_norms)    reads 2 N + L (+ L) words, writes <= 2 N
//     k_l2inf_max_part / k_l2inf_max_final   the observer: max_p g_p in two stages, fixed order    reads the groups' words of g
// No search and no ProjScalars: the bound is the scalar c, or VEC: one entry of cv per group.  The clip kernels keep the NBLK (stacked: up
// to L21S_MAX_BLOCKS) blocks of their VW groups in registers between the load and the store, so v is read once; a thread none of whose VW
// groups is clipped stores nothing, and in a stored vector the lanes of unclipped groups carry the bits they were loaded with.  Launch
// shapes, index width and the 16-byte rule are those of k_l21_scale / k_l21s_scale; no LDS outside the observer, no scratch.
template <typename T, int NBLK, int VW, bool VEC>
__global__ __launch_bounds__(BLOCK) void k_l2inf_clip(L21Args a, T* __restrict__ v, const T* __restrict__ cv, T c) {
  const unsigned nvec = (unsigned)(a.G.N / VW), step = gridDim.x * BLOCK;
  for (unsigned vi = blockIdx.x * BLOCK + threadIdx.x; vi < nvec; vi += step) {
    const unsigned p = vi * VW;
    const Coord co = coords(a.G, (long long)p);
    Vec<T, VW> x[NBLK];
    bool mem[NBLK][VW];
    double ss[VW];
#pragma unroll
    for (int k = 0; k < VW; ++k) ss[k] = 0.0;
#pragma unroll
    for (int q = 0; q < NBLK; ++q) {
      l21_members<VW>(a, co, q, mem[q]);
      x[q] = ldv<T, VW>(v + (size_t)q * (size_t)a.bstride + p);
#pragma unroll
      for (int k = 0; k < VW; ++k) ss[k] += l21_square<T>(x[q].v[k], mem[q][k]);
    }
    Vec<T, VW> cc;
    if constexpr (VEC) cc = ldv<T, VW>(cv + p);
    T f[VW];
    bool clip[VW], any = false;
#pragma unroll
    for (int k = 0; k < VW; ++k) {
      const T g = l21_norm_of<T>(ss[k]), ck = VEC ? cc.v[k] : c;
      clip[k] = l2inf_clipped<T>(g, ck);
      f[k] = clip[k] ? l2inf_factor<T>(g, ck) : T(1);
      any = any || clip[k];
    }
    if (!any) continue;
#pragma unroll
    for (int q = 0; q < NBLK; ++q) {
      T* vq = v + (size_t)q * (size_t)a.bstride + p;
      bool all = true;
#pragma unroll
      for (int k = 0; k < VW; ++k) {
        if (clip[k]) x[q].v[k] = l2inf_scaled<T>(x[q].v[k], f[k]);
        all = all && mem[q][k];
      }
      if (all) {
        stv<T, VW>(vq, x[q]);
      } else {            // the far face along dir[q]: rows the block does not have are not written
#pragma unroll
        for (int k = 0; k < VW; ++k)
          if (mem[q][k] && clip[k]) vq[k] = x[q].v[k];
      }
    }
  }
}
// NBLK = 3 and 6 (the Hessian of a 2-D / 3-D grid) are compiled as constants; NBLK = 0 takes the runtime B through a loop unrolled to
// L21S_MAX_BLOCKS with a guard on q < B, which keeps every block in a register of its own: v is not re-read
template <typename T, int NBLK, int VW, bool VEC>
__global__ __launch_bounds__(BLOCK) void k_l2infs_clip(unsigned G, int B, T* __restrict__ v, const T* __restrict__ cv, T c) {
  constexpr int NQ = NBLK > 0 ? NBLK : L21S_MAX_BLOCKS;
  const int nb = NBLK > 0 ? NBLK : B;
  const unsigned nvec = G / VW, step = gridDim.x * BLOCK;
  for (unsigned vi = blockIdx.x * BLOCK + threadIdx.x; vi < nvec; vi += step) {
    const unsigned p = vi * VW;
    Vec<T, VW> x[NQ];
    double ss[VW];
#pragma unroll
    for (int k = 0; k < VW; ++k) ss[k] = 0.0;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      if (q < nb) {
        x[q] = ldv<T, VW>(v + l21s_index((unsigned)q, G, p));
#pragma unroll
        for (int k = 0; k < VW; ++k) ss[k] = l21s_add_square<T>(ss[k], x[q].v[k]);
      }
    }
    Vec<T, VW> cc;
    if constexpr (VEC) cc = ldv<T, VW>(cv + p);
    T f[VW];
    bool clip[VW], any = false;
#pragma unroll
    for (int k = 0; k < VW; ++k) {
      const T g = l21_norm_of<T>(ss[k]), ck = VEC ? cc.v[k] : c;
      clip[k] = l2inf_clipped<T>(g, ck);
      f[k] = clip[k] ? l2inf_factor<T>(g, ck) : T(1);
      any = any || clip[k];
    }
    if (!any) continue;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      if (q < nb) {
#pragma unroll
        for (int k = 0; k < VW; ++k)
          if (clip[k]) x[q].v[k] = l2inf_scaled<T>(x[q].v[k], f[k]);
        stv<T, VW>(v + l21s_index((unsigned)q, G, p), x[q]);
      }
    }
  }
}
// JOINT: g holds one norm per pixel (and cv one bound), read at the pixel index p - k L of grid point p as k_l21_scale<..., JOINT = true> does
template <typename T, int NBLK, int VW, bool VEC, bool JOINT>
__global__ __launch_bounds__(BLOCK) void k_l2inf_scale(L21Args a, T* __restrict__ v, const T* __restrict__ g, const T* __restrict__ cv, T c) {
  const unsigned nvec = (unsigned)(a.G.N / VW), step = gridDim.x * BLOCK;
  for (unsigned vi = blockIdx.x * BLOCK + threadIdx.x; vi < nvec; vi += step) {
    const unsigned p = vi * VW;
    const Coord co = coords(a.G, (long long)p);
    const unsigned pg = JOINT ? p - (unsigned)co.k * (unsigned)a.G.st[2] : p;
    const Vec<T, VW> gv = ldv<T, VW>(g + pg);
    Vec<T, VW> cc;
    if constexpr (VEC) cc = ldv<T, VW>(cv + pg);
    T f[VW];
    bool clip[VW], any = false;
#pragma unroll
    for (int k = 0; k < VW; ++k) {
      const T ck = VEC ? cc.v[k] : c;
      clip[k] = l2inf_clipped<T>(gv.v[k], ck);
      f[k] = clip[k] ? l2inf_factor<T>(gv.v[k], ck) : T(1);
      any = any || clip[k];
    }
    if (!any) continue;            // nothing of v is read or written where no group is clipped
#pragma unroll
    for (int q = 0; q < NBLK; ++q) {
      bool mem[VW];
      l21_members<VW>(a, co, q, mem);
      T* vq = v + (size_t)q * (size_t)a.bstride + p;
      Vec<T, VW> x = ldv<T, VW>(vq);
      bool all = true;
#pragma unroll
      for (int k = 0; k < VW; ++k) {
        if (clip[k]) x.v[k] = l2inf_scaled<T>(x.v[k], f[k]);
        all = all && mem[k];
      }
      if (all) {
        stv<T, VW>(vq, x);
      } else {
#pragma unroll
        for (int k = 0; k < VW; ++k)
          if (mem[k] && clip[k]) vq[k] = x.v[k];
      }
    }
  }
}
// the observer: the maximum of g (n entries, all >= 0) -- every workgroup the maximum of its grid-stride share into part[block], then one
// workgroup the maximum of the partials; the tree over the BLOCK threads is the same in both.  No atomics.
template <typename T>
__device__ __forceinline__ T l2inf_block_max(T m, T* red) {
  red[threadIdx.x] = m;
  __syncthreads();
  for (int w = BLOCK / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      const T o = red[threadIdx.x + w];
      if (o > red[threadIdx.x]) red[threadIdx.x] = o;
    }
    __syncthreads();
  }
  return red[0];
}
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_l2inf_max_part(unsigned n, const T* __restrict__ g, T* __restrict__ part) {
  __shared__ T red[BLOCK];
  T m = T(0);
  for (unsigned p = blockIdx.x * BLOCK + threadIdx.x; p < n; p += gridDim.x * BLOCK) {
    const T a = g[p];
    if (a > m) m = a;
  }
  m = l2inf_block_max<T>(m, red);
  if (threadIdx.x == 0) part[blockIdx.x] = m;
}
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_l2inf_max_final(int nparts, const T* __restrict__ part, T* __restrict__ out) {
  __shared__ T red[BLOCK];
  T m = T(0);
  for (int b = threadIdx.x; b < nparts; b += BLOCK) {
    const T a = part[b];
    if (a > m) m = a;
  }
  m = l2inf_block_max<T>(m, red);
  if (threadIdx.x == 0) out[0] = m;
}

// ---- the weighted ball (l21_weighted.h): one weight per group, EXT_L21 and EXT_L21_JOINT built with ExtSpec::weighted ---------------------
//     k_l21w_part    one Michelot pass: the sums (S, C, count) of the groups in A_k, one partial per workgroup   reads 2 n words
//     k_l21w_finish   one workgroup: the partials in the same tree, then l21w_start / l21w_step on the device state
//     k_l21w_scale    k_l21_scale with w read alongside g; groups of weight 0 are skipped without a load or a store of v
// Both pass kernels return at once when the state says done, so the host enqueues them in batches and reads one word per batch
// (L21WSearch::run).  FIRST: the pass over every group, which also gives asum and the decision; the state is not read.
constexpr int L21W_GRID = 1024;        // most workgroups of a pass: four per compute unit, 5 doubles of partials each
constexpr int L21W_LOADS = 4;          // loads of g and of w a lane issues before it uses the first (16 bytes or one entry each)
constexpr int L21W_BATCH = 8;          // passes enqueued per read of the flag
// entries one sweep of the pass kernel's unrolled loop covers at full grid: beyond it a thread takes a second round
template <typename T>
constexpr long long l21w_sweep(bool wide) { return (long long)L21W_GRID * BLOCK * L21W_LOADS * (wide ? l21_vec_width<T>() : 1); }

template <typename T, int VW, bool FIRST>
__global__ __launch_bounds__(BLOCK) void k_l21w_part(unsigned n, const T* __restrict__ g, const T* __restrict__ w,
                                                     const L21WState* __restrict__ st, double* __restrict__ part) {
  if (!FIRST && st->done) return;
  __shared__ double red[5 * BLOCK];
  const double th = FIRST ? 0.0 : st->theta;
  const unsigned nvec = n / VW, step = gridDim.x * BLOCK;
  L21WSums a;
  auto take = [&](const Vec<T, VW>& gv, const Vec<T, VW>& wv) {
#pragma unroll
    for (int k = 0; k < VW; ++k) {
      const T wk = l21w_clean<T>(wv.v[k]);
      if (FIRST || l21w_active<T>(gv.v[k], wk, th)) l21w_add<T>(a, gv.v[k], wk);
    }
  };
  unsigned vi = blockIdx.x * BLOCK + threadIdx.x;
  for (; vi + (L21W_LOADS - 1) * step < nvec; vi += L21W_LOADS * step) {
    Vec<T, VW> gv[L21W_LOADS], wv[L21W_LOADS];
#pragma unroll
    for (int u = 0; u < L21W_LOADS; ++u) {
      gv[u] = ldv<T, VW>(g + (size_t)(vi + u * step) * VW);
      wv[u] = ldv<T, VW>(w + (size_t)(vi + u * step) * VW);
    }
#pragma unroll
    for (int u = 0; u < L21W_LOADS; ++u) take(gv[u], wv[u]);
  }
  for (; vi < nvec; vi += step) take(ldv<T, VW>(g + (size_t)vi * VW), ldv<T, VW>(w + (size_t)vi * VW));
  l21w_tree<BLOCK>(a, red);
  if (threadIdx.x == 0) {
    double* o = part + 5 * (size_t)blockIdx.x;
    o[0] = a.S.hi; o[1] = a.S.lo; o[2] = a.C.hi; o[3] = a.C.lo; o[4] = a.cnt;
  }
}
// flag[0] <- the passes so far once the iteration is done, 0 before: the one word the host reads
template <typename T, bool FIRST>
__global__ __launch_bounds__(BLOCK) void k_l21w_finish(int nparts, T tau, const double* __restrict__ part, L21WState* __restrict__ st,
                                                       T* __restrict__ theta, int* __restrict__ flag) {
  if (!FIRST && st->done) return;
  __shared__ double red[5 * BLOCK];
  L21WSums a;
  for (int b = threadIdx.x; b < nparts; b += BLOCK) {
    const double* o = part + 5 * (size_t)b;
    L21WSums x;
    x.S = L21Sum{o[0], o[1]}; x.C = L21Sum{o[2], o[3]}; x.cnt = o[4];
    l21w_merge(a, x);
  }
  l21w_tree<BLOCK>(a, red);
  if (threadIdx.x == 0) {
    L21WState s{};
    T th = T(0);
    if constexpr (FIRST) {
      l21w_start<T>(s, th, a, tau);
    } else {
      s = *st;
      l21w_step<T>(s, th, a, tau);
    }
    *st = s;
    if (s.done) theta[0] = th;
    flag[0] = s.done ? s.passes : 0;
  }
}
template <typename T>
__global__ void k_l21w_pick(const L21WState* __restrict__ st, T* __restrict__ out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) out[0] = (T)st->asum;
}
template <typename T, int NBLK, int VW, bool JOINT>
__global__ __launch_bounds__(BLOCK) void k_l21w_scale(L21Args a, T* __restrict__ v, const T* __restrict__ g, const T* __restrict__ w,
                                                      const L21WState* __restrict__ st, const T* __restrict__ theta) {
  if (!st->need) return;
  const T th = theta[0];
  const unsigned nvec = (unsigned)(a.G.N / VW), step = gridDim.x * BLOCK;
  for (unsigned vi = blockIdx.x * BLOCK + threadIdx.x; vi < nvec; vi += step) {
    const unsigned p = vi * VW;
    const Coord c = coords(a.G, (long long)p);
    const unsigned gi = JOINT ? p - (unsigned)c.k * (unsigned)a.G.st[2] : p;
    const Vec<T, VW> wv = ldv<T, VW>(w + gi);
    T wk[VW];
    bool any = false;
#pragma unroll
    for (int k = 0; k < VW; ++k) {
      wk[k] = l21w_clean<T>(wv.v[k]);
      any = any || wk[k] > T(0);
    }
    if (!any) continue;                // groups of weight 0: f = 1, nothing to do
    const Vec<T, VW> gv = ldv<T, VW>(g + gi);
    T f[VW];
#pragma unroll
    for (int k = 0; k < VW; ++k) f[k] = l21w_factor<T>(gv.v[k], wk[k], th);
#pragma unroll
    for (int q = 0; q < NBLK; ++q) {
      bool mem[VW];
      l21_members<VW>(a, c, q, mem);
      T* vq = v + (size_t)q * (size_t)a.bstride + p;
      Vec<T, VW> x = ldv<T, VW>(vq);
      bool all = true;
#pragma unroll
      for (int k = 0; k < VW; ++k) {
        x.v[k] = wk[k] > T(0) ? x.v[k] * f[k] : x.v[k];      // (weight 0 beside a weighted neighbour: its own bits are stored back)
        all = all && mem[k];
      }
      if (all) {
        stv<T, VW>(vq, x);
      } else {
#pragma unroll
        for (int k = 0; k < VW; ++k)
          if (mem[k] && wk[k] > T(0)) vq[k] = x.v[k];
      }
    }
  }
}

// ---- EXT_L1_WEIGHTED: the weighted l1 ball on the rows of an operator (l1_weighted.h), one weight per row -----------------------------------
// v and w are ONE flat array of n = max(nblk, 1) N entries each: the blocks of the padded layout lie side by side (bstride == N), and
// w holds 0 at every row a block does not have, so neither kernel needs a coordinate.
//     k_l1w_part      k_l21w_part with a = |v| taken in registers: no norms launch, no g array          reads 2 n words
//     k_l21w_finish   as above, unchanged
//     k_l1w_apply     the soft threshold theta w_i; entries of weight 0 are not written                reads 2 n words, writes n
template <typename T, int VW, bool FIRST>
__global__ __launch_bounds__(BLOCK) void k_l1w_part(unsigned n, const T* __restrict__ v, const T* __restrict__ w,
                                                    const L21WState* __restrict__ st, double* __restrict__ part) {
  if (!FIRST && st->done) return;
  __shared__ double red[5 * BLOCK];
  const double th = FIRST ? 0.0 : st->theta;
  const unsigned nvec = n / VW, step = gridDim.x * BLOCK;
  L21WSums a;
  auto take = [&](const Vec<T, VW>& xv, const Vec<T, VW>& wv) {
#pragma unroll
    for (int k = 0; k < VW; ++k) l1w_take<T, FIRST>(a, xv.v[k], l21w_clean<T>(wv.v[k]), th);
  };
  unsigned vi = blockIdx.x * BLOCK + threadIdx.x;
  for (; vi + (L21W_LOADS - 1) * step < nvec; vi += L21W_LOADS * step) {
    Vec<T, VW> xv[L21W_LOADS], wv[L21W_LOADS];
#pragma unroll
    for (int u = 0; u < L21W_LOADS; ++u) {
      xv[u] = ldv<T, VW>(v + (size_t)(vi + u * step) * VW);
      wv[u] = ldv<T, VW>(w + (size_t)(vi + u * step) * VW);
    }
#pragma unroll
    for (int u = 0; u < L21W_LOADS; ++u) take(xv[u], wv[u]);
  }
  for (; vi < nvec; vi += step) take(ldv<T, VW>(v + (size_t)vi * VW), ldv<T, VW>(w + (size_t)vi * VW));
  l21w_tree<BLOCK>(a, red);
  if (threadIdx.x == 0) {
    double* o = part + 5 * (size_t)blockIdx.x;
    o[0] = a.S.hi; o[1] = a.S.lo; o[2] = a.C.hi; o[3] = a.C.lo; o[4] = a.cnt;
  }
}
template <typename T, int VW>
__global__ __launch_bounds__(BLOCK) void k_l1w_apply(unsigned n, T* __restrict__ v, const T* __restrict__ w, const L21WState* __restrict__ st,
                                                     const T* __restrict__ theta) {
  if (!st->need) return;
  const T th = theta[0];
  const unsigned nvec = n / VW, step = gridDim.x * BLOCK;
  for (unsigned vi = blockIdx.x * BLOCK + threadIdx.x; vi < nvec; vi += step) {
    const Vec<T, VW> wv = ldv<T, VW>(w + (size_t)vi * VW);
    T wk[VW];
    bool any = false;
#pragma unroll
    for (int k = 0; k < VW; ++k) {
      wk[k] = l21w_clean<T>(wv.v[k]);
      any = any || wk[k] > T(0);
    }
    if (!any) continue;                // rows of weight 0, pads among them: nothing to do
    T* const p = v + (size_t)vi * VW;
    Vec<T, VW> x = ldv<T, VW>(p);
#pragma unroll
    for (int k = 0; k < VW; ++k) x.v[k] = wk[k] > T(0) ? l1w_shrink<T>(x.v[k], wk[k], th) : x.v[k];      // (weight 0: its own bits go back)
    stv<T, VW>(p, x);
  }
}

// ---- EXT_L21_JOINT: the l2,1 ball whose groups span the frames, on the range of TV_xy (l21_joint.h) ---------------------------------------
//     k_l21j_norms    the z-march: g[pixel] or the chunk sums part[c L + pixel]               reads 2 N words, writes L (or nchunk L doubles)
//     k_l21j_finish   more than one chunk: g[pixel] from the chunk sums, ascending c           reads nchunk L doubles, writes L
//     the engine's l1 threshold search on the L numbers g (and the Float64 refinement above)   its passes over L words
//     k_l21_scale     the JOINT form: the weight of grid point p from g[p - k L]               reads 2 N + L words, writes 2 N
struct L21JArgs {
  Grid G;
  long long bstride;
  L21JointPlan plan;
};
// frames a thread loads before it uses the first: 2 L21J_BATCH loads of 16 bytes (or one entry) in flight per lane, as l21_seg_each
// keeps L21_SEG_LOADS -- a thread's walk is a chain of n3 / L21J_BATCH exposed memory latencies, not n3
constexpr int L21J_BATCH = L21_SEG_LOADS / 2;

// A thread owns the VW consecutive pixels p .. p + VW - 1 (one grid line of the frame) in one chunk and walks the chunk's frames with
// stride L; PART: the float64 chunk sums go to part[c L + p] (k_l21j_finish adds them), otherwise the chunk is the whole z range and
// g is written.  Grid-stride over the nchunk L / VW items; every index stays below N < 2^31.
template <typename T, int VW, bool PART>
__global__ __launch_bounds__(BLOCK) void k_l21j_norms(L21JArgs a, const T* __restrict__ v, T* __restrict__ g, double* __restrict__ part) {
  const unsigned L = (unsigned)a.G.st[2], n3 = (unsigned)a.G.n[2], nvec = L / VW;
  const unsigned items = nvec * (PART ? (unsigned)a.plan.nchunk : 1u), step = gridDim.x * BLOCK;
  const T* const vx = v + (size_t)a.bstride;
  for (unsigned it = blockIdx.x * BLOCK + threadIdx.x; it < items; it += step) {
    const unsigned c = PART ? it / nvec : 0u, p = (it - c * nvec) * VW;
    const Coord cd = coords(a.G, (long long)p);                 // (p < L: the pixel's i, j)
    const bool my = l21_member(cd.j, (int)a.G.n[1]);
    bool mx[VW];
#pragma unroll
    for (int w = 0; w < VW; ++w) mx[w] = l21_member(cd.i + w, (int)a.G.n[0]);
    const unsigned z0 = PART ? (unsigned)a.plan.z0((int)c) : 0u, z1 = PART ? (unsigned)a.plan.z1((int)c, (int)n3) : n3;
    double ss[VW];
#pragma unroll
    for (int w = 0; w < VW; ++w) ss[w] = 0.0;
    unsigned k = z0, off = z0 * L + p;
    for (; k + L21J_BATCH <= z1; k += L21J_BATCH, off += L21J_BATCH * L) {
      Vec<T, VW> y[L21J_BATCH], x[L21J_BATCH];
#pragma unroll
      for (int u = 0; u < L21J_BATCH; ++u) {
        y[u] = ldv<T, VW>(v + off + u * L);
        x[u] = ldv<T, VW>(vx + off + u * L);
      }
#pragma unroll
      for (int u = 0; u < L21J_BATCH; ++u)
#pragma unroll
        for (int w = 0; w < VW; ++w) l21_joint_add<T>(ss[w], y[u].v[w], x[u].v[w], my, mx[w]);
    }
    for (; k < z1; ++k, off += L) {
      const Vec<T, VW> y = ldv<T, VW>(v + off), x = ldv<T, VW>(vx + off);
#pragma unroll
      for (int w = 0; w < VW; ++w) l21_joint_add<T>(ss[w], y.v[w], x.v[w], my, mx[w]);
    }
    if constexpr (PART) {
      double* const dst = part + (size_t)c * L + p;
#pragma unroll
      for (int w = 0; w < VW; ++w) dst[w] = ss[w];
    } else {
      Vec<T, VW> out;
#pragma unroll
      for (int w = 0; w < VW; ++w) out.v[w] = l21_norm_of<T>(ss[w]);
      stv<T, VW>(g + p, out);
    }
  }
}
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_l21j_finish(unsigned L, int nchunk, const double* __restrict__ part, T* __restrict__ g) {
  for (unsigned p = blockIdx.x * BLOCK + threadIdx.x; p < L; p += gridDim.x * BLOCK)
    g[p] = l21_norm_of<T>(l21_joint_total(part, (long long)L, (long long)p, nchunk));
}

// ---- EXT_TNV: the nuclear-norm ball on the 2 x n3 Jacobians of the pixels, on the range of TV_xy (tnv.h) ------------------------------------
//     k_tnv_gram      the z-march of k_l21j_norms with three sums per pixel: (s, rot) of the pixel,   reads 2 N words, writes 4 L
//                     or the chunk sums part[(c W + word) L + pixel], W = 3 (Float64: 6)              (or nchunk W L doubles)
//     k_tnv_finish    more than one chunk: (s, rot) from the chunk sums, ascending c                  reads nchunk W L doubles, writes 4 L
//     the engine's l1 threshold search on the 2 L numbers s (and the Float64 refinement above)         its passes over 2 L words
//     k_tnv_apply     M_p from (s, rot, theta) at the pixel of grid point p, (vy, vx) <- M_p (vy, vx)  reads 2 N + 4 L words, writes 2 N
template <typename T, int VW, bool PART>
__global__ __launch_bounds__(BLOCK) void k_tnv_gram(L21JArgs a, const T* __restrict__ v, T* __restrict__ s, T* __restrict__ rot,
                                                    double* __restrict__ part) {
  const unsigned L = (unsigned)a.G.st[2], n3 = (unsigned)a.G.n[2], nvec = L / VW;
  const unsigned items = nvec * (PART ? (unsigned)a.plan.nchunk : 1u), step = gridDim.x * BLOCK;
  const T* const vx = v + (size_t)a.bstride;
  for (unsigned it = blockIdx.x * BLOCK + threadIdx.x; it < items; it += step) {
    const unsigned c = PART ? it / nvec : 0u, p = (it - c * nvec) * VW;
    const Coord cd = coords(a.G, (long long)p);                 // (p < L: the pixel's i, j)
    const bool my = l21_member(cd.j, (int)a.G.n[1]);
    bool mx[VW];
#pragma unroll
    for (int w = 0; w < VW; ++w) mx[w] = l21_member(cd.i + w, (int)a.G.n[0]);
    const unsigned z0 = PART ? (unsigned)a.plan.z0((int)c) : 0u, z1 = PART ? (unsigned)a.plan.z1((int)c, (int)n3) : n3;
    TnvGram acc[VW];
#pragma unroll
    for (int w = 0; w < VW; ++w) acc[w] = TnvGram{};
    unsigned k = z0, off = z0 * L + p;
    for (; k + L21J_BATCH <= z1; k += L21J_BATCH, off += L21J_BATCH * L) {
      Vec<T, VW> y[L21J_BATCH], x[L21J_BATCH];
#pragma unroll
      for (int u = 0; u < L21J_BATCH; ++u) {
        y[u] = ldv<T, VW>(v + off + u * L);
        x[u] = ldv<T, VW>(vx + off + u * L);
      }
#pragma unroll
      for (int u = 0; u < L21J_BATCH; ++u)
#pragma unroll
        for (int w = 0; w < VW; ++w) tnv_gram_add<T>(acc[w], y[u].v[w], x[u].v[w], my, mx[w]);
    }
    for (; k < z1; ++k, off += L) {
      const Vec<T, VW> y = ldv<T, VW>(v + off), x = ldv<T, VW>(vx + off);
#pragma unroll
      for (int w = 0; w < VW; ++w) tnv_gram_add<T>(acc[w], y.v[w], x.v[w], my, mx[w]);
    }
    if constexpr (PART) {
#pragma unroll
      for (int w = 0; w < VW; ++w) tnv_gram_store<T>(acc[w], part, (long long)L, (long long)(p + w), (int)c);
    } else {
      Vec<T, VW> s1, s2, cs, sn;
#pragma unroll
      for (int w = 0; w < VW; ++w) {
        const TnvPixel<T> o = tnv_decompose<T>(acc[w]);
        s1.v[w] = o.s1; s2.v[w] = o.s2; cs.v[w] = o.cs; sn.v[w] = o.sn;
      }
      stv<T, VW>(s + p, s1);
      stv<T, VW>(s + L + p, s2);
      stv<T, VW>(rot + p, cs);
      stv<T, VW>(rot + L + p, sn);
    }
  }
}
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_tnv_finish(unsigned L, int nchunk, const double* __restrict__ part, T* __restrict__ s,
                                                      T* __restrict__ rot) {
  for (unsigned p = blockIdx.x * BLOCK + threadIdx.x; p < L; p += gridDim.x * BLOCK) {
    const TnvPixel<T> o = tnv_decompose<T>(tnv_gram_total<T>(part, (long long)L, (long long)p, nchunk));
    s[p] = o.s1; s[L + p] = o.s2; rot[p] = o.cs; rot[L + p] = o.sn;
  }
}
// Grid-stride over the N grid points as k_l21_scale, VW points of one grid line (one frame) per thread: the thread builds M_p of its VW
// pixels once and multiplies the pair (vy, vx) of each; nothing at all is read when the search found v inside the ball.  Rows a block
// does not have enter as zeros and are not written.
template <typename T, int VW>
__global__ __launch_bounds__(BLOCK) void k_tnv_apply(L21Args a, T* __restrict__ v, const T* __restrict__ s, const T* __restrict__ rot,
                                                     const ProjScalars<T>* __restrict__ ps, const T* __restrict__ theta) {
  if (!ps->need) return;
  const T th = theta ? theta[0] : ps->theta;                // (Float64: the threshold k_l21_theta_final left)
  const unsigned L = (unsigned)a.G.st[2], nvec = (unsigned)(a.G.N / VW), step = gridDim.x * BLOCK;
  for (unsigned vi = blockIdx.x * BLOCK + threadIdx.x; vi < nvec; vi += step) {
    const unsigned p = vi * VW;
    const Coord c = coords(a.G, (long long)p);
    const unsigned px = p - (unsigned)c.k * L;
    const Vec<T, VW> s1 = ldv<T, VW>(s + px), s2 = ldv<T, VW>(s + L + px), cs = ldv<T, VW>(rot + px), sn = ldv<T, VW>(rot + L + px);
    bool my[VW], mx[VW];
    l21_members<VW>(a, c, 0, my);
    l21_members<VW>(a, c, 1, mx);
    T* const py = v + p;
    T* const pxx = v + (size_t)a.bstride + p;
    Vec<T, VW> y = ldv<T, VW>(py), x = ldv<T, VW>(pxx);
    bool ally = true, allx = true;
#pragma unroll
    for (int k = 0; k < VW; ++k) {
      double m00, m01, m11;
      tnv_matrix<T>(s1.v[k], s2.v[k], cs.v[k], sn.v[k], th, m00, m01, m11);
      T oy, ox;
      tnv_apply_pair<T>(m00, m01, m11, y.v[k], x.v[k], my[k], mx[k], oy, ox);
      y.v[k] = oy; x.v[k] = ox;
      ally = ally && my[k];
      allx = allx && mx[k];
    }
    if (ally) {
      stv<T, VW>(py, y);
    } else {              // the far face along y: rows the block does not have are not written
#pragma unroll
      for (int k = 0; k < VW; ++k)
        if (my[k]) py[k] = y.v[k];
    }
    if (allx) {
      stv<T, VW>(pxx, x);
    } else {
#pragma unroll
      for (int k = 0; k < VW; ++k)
        if (mx[k]) pxx[k] = x.v[k];
    }
  }
}

// ---- EXT_L21_GROUPS: the l2,1 ball whose groups are the fibers or slices of a one-block operator's range (l21_groups.h) ----------------------
//     fibers: k_seg_observe<T, SEGN_L2> (seg_norm.h)      g[s] in segn_pass1's order                     reads N words, writes nseg
//     slices: k_l21g_part                                  one (tile, chunk) per workgroup: its partial    reads N words, writes 2 ntA F nchunk doubles
//             k_l21g_finish                                g[s] from a slice's partials, ascending chunk   reads 2 nseg nchunk doubles, writes nseg
//     k_l21w_part / k_l21w_finish on (g, w), n = nseg      the passes of l21_weighted.h                     passes * 2 nseg words
//     k_l21g_scale                                         coords -> segment -> f_s -> multiply             reads N + up to 2 N words, writes N
struct L21GArgs {
  Grid G;
  int d[3];                   // the valid extents TD_n
  int cs[3];                  // s = i cs[0] + j cs[1] + k cs[2]: the segment of grid point (i, j, k), all six geometries
};

// VW: consecutive element indices a thread takes before it strides (plan.vw); WIDE: they are one 16-byte load (VW > 1, the valid extent
// along x a multiple of VW, 16-byte aligned rows), otherwise VW scalar loads of the same entries in the same order
template <typename T, int VW, bool WIDE>
__global__ __launch_bounds__(BLOCK) void k_l21g_part(SegMap m, L21GroupsPlan p, const T* __restrict__ v, double* __restrict__ part) {
  __shared__ double red[2 * BLOCK];
  const int F = p.F, G = BLOCK >> p.logF;
  const int f = (int)threadIdx.x & (F - 1), r = (int)threadIdx.x >> p.logF;
  const long long c = (long long)blockIdx.x % p.nchunk, tile = (long long)blockIdx.x / p.nchunk;
  const long long sa = tile * F + f;
  const bool live = sa < m.nseg;
  const T* const vs = v + sa * m.sSa;
  const long long t1 = p.t1(c, m.L);
  L21Sum acc{0.0, 0.0};
  if (live)
    for (long long t = p.t0(c) + (long long)r * VW; t < t1; t += (long long)G * VW) {
      if constexpr (WIDE) {
        const Vec<T, VW> x = ldv<T, VW>(vs + seg_toff(m, t));
#pragma unroll
        for (int k = 0; k < VW; ++k) l21g_add_square<T>(acc, x.v[k]);
      } else {
#pragma unroll
        for (int k = 0; k < VW; ++k)
          if (t + k < t1) l21g_add_square<T>(acc, vs[seg_toff(m, t + k)]);
      }
    }
  // the halving tree over the lanes of one slice: thread t merges with t + w, w = BLOCK / 2 .. F (t and t + w share f)
  double *sh = red, *sl = red + BLOCK;
  sh[threadIdx.x] = acc.hi; sl[threadIdx.x] = acc.lo;
  __syncthreads();
  for (int w = BLOCK / 2; w >= F; w >>= 1) {
    if ((int)threadIdx.x < w) {
      L21Sum x{sh[threadIdx.x], sl[threadIdx.x]};
      l21_sum_merge(x, L21Sum{sh[threadIdx.x + w], sl[threadIdx.x + w]});
      sh[threadIdx.x] = x.hi; sl[threadIdx.x] = x.lo;
    }
    __syncthreads();
  }
  if ((int)threadIdx.x < F && live) {
    double* const o = part + 2 * (sa * p.nchunk + c);
    o[0] = sh[threadIdx.x]; o[1] = sl[threadIdx.x];
  }
}
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_l21g_finish(long long nseg, long long nchunk, const double* __restrict__ part, T* __restrict__ g) {
  for (long long s = (long long)blockIdx.x * BLOCK + threadIdx.x; s < nseg; s += (long long)gridDim.x * BLOCK) {
    L21Sum a{0.0, 0.0};
    for (long long c = 0; c < nchunk; ++c) l21_sum_merge(a, L21Sum{part[2 * (s * nchunk + c)], part[2 * (s * nchunk + c) + 1]});
    g[s] = l21g_norm_of<T>(a);
  }
}
// Grid-stride over the padded grid, VW points of one grid line per thread.  A point outside the valid extents, or in a segment of weight
// 0, is neither multiplied nor stored; nothing at all is read when the search found v inside the ball.
template <typename T, int VW>
__global__ __launch_bounds__(BLOCK) void k_l21g_scale(L21GArgs a, T* __restrict__ v, const T* __restrict__ g, const T* __restrict__ w,
                                                      const L21WState* __restrict__ st, const T* __restrict__ theta) {
  if (!st->need) return;
  const T th = theta[0];
  const unsigned nvec = (unsigned)(a.G.N / VW), step = gridDim.x * BLOCK;
  for (unsigned vi = blockIdx.x * BLOCK + threadIdx.x; vi < nvec; vi += step) {
    const unsigned p = vi * VW;
    const Coord c = coords(a.G, (long long)p);
    if (c.j >= a.d[1] || c.k >= a.d[2]) continue;
    const int sb = c.j * a.cs[1] + c.k * a.cs[2];
    T f[VW];
    bool wr[VW], any = false, all = true;
#pragma unroll
    for (int k = 0; k < VW; ++k) {
      wr[k] = false;
      f[k] = T(1);
      const int i = c.i + k;
      if (i < a.d[0]) {
        const int s = sb + i * a.cs[0];
        const T wk = l21w_clean<T>(w[s]);
        if (wk > T(0)) { f[k] = l21w_factor<T>(g[s], wk, th); wr[k] = true; }
      }
      any = any || wr[k];
      all = all && wr[k];
    }
    if (!any) continue;
    Vec<T, VW> x = ldv<T, VW>(v + p);
#pragma unroll
    for (int k = 0; k < VW; ++k) x.v[k] = wr[k] ? x.v[k] * f[k] : x.v[k];
    if (all) {
      stv<T, VW>(v + p, x);
    } else {
#pragma unroll
      for (int k = 0; k < VW; ++k)
        if (wr[k]) v[p + k] = x.v[k];
    }
  }
}

// ---- EXT_CARD_GROUPS: at most k non-zero fibers or slices of a one-block operator's range (card_groups.h) -----------------------------------
//     the norms launch of EXT_L21_GROUPS (GroupNorms)        g[s]                                           reads N words, writes nseg
//     k_cardg_rank, or the engine's cardinality search on g   (need, tau, cut) into a ProjScalars            nseg words, which stay in cache
//     k_cardg_zero                                            coords -> segment -> dropped: +0                reads nseg words, writes <= N
// The small route of the selection: ONE workgroup, g staged in LDS; thread s owns segment s and counts its place r_s in the stable
// descending order (cardg_rank_of).  The places are a permutation, so exactly one segment has r_s == k - 1 and writes (tau, cut); thread 0
// writes need, and the values of "nothing is dropped" when there is none.  No atomics, no host read.
template <typename T>
__global__ __launch_bounds__(CARDG_SMALL_MAX) void k_cardg_rank(int nseg, int k, const T* __restrict__ g, ProjScalars<T>* __restrict__ ps) {
  static_assert(CARDG_SMALL_MAX <= 1024 && CARDG_SMALL_MAX % 64 == 0, "one segment a thread of one workgroup");
  __shared__ T sg[CARDG_SMALL_MAX];
  __shared__ int snz[CARDG_SMALL_MAX / 64];
  const int s = (int)threadIdx.x;
  const T gs = s < nseg ? g[s] : T(0);
  sg[s] = gs;
  int nz = gs > T(0) ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nz += __shfl_down(nz, o, 64);
  if ((threadIdx.x & 63) == 0) snz[threadIdx.x >> 6] = nz;
  __syncthreads();                     // (sg and snz are complete)
  int nnz = 0;
#pragma unroll
  for (int i = 0; i < CARDG_SMALL_MAX / 64; ++i) nnz += snz[i];
  const bool need = k < nseg && nnz > k;
  if (threadIdx.x == 0) {
    ps->need = need ? 1 : 0;
    if (!need) { ps->tau = T(0); ps->quota = CARDG_NO_CUT; }
  }
  if (!need || s >= nseg) return;
  int r = 0;
  for (int t = 0; t < nseg; ++t) {
    const T gt = sg[t];                  // (every lane reads the same word: an LDS broadcast)
    r += (gt > gs || (gt == gs && t < s)) ? 1 : 0;
  }
  if (r == k - 1) { ps->tau = gs; ps->quota = (long long)s; }
}

// Grid-stride over the padded grid, VW points of one grid line per thread, the coordinate -> segment arithmetic of k_l21g_scale.  v is
// never loaded: a dropped segment's entries are stored as +0 -- one 16-byte store where all VW points are valid and dropped, scalar
// stores otherwise -- and a kept segment, a pad, or anything at all when the selection found nothing to drop, is not touched.
template <typename T, int VW>
__global__ __launch_bounds__(BLOCK) void k_cardg_zero(L21GArgs a, T* __restrict__ v, const T* __restrict__ g, const ProjScalars<T>* __restrict__ ps) {
  if (!ps->need) return;
  const T tau = ps->tau;
  const long long cut = ps->quota;
  const unsigned nvec = (unsigned)(a.G.N / VW), step = gridDim.x * BLOCK;
  for (unsigned vi = blockIdx.x * BLOCK + threadIdx.x; vi < nvec; vi += step) {
    const unsigned p = vi * VW;
    const Coord c = coords(a.G, (long long)p);
    if (c.j >= a.d[1] || c.k >= a.d[2]) continue;
    const int sb = c.j * a.cs[1] + c.k * a.cs[2];
    bool drop[VW], any = false, all = true;
#pragma unroll
    for (int q = 0; q < VW; ++q) {
      drop[q] = false;
      const int i = c.i + q;
      if (i < a.d[0]) {
        const int s = sb + i * a.cs[0];
        drop[q] = !cardg_keeps<T>(g[s], (long long)s, tau, cut);
      }
      any = any || drop[q];
      all = all && drop[q];
    }
    if (!any) continue;
    if (all) {
      Vec<T, VW> z;
#pragma unroll
      for (int q = 0; q < VW; ++q) z.v[q] = T(0);
      stv<T, VW>(v + p, z);
    } else {
#pragma unroll
      for (int q = 0; q < VW; ++q)
        if (drop[q]) v[p + q] = T(0);
    }
  }
}

// ---- EXT_L20, EXT_L20_SEG, EXT_L20_JOINT: at most k grid points (pixels) with a non-zero gradient vector (l20.h) ------------------------------
//     the norms launch of the l2,1 ball on the same operator (l21_norms)   g[p], or g[pixel] for the joint set
//     CardgSelect on g, or k_l20_frames per frame                          (need, tau, cut), one triple or one per frame
//     k_l20_zero                                                           reads N words of g (joint: L, which stay in cache), writes <= nblk N
// The loop of k_l21_scale: grid-stride over the N points, VW points of one grid line per thread, l21_members for the pads.  v is never
// loaded: the members of a dropped group are stored as +0 -- one 16-byte store per block where all VW points are members and dropped,
// scalar stores otherwise -- and a kept group, a pad, a frame without need, or anything at all when the selection found nothing to drop, is
// not touched.  The group index the rule compares with the cut: the point index p, the in-frame pixel index (FRAMES) or the pixel index
// (JOINT), both p - k L.  32-bit index arithmetic, no LDS, no atomics.
template <typename T, int NBLK, int VW, bool FRAMES, bool JOINT>
__global__ __launch_bounds__(BLOCK) void k_l20_zero(L21Args a, T* __restrict__ v, const T* __restrict__ g, const ProjScalars<T>* __restrict__ ps,
                                                    const int* __restrict__ need, const T* __restrict__ ftau, const int* __restrict__ fcut) {
  T tau = T(0);
  long long cut = 0;
  if constexpr (!FRAMES) {
    if (!ps->need) return;
    tau = ps->tau;
    cut = ps->quota;
  }
  const unsigned nvec = (unsigned)(a.G.N / VW), step = gridDim.x * BLOCK;
  for (unsigned vi = blockIdx.x * BLOCK + threadIdx.x; vi < nvec; vi += step) {
    const unsigned p = vi * VW;
    const Coord c = coords(a.G, (long long)p);
    if constexpr (FRAMES) {
      if (!need[c.k]) continue;
      tau = ftau[c.k];
      cut = (long long)fcut[c.k];
    }
    const unsigned px = (FRAMES || JOINT) ? p - (unsigned)c.k * (unsigned)a.G.st[2] : p;
    const Vec<T, VW> gv = ldv<T, VW>(g + (JOINT ? px : p));
    bool drop[VW], any = false;
#pragma unroll
    for (int k = 0; k < VW; ++k) {
      drop[k] = !cardg_keeps<T>(gv.v[k], (long long)(px + (unsigned)k), tau, cut);
      any = any || drop[k];
    }
    if (!any) continue;
#pragma unroll
    for (int q = 0; q < NBLK; ++q) {
      bool mem[VW];
      l21_members<VW>(a, c, q, mem);
      T* vq = v + (size_t)q * (size_t)a.bstride + p;
      bool all = true;
#pragma unroll
      for (int k = 0; k < VW; ++k) all = all && mem[k] && drop[k];
      if (all) {
        Vec<T, VW> z;
#pragma unroll
        for (int k = 0; k < VW; ++k) z.v[k] = T(0);
        stv<T, VW>(vq, z);
      } else {            // a kept neighbour, or the far face along dir[q]: rows the block does not have are not written
#pragma unroll
        for (int k = 0; k < VW; ++k)
          if (mem[k] && drop[k]) vq[k] = T(0);
      }
    }
  }
}

// The per-frame selection (l20.h, l20_frame_select): one workgroup per frame, grid-stride over the frames, on g alone (frame f at g + f L).
// The plan of k_l21_frames: the frame's L keys are staged in LDS when they fit seg_norm.h's budget, otherwise every pass re-reads them.
//   1. the count of the keys > 0; at most k of them (k >= L included, then without a read): need = 0
//   2. radix select on the bit pattern, 8 bits a pass, a 256-bin histogram in LDS: tau = the k-th largest key, kk = how many keys equal
//      to it stay.  The bins are LDS atomics (integer: the counts do not depend on the order).  Keys of one frame share their high bytes,
//      so the first passes would send a whole wave to one bin; one round of aggregation takes that out: the lanes that share the bin of
//      the wave's first live lane add once, through that lane, the others add one each.
//   3. cut = the in-frame index of the kk-th key equal to tau.  Where all the keys equal to tau stay (no tie across the k-th place) that
//      is the last of them: one more streamed pass and a max-reduction.  Otherwise one ordered pass, BLOCK keys a step, with wave
//      ballots -- a chain of L / BLOCK dependent loads and barriers, which only an input with ties across the cut pays.
// A budget from device memory that is not >= 1 (every host path refuses it) keeps no group: tau = +inf.  Nothing is kept between calls.
template <typename T> struct L20Bits;
template <> struct L20Bits<float> {
  using U = unsigned int;
  static __device__ __forceinline__ U of(float x) { return __float_as_uint(x); }
  static __device__ __forceinline__ float back(U u) { return __uint_as_float(u); }
};
template <> struct L20Bits<double> {
  using U = unsigned long long;
  static __device__ __forceinline__ U of(double x) { return (U)__double_as_longlong(x); }
  static __device__ __forceinline__ double back(U u) { return __longlong_as_double((long long)u); }
};
constexpr int L20_NO_CUT = 0x7fffffff;      // the cut of a frame where nothing is dropped
template <typename T, bool VEC>
__global__ __launch_bounds__(BLOCK) void k_l20_frames(L21SegPlan p, unsigned L, unsigned nframes, const T* __restrict__ g, T kall,
                                                      const T* __restrict__ kvec, int* __restrict__ need, T* __restrict__ tau,
                                                      int* __restrict__ cut) {
  using B = L20Bits<T>;
  using U = typename B::U;
  constexpr int BITS = (int)sizeof(U) * 8;
  static_assert(BLOCK == 256, "one histogram bin a thread, four waves");
  extern __shared__ __align__(16) unsigned char l20_lds[];
  __shared__ unsigned int hist[256];
  __shared__ unsigned int s_w[BLOCK / 64];
  __shared__ U s_prefix;
  __shared__ unsigned int s_kk, s_neq, s_run, s_cut;
  T* const sm = reinterpret_cast<T*>(l20_lds);
  const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (unsigned f = blockIdx.x; f < nframes; f += gridDim.x) {
    const T* const gf = g + (size_t)f * L;
    const T kf = VEC ? kvec[f] : kall;
    if (kf >= (T)L) {                  // every group of the frame stays (uniform: no thread has read anything)
      if (tid == 0) { need[f] = 0; tau[f] = T(0); cut[f] = L20_NO_CUT; }
      continue;
    }
    const unsigned k = kf >= T(1) ? (unsigned)kf : 0u;
    unsigned nz = 0;
    l21_seg_each<T>(gf, L, [&](unsigned t, T x) {
      if (p.lds) sm[t] = x;
      nz += x > T(0) ? 1u : 0u;
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nz += __shfl_down(nz, o, 64);
    if (lane == 0) s_w[w] = nz;
    __syncthreads();                   // (sm and s_w are complete)
    const unsigned nnz = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    __syncthreads();
    if (nnz <= k || k == 0) {          // uniform
      if (tid == 0) {
        need[f] = k == 0 && nnz > 0 ? 1 : 0;
        tau[f] = k == 0 && nnz > 0 ? (T)INFINITY : T(0);
        cut[f] = k == 0 && nnz > 0 ? -1 : L20_NO_CUT;
      }
      continue;
    }
    auto each = [&](auto&& fn) {       // (two calls, so that the loads keep their address space)
      if (p.lds) l21_seg_each<T>(sm, L, fn);
      else l21_seg_each<T>(gf, L, fn);
    };
    U prefix = 0, mask = 0;
    unsigned kk = k;
    for (int shift = BITS - 8; shift >= 0; shift -= 8) {
      hist[tid] = 0;
      __syncthreads();
      each([&](unsigned, T x) {
        const U key = B::of(x);
        const bool act = (key & mask) == prefix;
        const unsigned bin = (unsigned)(key >> shift) & 255u;
        const unsigned long long live = __ballot(act);
        if (live) {
          const int lead = __ffsll((long long)live) - 1;
          const unsigned lb = (unsigned)__shfl((int)bin, lead, 64);
          const unsigned long long same = __ballot(act && bin == lb);
          if (lane == lead) atomicAdd(&hist[lb], (unsigned)__popcll(same));
          else if (act && bin != lb) atomicAdd(&hist[bin], 1u);
        }
      });
      __syncthreads();
      if (tid == 0) {
        unsigned cum = 0;
        int b = 255;
        for (; b > 0; --b) {
          if (cum + hist[b] >= kk) break;
          cum += hist[b];
        }
        s_prefix = prefix | ((U)b << shift);
        s_kk = kk - cum;
        s_neq = hist[b];               // (after the last pass: the keys equal to tau)
      }
      __syncthreads();
      prefix = s_prefix;
      kk = s_kk;
      mask |= (U)255 << shift;
    }
    // prefix = the bits of the k-th largest key, kk >= 1 of the s_neq keys equal to it stay: the cut is the index of the kk-th of them
    if (kk == s_neq) {                 // uniform.  All of them stay -- no tie across the k-th place, the usual case: the cut is the last
      unsigned last = 0;               // of them, one more streamed pass with its loads in flight and one reduction
      each([&](unsigned t, T x) { last = (B::of(x) == prefix && t > last) ? t : last; });
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const unsigned other = (unsigned)__shfl_down((int)last, o, 64);
        last = other > last ? other : last;
      }
      if (lane == 0) s_w[w] = last;
      __syncthreads();
      if (tid == 0) {
        unsigned m = s_w[0];
        for (int i = 1; i < BLOCK / 64; ++i) m = s_w[i] > m ? s_w[i] : m;
        need[f] = 1; tau[f] = B::back(prefix); cut[f] = (int)m;
      }
      __syncthreads();                 // (s_w, s_neq and sm are free for the next frame)
      continue;
    }
    if (tid == 0) { s_run = 0; s_cut = 0; }
    __syncthreads();
    for (unsigned c0 = 0; c0 < L; c0 += BLOCK) {
      const unsigned t = c0 + (unsigned)tid;
      const bool eq = t < L && B::of(p.lds ? sm[t] : gf[t]) == prefix;
      const unsigned long long bal = __ballot(eq);
      const unsigned rank = (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
      if (lane == 0) s_w[w] = (unsigned)__popcll(bal);
      __syncthreads();
      unsigned off = s_run;
      for (int i = 0; i < w; ++i) off += s_w[i];
      if (eq && off + rank + 1 == kk) s_cut = t;
      const unsigned tot = s_run + s_w[0] + s_w[1] + s_w[2] + s_w[3];
      __syncthreads();
      if (tid == 0) s_run = tot;
      __syncthreads();
      if (tot >= kk) break;            // uniform: the cut is found
    }
    if (tid == 0) { need[f] = 1; tau[f] = B::back(prefix); cut[f] = (int)s_cut; }
    __syncthreads();                   // (s_cut and sm are free for the next frame)
  }
}

static void l21_check_spec(const ExtSpec& sp) {
  if (sp.nblk != 2 && sp.nblk != 3) throw std::runtime_error("the l2,1 ball needs the 2 or 3 blocks of the TV or TV_xy operator");
  if (sp.nblk > sp.ndim) throw std::runtime_error("the l2,1 ball: more blocks than grid dimensions");
  for (int q = 0; q < sp.nblk; ++q)
    for (int r = 0; r < q; ++r)
      if (sp.bdir[q] == sp.bdir[r]) throw std::runtime_error("the l2,1 ball: two blocks along one direction");
  if (sp.G.N >= (1ll << 31)) throw std::runtime_error("the l2,1 ball: the grid needs fewer than 2^31 points");
  if (sp.bstride < sp.G.N) throw std::runtime_error("the l2,1 ball: the blocks overlap");
  for (int q = 0; q < sp.nblk; ++q)
    if (sp.bdir[q] < 0 || sp.bdir[q] >= sp.ndim) throw std::runtime_error("the l2,1 ball: block direction out of range");
}
static void l21_seg_check_spec(const ExtSpec& sp) {
  l21_check_spec(sp);
  if (sp.ndim != 3 || sp.nblk != 2 || sp.bdir[0] != 1 || sp.bdir[1] != 0)
    throw std::runtime_error("the l2,1 ball per frame needs the blocks (D_y, D_x) of the TV_xy operator on a 3-D grid");
  if (sp.mode != SIPX_MODE_SLICE || sp.dir != 2) throw std::runtime_error("the l2,1 ball on TV_xy: frames run along z, the mode is (slice, z)");
}
static void l21_joint_check_spec(const ExtSpec& sp) {
  l21_check_spec(sp);
  if (sp.ndim != 3 || sp.nblk != 2 || sp.bdir[0] != 1 || sp.bdir[1] != 0 || sp.mode != SIPX_MODE_WHOLE)
    throw std::runtime_error(L21_JOINT_ROUTE);
}
static void tnv_check_spec(const ExtSpec& sp) {
  l21_check_spec(sp);
  if (sp.ndim != 3 || sp.nblk != 2 || sp.bdir[0] != 1 || sp.bdir[1] != 0 || sp.mode != SIPX_MODE_WHOLE) throw std::runtime_error(TNV_ROUTE);
  if (sp.weighted || sp.lb || sp.ub) throw std::runtime_error(TNV_NO_WEIGHTS);
}
static L21Args l21_args(const ExtSpec& sp) {
  L21Args a;
  a.G = sp.G;
  a.G.set_fast_div();
  for (int q = 0; q < 3; ++q) a.dir[q] = q < sp.nblk ? sp.bdir[q] : 0;
  a.bstride = sp.bstride;
  return a;
}
// 16-byte accesses: n1 % 4 == 0 (N and every block base then are multiples of 4 entries) and 16-byte aligned arrays
template <typename T>
static bool l21_wide(const ExtSpec& sp, const T* v, const T* g) {
  return sp.G.n[0] % 4 == 0 && sp.bstride % 4 == 0 && aligned16(v, g);
}

// g <- the group norms of v, for every set of the family: N entries by k_l21_norms, or the L entries of EXT_L21_JOINT by the z-march
// (part: the nchunk L doubles of l21_joint_plan when it chunks, not looked at otherwise)
template <typename T>
static void l21_norms(hipStream_t s, const ExtSpec& sp, const T* v, T* g, double* part = nullptr) {
  constexpr int W = l21_vec_width<T>();
  const bool wide = l21_wide(sp, v, g);
  const long long N = sp.G.N, L = sp.G.st[2];
  if (sp.kind != EXT_L21_JOINT && sp.kind != EXT_L20_JOINT && sp.kind != EXT_L2INF_JOINT) {
    void (*const k)(L21Args, const T*, T*) = sp.nblk == 2 ? (wide ? k_l21_norms<T, 2, W> : k_l21_norms<T, 2, 1>)
                                                          : (wide ? k_l21_norms<T, 3, W> : k_l21_norms<T, 3, 1>);
    ObsScope obs(KID_L21_NORMS, s, (double)(sp.nblk + 1) * N * sizeof(T));
    hipLaunchKernelGGL(k, dim3(fit_grid(N / (wide ? W : 1), NB)), dim3(BLOCK), 0, s, l21_args(sp), v, g);
    SIPX_HIP(hipGetLastError());
    return;
  }
  L21JArgs a;
  a.G = sp.G;
  a.G.set_fast_div();
  a.bstride = sp.bstride;
  a.plan = l21_joint_plan(L, sp.G.n[2], (int)sizeof(T));
  const bool chunks = a.plan.nchunk > 1;
  {
    void (*const k)(L21JArgs, const T*, T*, double*) = chunks ? (wide ? k_l21j_norms<T, W, true> : k_l21j_norms<T, 1, true>)
                                                              : (wide ? k_l21j_norms<T, W, false> : k_l21j_norms<T, 1, false>);
    ObsScope obs(KID_L21J_NORMS, s, (double)(2 * N + L) * sizeof(T));
    hipLaunchKernelGGL(k, dim3(fit_grid(L / (wide ? W : 1) * a.plan.nchunk, NB)), dim3(BLOCK), 0, s, a, v, g, part);
    SIPX_HIP(hipGetLastError());
  }
  if (chunks) {
    ObsScope obs(KID_L21J_FINISH, s, (double)L * (a.plan.nchunk * sizeof(double) + sizeof(T)));
    hipLaunchKernelGGL((k_l21j_finish<T>), dim3(fit_grid(L, NB)), dim3(BLOCK), 0, s, (unsigned)L, a.plan.nchunk, part, g);
    SIPX_HIP(hipGetLastError());
  }
}
// v <- v scaled by the weights of g, for every set of the family: (ps, theta) the search's decision and the Float64 threshold, or
// EXT_L21_SEG's (theta, need) per frame; kid / bytes: the row of sipx_kernel_stats the launch is booked on
template <typename T>
static void l21_scale(hipStream_t s, const ExtSpec& sp, int kid, double bytes, T* v, const T* g, const ProjScalars<T>* ps, const T* theta,
                      const int* need) {
  constexpr int W = l21_vec_width<T>();
  const bool wide = l21_wide(sp, v, g);
  void (*const k)(L21Args, T*, const T*, const ProjScalars<T>*, const T*, const int*) =
      sp.kind == EXT_L21_SEG     ? (wide ? k_l21_scale<T, 2, W, true> : k_l21_scale<T, 2, 1, true>)
      : sp.kind == EXT_L21_JOINT ? (wide ? k_l21_scale<T, 2, W, false, true> : k_l21_scale<T, 2, 1, false, true>)
      : sp.nblk == 2             ? (wide ? k_l21_scale<T, 2, W, false> : k_l21_scale<T, 2, 1, false>)
                                 : (wide ? k_l21_scale<T, 3, W, false> : k_l21_scale<T, 3, 1, false>);
  ObsScope obs(kid, s, bytes);
  hipLaunchKernelGGL(k, dim3(fit_grid(sp.G.N / (wide ? W : 1), NB)), dim3(BLOCK), 0, s, l21_args(sp), v, g, ps, theta, need);
  SIPX_HIP(hipGetLastError());
}
template <typename T, bool OBSERVE>
static void l21_frames(hipStream_t s, const ExtSpec& sp, const T* g, T tau, const T* rmax, T* theta, int* need, T* asum, int* passes) {
  const long long L = sp.G.n[0] * sp.G.n[1], nf = sp.G.n[2];
  L21SegPlan plan = l21_seg_plan(L, nf, (int)sizeof(T));
  if (OBSERVE) { plan.lds = 0; plan.lds_bytes = 0; }
  ObsScope obs(KID_L21_FRAMES, s, (double)sp.G.N * sizeof(T));
  if (rmax)
    hipLaunchKernelGGL((k_l21_frames<T, true, OBSERVE>), dim3(plan.grid), dim3(BLOCK), plan.lds_bytes, s, plan, (unsigned)L, (unsigned)nf, g, tau,
                       rmax, theta, need, asum, passes);
  else
    hipLaunchKernelGGL((k_l21_frames<T, false, OBSERVE>), dim3(plan.grid), dim3(BLOCK), plan.lds_bytes, s, plan, (unsigned)L, (unsigned)nf, g, tau,
                       rmax, theta, need, asum, passes);
  SIPX_HIP(hipGetLastError());
}

// ---- EXT_L21_STACKED (l21_stacked.h): the spec -- nblk = B blocks of bstride = G rows on the 1-D grid of the M = B G rows -- and the launchers
static void l21s_check_spec(const ExtSpec& sp) {
  const long long G = l21s_check_shape(sp.G.N, sp.nblk);
  if (sp.bstride != G) throw std::runtime_error("the stacked l2,1 ball: the block stride must be the rows of one block");
  if (sp.mode != SIPX_MODE_WHOLE) throw std::runtime_error(L21S_WHOLE_ONLY);
  if (sp.weighted || sp.lb || sp.ub) throw std::runtime_error(L21S_NO_VECTORS);
}
// 16-byte accesses: G a multiple of the vector width (every block base q G then is 16-byte aligned) and 16-byte aligned arrays
template <typename T>
static bool l21s_wide(const ExtSpec& sp, const T* v, const T* g) {
  return sp.bstride % l21_vec_width<T>() == 0 && aligned16(v, g);
}
// the thread-iterations of one trip of the grid-stride loops: with VW groups each, G above L21S_TRIP * VW takes a second trip
constexpr long long L21S_TRIP = (long long)NB * BLOCK;
template <typename T>
static void l21s_norms(hipStream_t s, const ExtSpec& sp, const T* v, T* g) {
  constexpr int W = l21_vec_width<T>();
  const bool wide = l21s_wide(sp, v, g);
  const long long G = sp.bstride;
  void (*const k)(unsigned, int, const T*, T*) = sp.nblk == 3   ? (wide ? k_l21s_norms<T, 3, W> : k_l21s_norms<T, 3, 1>)
                                                 : sp.nblk == 6 ? (wide ? k_l21s_norms<T, 6, W> : k_l21s_norms<T, 6, 1>)
                                                                : (wide ? k_l21s_norms<T, 0, W> : k_l21s_norms<T, 0, 1>);
  ObsScope obs(KID_L21S_NORMS, s, (double)(sp.nblk + 1) * G * sizeof(T));
  hipLaunchKernelGGL(k, dim3(fit_grid(G / (wide ? W : 1), NB)), dim3(BLOCK), 0, s, (unsigned)G, sp.nblk, v, g);
  SIPX_HIP(hipGetLastError());
}
template <typename T>
static void l21s_scale(hipStream_t s, const ExtSpec& sp, T* v, const T* g, const ProjScalars<T>* ps, const T* theta) {
  constexpr int W = l21_vec_width<T>();
  const bool wide = l21s_wide(sp, v, g);
  const long long G = sp.bstride;
  void (*const k)(unsigned, int, T*, const T*, const ProjScalars<T>*, const T*) =
      sp.nblk == 3   ? (wide ? k_l21s_scale<T, 3, W> : k_l21s_scale<T, 3, 1>)
      : sp.nblk == 6 ? (wide ? k_l21s_scale<T, 6, W> : k_l21s_scale<T, 6, 1>)
                     : (wide ? k_l21s_scale<T, 0, W> : k_l21s_scale<T, 0, 1>);
  ObsScope obs(KID_L21S_SCALE, s, (double)(2 * sp.nblk + 1) * G * sizeof(T));
  hipLaunchKernelGGL(k, dim3(fit_grid(G / (wide ? W : 1), NB)), dim3(BLOCK), 0, s, (unsigned)G, sp.nblk, v, g, ps, theta);
  SIPX_HIP(hipGetLastError());
}

// ---- the weighted Michelot iteration on n entries (g, w) (l21_weighted.h): the device state and the launches, for BallProj's weighted
// route and for GroupsProj.  wide: 16-byte loads of g and w (n a multiple of 16 bytes' worth of entries, both arrays aligned).
// L1: the pass kernel is k_l1w_part, which takes g = |v| from v itself (l1_weighted.h, L1WProj); the finish, the batches, the flag are these.
template <typename T, bool L1 = false>
struct L21WSearch {
  L21WState* st = nullptr;             // the state of the iteration
  double* part = nullptr;              // the partials of a pass, 5 per workgroup
  T* theta = nullptr;                  // theta in T, written when the iteration is done
  int* flag = nullptr;                 // device: 0, or the passes once done
  int* h_flag = nullptr;               // pinned: where the host reads it
  long long last_passes = 0, last_reads = 0, calls = 0;
  L21WSearch() = default;
  L21WSearch(const L21WSearch&) = delete;
  ~L21WSearch() { if (h_flag) (void)hipHostFree(h_flag); }
  void build(ExtImpl<T>& owner) {
    st = owner.template alloc<L21WState>(1);
    part = owner.template alloc<double>(5 * L21W_GRID);
    theta = owner.template alloc<T>(1);
    flag = owner.template alloc<int>(1);
    SIPX_HIP(hipHostMalloc((void**)&h_flag, sizeof(int), hipHostMallocDefault));
  }
  // one pass: the partial kernel and the one-workgroup finish (both return at once when the state says done)
  template <bool FIRST>
  void pass(hipStream_t stream, long long n, const T* g, const T* w, bool wide, T tau) {
    constexpr int W = l21_vec_width<T>();
    const int grid = fit_grid((n / (wide ? W : 1) + L21W_LOADS - 1) / L21W_LOADS, L21W_GRID);
    void (*const k)(unsigned, const T*, const T*, const L21WState*, double*) =
        L1 ? (wide ? k_l1w_part<T, W, FIRST> : k_l1w_part<T, 1, FIRST>) : (wide ? k_l21w_part<T, W, FIRST> : k_l21w_part<T, 1, FIRST>);
    {
      ObsScope obs(L1 ? KID_L1W_PASS : KID_L21W_PASS, stream, 2.0 * n * sizeof(T));
      hipLaunchKernelGGL(k, dim3(grid), dim3(BLOCK), 0, stream, (unsigned)n, g, w, st, part);
    }
    hipLaunchKernelGGL((k_l21w_finish<T, FIRST>), dim3(1), dim3(BLOCK), 0, stream, grid, tau, part, st, theta, flag);
    SIPX_HIP(hipGetLastError());
  }
  // the iteration: passes in batches of L21W_BATCH, one 4-byte read of the flag per batch; more than n + 1 passes is an error
  void run(hipStream_t stream, long long n, const T* g, const T* w, bool wide, T tau) {
    pass<true>(stream, n, g, w, wide, tau);
    long long queued = 1;
    last_reads = 0;
    for (;;) {
      for (; queued % L21W_BATCH != 0; ++queued) pass<false>(stream, n, g, w, wide, tau);
      SIPX_HIP(hipMemcpyAsync(h_flag, flag, sizeof(int), hipMemcpyDeviceToHost, stream));
      SIPX_HIP(hipStreamSynchronize(stream));
      ++last_reads;
      if (*h_flag) break;
      if (queued > n + 1)
        throw std::runtime_error(L1 ? "the weighted l1 ball: the threshold iteration did not end within n + 1 passes"
                                    : "the weighted l2,1 ball: the threshold iteration did not end within n + 1 passes");
      pass<false>(stream, n, g, w, wide, tau);
      ++queued;
    }
    last_passes = *h_flag;
    ++calls;
  }
  // out[0] <- (T)asum of the last first pass
  void pick(hipStream_t stream, T* out) {
    hipLaunchKernelGGL((k_l21w_pick<T>), dim3(1), dim3(64), 0, stream, st, out);
    SIPX_HIP(hipGetLastError());
  }
};

// ---- EXT_L21, EXT_L21_JOINT, EXT_L21_STACKED: one ball on the whole array -- the norms, the engine's search on g, Float64: the refinement, the scale ----
// The sets differ in what a group is, hence in the norms and scale launches and in the length of g: the N grid points, the L pixels, or the
// G rows of one block of a stacked operator.
template <typename T>
struct BallProj : ExtImpl<T> {
  using ExtImpl<T>::sp;
  using ExtImpl<T>::stream;
  const bool joint, stacked;
  long long n = 0;                     // groups: the entries of g, the length of the search
  T* g = nullptr;                      // the group norms
  double* part = nullptr;              // EXT_L21_JOINT: the chunk sums, nchunk L entries, when the plan chunks
  double* tpart = nullptr;             // Float64: the partial sums of k_l21_theta_part
  T* theta = nullptr;                  // Float64: the threshold k_l21_scale applies
  SearchState<T> search;
  ProjScalars<T>* ps_obs = nullptr;    // the state of observe's search, taken at its first call
  // the weighted route (l21_weighted.h), taken when the spec carries weights: none of the members above but g and part is used
  T* w = nullptr;                      // one weight per group
  L21WSearch<T> ws;                    // the iteration on (g, w)
  void reset() override { search.reinit(stream); }
  BallProj(const ExtSpec& spec, hipStream_t s) : ExtImpl<T>(spec, s), joint(spec.kind == EXT_L21_JOINT), stacked(spec.kind == EXT_L21_STACKED) {
    if (stacked) l21s_check_spec(sp);
    else if (joint) l21_joint_check_spec(sp);
    else l21_check_spec(sp);
    if (!(sp.pmax > 0)) throw std::runtime_error("Radius of L1 ball is negative");
    n = stacked ? sp.bstride : (joint ? sp.G.st[2] : sp.G.N);
    g = this->template alloc<T>(n);
    const int nchunk = joint ? l21_joint_plan(n, sp.G.n[2], (int)sizeof(T)).nchunk : 1;
    if (nchunk > 1) part = this->template alloc<double>((size_t)nchunk * n);
    if (sp.weighted) {
      w = this->template alloc<T>(n);
      ws.build(*this);
      if (sp.lb) SIPX_HIP(hipMemcpy(w, sp.lb, sizeof(T) * (size_t)n, hipMemcpyHostToDevice));
      else SIPX_HIP(hipMemsetAsync(w, 0, sizeof(T) * (size_t)n, s));      // (set_data brings them; until then no group is constrained)
      return;
    }
    if (sizeof(T) == 8) {
      tpart = this->template alloc<double>(3 * L21_THETA_GRID);
      theta = this->template alloc<T>(1);
    }
    search.build(this->mem, s, 0);
  }
  // g <- the group norms of v
  void norms(const T* v) {
    if (stacked) l21s_norms<T>(stream, sp, v, g);
    else l21_norms<T>(stream, sp, v, g, part);
  }
  // the search on g; Float64: then the threshold of its active set in twice the working precision, left in theta[0]
  void threshold(ProjScalars<T>* ps, double* partials, T* maxpart, T* compact) {
    K<T>::proj_scalars_arr(stream, n, g, PX_L1, T(0), (T)sp.pmax, ps, partials, maxpart, compact, n);
    if constexpr (sizeof(T) == 8) {
      const int grid = fit_grid(n, L21_THETA_GRID);
      hipLaunchKernelGGL(k_l21_theta_part, dim3(grid), dim3(BLOCK), 0, stream, (unsigned)n, g, ps, tpart);
      hipLaunchKernelGGL(k_l21_theta_final, dim3(1), dim3(BLOCK), 0, stream, grid, (unsigned)n, (double)sp.pmax, tpart, ps, theta);
      SIPX_HIP(hipGetLastError());
    }
  }
  // ---- the weighted route ----
  bool weighted_wide() const { return sp.G.n[0] % 4 == 0 && aligned16(g, w); }
  void weighted_scale(T* v) {
    constexpr int W = l21_vec_width<T>();
    const bool wide = l21_wide(sp, v, g) && aligned16(w);
    void (*const k)(L21Args, T*, const T*, const T*, const L21WState*, const T*) =
        joint           ? (wide ? k_l21w_scale<T, 2, W, true> : k_l21w_scale<T, 2, 1, true>)
        : sp.nblk == 2  ? (wide ? k_l21w_scale<T, 2, W, false> : k_l21w_scale<T, 2, 1, false>)
                        : (wide ? k_l21w_scale<T, 3, W, false> : k_l21w_scale<T, 3, 1, false>);
    ObsScope obs(KID_L21W_SCALE, stream, (2.0 * sp.nblk * sp.G.N + 2.0 * n) * sizeof(T));
    hipLaunchKernelGGL(k, dim3(fit_grid(sp.G.N / (wide ? W : 1), NB)), dim3(BLOCK), 0, stream, l21_args(sp), v, g, w, ws.st, ws.theta);
    SIPX_HIP(hipGetLastError());
  }
  void set_data(const T* new_lb, const T* new_ub, bool on_device) override {
    if (!w) ExtImpl<T>::set_data(new_lb, new_ub, on_device);
    if (new_ub) throw std::runtime_error("the weighted l2,1 ball: the weights are its lb, it has no ub (the radius is fixed at sipx_add_set)");
    if (new_lb) SIPX_HIP(hipMemcpyAsync(w, new_lb, sizeof(T) * (size_t)n, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
  }
  // the passes of the last call (the first included), the reads of the flag it took, the calls so far, the groups
  void route_counts(long long out[4]) const override {
    out[0] = ws.last_passes; out[1] = ws.last_reads; out[2] = ws.calls; out[3] = w ? n : 0;
  }

  void project(T* v, bool feas, double* partials, T* maxpart, T* compact) override {
    const double N = (double)sp.G.N;
    if (w) {
      l21_norms<T>(stream, sp, v, g, part);
      ws.run(stream, n, g, w, weighted_wide(), (T)sp.pmax);
      weighted_scale(v);
      return;
    }
    ProjScalars<T>* ps = search.pick(feas);
    norms(v);
    threshold(ps, partials, maxpart, compact);
    if (stacked) l21s_scale<T>(stream, sp, v, g, ps, theta);
    else if (joint) l21_scale<T>(stream, sp, KID_L21J_SCALE, (4 * N + n) * sizeof(T), v, g, ps, theta, nullptr);
    else l21_scale<T>(stream, sp, KID_L21_SCALE, (2 * sp.nblk + 1) * N * sizeof(T), v, g, ps, theta, nullptr);
  }
  // out[0] <- the sum of the group norms as project decides on it: its norms launch into its g, then the first pass of a search with
  // a new state and an infinite radius -- the sum, and the rounding to T, that project compares with the radius.  The warm starts stay.
  void observe(const T* v, T* out, double* partials, T* maxpart, T* compact) override {
    if (w) {                // the weighted norm: the norms launch and the first pass of project(), (T)asum as that pass compares it
      l21_norms<T>(stream, sp, v, g, part);
      ws.template pass<true>(stream, n, g, w, weighted_wide(), (T)INFINITY);
      ws.pick(stream, out);
      return;
    }
    if (!ps_obs) ps_obs = this->template alloc<ProjScalars<T>>(1);
    norms(v);
    K<T>::ps_init(stream, ps_obs, nullptr);
    K<T>::proj_scalars_arr(stream, n, g, PX_L1, T(0), (T)INFINITY, ps_obs, partials, maxpart, compact, n);
    hipLaunchKernelGGL((k_l21_pick<T>), dim3(1), dim3(64), 0, stream, ps_obs, out);
    SIPX_HIP(hipGetLastError());
  }
};

// ---- EXT_L21_SEG: the l2,1 ball of every z-slice on the range of TV_xy (l21_seg.h) -------------------------------------------------------
//     k_l21_norms     as above, two blocks on the 3-D grid                                    reads 2 N words, writes N
//     k_l21_frames    one workgroup per frame on g alone: asum, the decision, Michelot's passes  reads N (LDS) or passes * N
//     k_l21_scale     the per-frame form; frames inside their ball are skipped without a store  reads up to 3 N, writes up to 2 N
// Nothing is kept between calls: the call of the feasibility estimate and the one of the y update are independent, reset() has
// nothing to forget.  Built with ExtSpec::ub every frame has its own radius (rmax, n3 entries), sipx_set_data replaces them.
template <typename T>
struct FrameProj : ExtImpl<T> {
  using ExtImpl<T>::sp;
  using ExtImpl<T>::stream;
  T *g = nullptr, *theta = nullptr, *asum = nullptr, *rmax = nullptr;
  int *need = nullptr, *passes = nullptr;
  long long nf = 0;
  FrameProj(const ExtSpec& spec, hipStream_t s) : ExtImpl<T>(spec, s) {
    l21_seg_check_spec(sp);
    nf = sp.G.n[2];
    if (!sp.ub && !((T)sp.pmax > T(0))) throw std::runtime_error("Radius of L1 ball is negative");
    if (sp.ub) {
      const T* h = (const T*)sp.ub;
      for (long long k = 0; k < nf; ++k)
        if (!(h[k] > T(0))) throw std::runtime_error("Radius of L1 ball is negative");
    }
    g = this->template alloc<T>(sp.G.N);
    theta = this->template alloc<T>(nf);
    asum = this->template alloc<T>(nf);
    need = this->template alloc<int>(2 * nf);
    passes = need + nf;
    SIPX_HIP(hipMemset(need, 0, sizeof(int) * 2 * (size_t)nf));      // (route_counts may be asked before the first projection)
    if (sp.ub) {
      rmax = this->template alloc<T>(nf);
      SIPX_HIP(hipMemcpy(rmax, sp.ub, sizeof(T) * (size_t)nf, hipMemcpyHostToDevice));
    }
  }
  void project(T* v, bool, double*, T*, T*) override {
    l21_norms<T>(stream, sp, v, g);
    l21_frames<T, false>(stream, sp, g, (T)sp.pmax, rmax, theta, need, asum, passes);
    l21_scale<T>(stream, sp, KID_L21_SCALE, (2 * sp.nblk + 1) * (double)sp.G.N * sizeof(T), v, g, nullptr, theta, need);
  }
  // out[k] (n3 entries) <- (T)asum_k of the frames as project decides on them: its norms launch into its g, then pass 1 of k_l21_frames
  void observe(const T* v, T* out, double*, T*, T*) override {
    l21_norms<T>(stream, sp, v, g);
    l21_frames<T, true>(stream, sp, g, T(0), (const T*)nullptr, (T*)nullptr, (int*)nullptr, out, (int*)nullptr);
  }
  void set_data(const T* new_lb, const T* new_ub, bool on_device) override {
    if (!rmax) ExtImpl<T>::set_data(new_lb, new_ub, on_device);
    if (new_lb) throw std::runtime_error("only the annulus has inner radii: pass the radii of this set as ub");
    if (new_ub)
      SIPX_HIP(hipMemcpyAsync(rmax, new_ub, sizeof(T) * (size_t)nf, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
  }
  // the Michelot passes of the last call, per frame (tools/l21_frames_bench.py)
  void route_counts(long long out[4]) const override {
    std::vector<int> h((size_t)nf);
    SIPX_HIP(hipStreamSynchronize(stream));
    SIPX_HIP(hipMemcpy(h.data(), passes, sizeof(int) * h.size(), hipMemcpyDeviceToHost));
    out[0] = out[1] = out[2] = 0; out[3] = nf;
    for (int x : h) { out[0] += x; out[1] = std::max<long long>(out[1], x); }
  }
};

// ---- EXT_TNV: the nuclear-norm ball on the pixels' Jacobians (tnv.h) -- the Gram march, the engine's search on the 2 L singular values,
// Float64: the refinement, the 2 x 2 matrices.  BallProj's sequence with s in place of g; the search runs on 2 L entries, which the scratch
// every caller hands over (N entries at least) holds: a 3-D grid has n3 >= 2 frames, so 2 L <= N -- checked when the projector is built.
template <typename T>
struct TnvProj : ExtImpl<T> {
  using ExtImpl<T>::sp;
  using ExtImpl<T>::stream;
  L21JointPlan plan{};
  long long L = 0;                     // pixels
  T* s = nullptr;                      // [sigma1; sigma2], 2 L entries: the array of the search
  T* rot = nullptr;                    // [cs; sn], 2 L entries
  double* part = nullptr;              // the chunk sums, nchunk tnv_words L entries, when the plan chunks
  double* tpart = nullptr;             // Float64: the partial sums of k_l21_theta_part
  T* theta = nullptr;                  // Float64: the threshold k_tnv_apply applies
  SearchState<T> search;
  ProjScalars<T>* ps_obs = nullptr;    // the state of observe's search, taken at its first call
  void reset() override { search.reinit(stream); }
  TnvProj(const ExtSpec& spec, hipStream_t st) : ExtImpl<T>(spec, st) {
    tnv_check_spec(sp);
    if (!(sp.pmax > 0)) throw std::runtime_error("Radius of L1 ball is negative");
    L = sp.G.st[2];
    if (2 * L > sp.G.N) throw std::runtime_error("total nuclear variation: the search over 2 n1 n2 singular values needs a grid of at least 2 frames");
    plan = l21_joint_plan(L, sp.G.n[2], (int)sizeof(T));
    s = this->template alloc<T>(2 * L);
    rot = this->template alloc<T>(2 * L);
    if (plan.nchunk > 1) part = this->template alloc<double>((size_t)plan.nchunk * tnv_words<T>() * L);
    if (sizeof(T) == 8) {
      tpart = this->template alloc<double>(3 * L21_THETA_GRID);
      theta = this->template alloc<T>(1);
    }
    search.build(this->mem, st, 0);
  }
  // (s, rot) <- the singular values and rotations of the pixels of v
  void gram(const T* v) {
    constexpr int W = l21_vec_width<T>();
    const bool wide = l21_wide(sp, v, s) && aligned16(rot), chunks = plan.nchunk > 1;
    L21JArgs a;
    a.G = sp.G;
    a.G.set_fast_div();
    a.bstride = sp.bstride;
    a.plan = plan;
    {
      void (*const k)(L21JArgs, const T*, T*, T*, double*) = chunks ? (wide ? k_tnv_gram<T, W, true> : k_tnv_gram<T, 1, true>)
                                                                    : (wide ? k_tnv_gram<T, W, false> : k_tnv_gram<T, 1, false>);
      ObsScope obs(KID_TNV_GRAM, stream, (double)(2 * sp.G.N + 4 * L) * sizeof(T));
      hipLaunchKernelGGL(k, dim3(fit_grid(L / (wide ? W : 1) * plan.nchunk, NB)), dim3(BLOCK), 0, stream, a, v, s, rot, part);
      SIPX_HIP(hipGetLastError());
    }
    if (chunks) {
      ObsScope obs(KID_TNV_FINISH, stream, (double)L * (plan.nchunk * tnv_words<T>() * sizeof(double) + 4 * sizeof(T)));
      hipLaunchKernelGGL((k_tnv_finish<T>), dim3(fit_grid(L, NB)), dim3(BLOCK), 0, stream, (unsigned)L, plan.nchunk, part, s, rot);
      SIPX_HIP(hipGetLastError());
    }
  }
  void project(T* v, bool feas, double* partials, T* maxpart, T* compact) override {
    constexpr int W = l21_vec_width<T>();
    ProjScalars<T>* ps = search.pick(feas);
    gram(v);
    K<T>::proj_scalars_arr(stream, 2 * L, s, PX_L1, T(0), (T)sp.pmax, ps, partials, maxpart, compact, 2 * L);
    if constexpr (sizeof(T) == 8) {
      const int grid = fit_grid(2 * L, L21_THETA_GRID);
      hipLaunchKernelGGL(k_l21_theta_part, dim3(grid), dim3(BLOCK), 0, stream, (unsigned)(2 * L), s, ps, tpart);
      hipLaunchKernelGGL(k_l21_theta_final, dim3(1), dim3(BLOCK), 0, stream, grid, (unsigned)(2 * L), (double)sp.pmax, tpart, ps, theta);
      SIPX_HIP(hipGetLastError());
    }
    const bool wide = l21_wide(sp, v, s) && aligned16(rot);
    ObsScope obs(KID_TNV_APPLY, stream, (double)(4 * sp.G.N + 4 * L) * sizeof(T));
    hipLaunchKernelGGL((wide ? k_tnv_apply<T, W> : k_tnv_apply<T, 1>), dim3(fit_grid(sp.G.N / (wide ? W : 1), NB)), dim3(BLOCK), 0, stream,
                       l21_args(sp), v, s, rot, ps, theta);
    SIPX_HIP(hipGetLastError());
  }
  // out[0] <- ||s||_1 as project compares it: its Gram launch into its s, then the first pass of a search with a new state and an
  // infinite radius -- the sum, and the rounding to T, of project's decision.  The warm starts stay.
  void observe(const T* v, T* out, double* partials, T* maxpart, T* compact) override {
    if (!ps_obs) ps_obs = this->template alloc<ProjScalars<T>>(1);
    gram(v);
    K<T>::ps_init(stream, ps_obs, nullptr);
    K<T>::proj_scalars_arr(stream, 2 * L, s, PX_L1, T(0), (T)INFINITY, ps_obs, partials, maxpart, compact, 2 * L);
    hipLaunchKernelGGL((k_l21_pick<T>), dim3(1), dim3(64), 0, stream, ps_obs, out);
    SIPX_HIP(hipGetLastError());
  }
};

// ---- EXT_L21_GROUPS: one ball whose groups are the fibers or slices of the valid block (l21_groups.h) ---------------------------------------
// The norms by the plan of l21_groups.h, the iteration of the weighted route on the nseg pairs (g, w), k_l21g_scale.  Built without weights
// w is a vector of ones: not one launch, and not one bit, differs from the set built with np.ones(nseg).  Nothing is kept between calls.
static void l21g_check_spec(const ExtSpec& sp) {
  if (sp.nblk > 1) throw std::runtime_error(L21G_ONE_BLOCK);
  if (sp.mode != SIPX_MODE_FIBER && sp.mode != SIPX_MODE_SLICE) throw std::runtime_error(L21G_NEEDS_MODE);
  if (sp.ndim == 2 && sp.mode == SIPX_MODE_SLICE) throw std::runtime_error(L21G_2D_SLICE);
  if (sp.G.N >= (1ll << 31)) throw std::runtime_error("the l2,1 ball over fibers or slices: the grid needs fewer than 2^31 points");
}
// The norms launch of the sets whose groups are the fibers or slices of the valid block, with its plan, its g and its chunk partials:
// GroupsProj and CardGroupsProj hold one each.  g[s], s < n, in the order of sipx_segment_norms (l21_groups.h RULE, PLAN).
template <typename T>
struct GroupNorms {
  SegMap map{};
  L21GroupsPlan plan{};
  long long n = 0;                     // segments: the entries of g
  T* g = nullptr;
  double* part = nullptr;              // slices: the chunk partials, 2 per (slice, chunk)
  void build(ExtImpl<T>& owner, const char* empty) {
    map = make_segmap(owner.sp);
    if (map.nseg < 1 || map.L < 1) throw std::runtime_error(empty);
    plan = l21_groups_plan(map, owner.sp.mode, (int)sizeof(T));
    n = map.nseg;
    g = owner.template alloc<T>(n);
    if (plan.slices) part = owner.template alloc<double>(2 * (size_t)(plan.ntA * plan.F * plan.nchunk));
  }
  void run(hipStream_t stream, const ExtSpec& sp, const T* v) const {
    if (!plan.slices) {                // k_seg_observe with the tile mapping of seg_norm.h: the bits of sipx_segment_norms
      ObsScope obs(KID_L21G_NORMS, stream, (double)(map.nseg * map.L + n) * sizeof(T));
      hipLaunchKernelGGL((k_seg_observe<T, SEGN_L2>), dim3(plan.fiber.grid), dim3(BLOCK), 0, stream, map, plan.fiber, v, g);
      SIPX_HIP(hipGetLastError());
      return;
    }
    constexpr int W = l21_vec_width<T>();
    // 16-byte loads: a thread's VW entries lie in one row of the slice (LA % VW) whose start is 16-byte aligned (every stride % VW)
    const bool wide = plan.vw == W && map.LA % W == 0 && sp.G.n[0] % 4 == 0 && aligned16(v);
    void (*const k)(SegMap, L21GroupsPlan, const T*, double*) =
        plan.vw == 1 ? k_l21g_part<T, 1, false> : (wide ? k_l21g_part<T, W, true> : k_l21g_part<T, W, false>);
    {
      ObsScope obs(KID_L21G_NORMS, stream, (double)(map.nseg * map.L) * sizeof(T) + 16.0 * plan.grid);
      hipLaunchKernelGGL(k, dim3((unsigned)plan.grid), dim3(BLOCK), 0, stream, map, plan, v, part);
    }
    {
      ObsScope obs(KID_L21G_FINISH, stream, (double)n * (16.0 * plan.nchunk + sizeof(T)));
      hipLaunchKernelGGL((k_l21g_finish<T>), dim3(fit_grid(n, NB)), dim3(BLOCK), 0, stream, n, plan.nchunk, part, g);
    }
    SIPX_HIP(hipGetLastError());
  }
};
// grid point -> segment for k_l21g_scale and k_cardg_zero
static L21GArgs l21g_args(const ExtSpec& sp) {
  L21GArgs a;
  a.G = sp.G;
  a.G.set_fast_div();
  for (int q = 0; q < 3; ++q) { a.d[q] = (int)sp.dims[q]; a.cs[q] = 0; }
  if (sp.mode == SIPX_MODE_SLICE) {
    a.cs[sp.dir] = 1;
  } else {                             // make_segmap: s = c_a + d_a c_b over the two other axes a < b
    const int ax = sp.dir == 0 ? 1 : 0, bx = sp.dir == 2 ? 1 : 2;
    a.cs[ax] = 1;
    a.cs[bx] = (int)sp.dims[ax];
  }
  return a;
}

template <typename T>
struct GroupsProj : ExtImpl<T> {
  using ExtImpl<T>::sp;
  using ExtImpl<T>::stream;
  GroupNorms<T> nm;
  long long n = 0;                     // segments: the entries of g and w, the length of the search
  T* w = nullptr;
  L21WSearch<T> ws;
  GroupsProj(const ExtSpec& spec, hipStream_t s) : ExtImpl<T>(spec, s) {
    l21g_check_spec(sp);
    if (!(sp.pmax > 0)) throw std::runtime_error("Radius of L1 ball is negative");
    nm.build(*this, "the l2,1 ball over fibers or slices: empty segments");
    n = nm.n;
    w = this->template alloc<T>(n);
    ws.build(*this);
    if (sp.lb) {
      SIPX_HIP(hipMemcpy(w, sp.lb, sizeof(T) * (size_t)n, hipMemcpyHostToDevice));
    } else if (sp.weighted) {
      SIPX_HIP(hipMemsetAsync(w, 0, sizeof(T) * (size_t)n, s));      // (set_data brings them; until then no segment is constrained)
    } else {
      const std::vector<T> ones((size_t)n, T(1));
      SIPX_HIP(hipMemcpy(w, ones.data(), sizeof(T) * (size_t)n, hipMemcpyHostToDevice));
    }
  }
  bool search_wide() const { return n % 4 == 0 && aligned16(nm.g, w); }
  void scale(T* v) {
    constexpr int W = l21_vec_width<T>();
    const bool wide = sp.G.n[0] % 4 == 0 && aligned16(v);
    ObsScope obs(KID_L21G_SCALE, stream, (2.0 * sp.G.N + 2.0 * n) * sizeof(T));
    hipLaunchKernelGGL((wide ? k_l21g_scale<T, W> : k_l21g_scale<T, 1>), dim3(fit_grid(sp.G.N / (wide ? W : 1), NB)), dim3(BLOCK), 0, stream,
                       l21g_args(sp), v, nm.g, w, ws.st, ws.theta);
    SIPX_HIP(hipGetLastError());
  }
  void project(T* v, bool, double*, T*, T*) override {
    nm.run(stream, sp, v);
    ws.run(stream, n, nm.g, w, search_wide(), (T)sp.pmax);
    scale(v);
  }
  // out[0] <- (T)asum as project decides on it: its norms launch into its g, then the first pass of its iteration
  void observe(const T* v, T* out, double*, T*, T*) override {
    nm.run(stream, sp, v);
    ws.template pass<true>(stream, n, nm.g, w, search_wide(), (T)INFINITY);
    ws.pick(stream, out);
  }
  void set_data(const T* new_lb, const T* new_ub, bool on_device) override {
    if (!sp.weighted) ExtImpl<T>::set_data(new_lb, new_ub, on_device);
    if (new_ub) throw std::runtime_error("the weighted l2,1 ball: the weights are its lb, it has no ub (the radius is fixed at sipx_add_set)");
    if (new_lb) SIPX_HIP(hipMemcpyAsync(w, new_lb, sizeof(T) * (size_t)n, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
  }
  // the passes of the last call (the first included), the reads of the flag it took, the calls so far, the segments
  void route_counts(long long out[4]) const override {
    out[0] = ws.last_passes; out[1] = ws.last_reads; out[2] = ws.calls; out[3] = n;
  }
};

// ---- EXT_CARD_GROUPS: at most k non-zero fibers or slices of the valid block (card_groups.h) ------------------------------------------------
// The norms launch of GroupsProj into a g of its own, the selection by one of two routes into the need / tau / quota of a ProjScalars,
// k_cardg_zero.  The route is fixed when the projector is built: the small route where nseg <= CARDG_SMALL_MAX, unless
// sipx_card_groups_route (a hook of the tests and of tools/card_groups_bench.py) forces one.  The search keeps one state for the y update
// and one for the feasibility estimate; they warm-start its probes and do not change what it selects.  k >= nseg launches nothing.
// (an atomic word: a test thread may set it while another builds a context; a projector reads it once, in its constructor)
static std::atomic<int> g_cardg_route{0};      // 0: by nseg; 1: the small route (refused above its cap); 2: the search route
void card_groups_force_route(int route) {
  if (route < 0 || route > 2) throw std::runtime_error("sipx_card_groups_route: 0 (by the number of segments), 1 (small route) or 2 (search route)");
  g_cardg_route.store(route, std::memory_order_relaxed);
}
static void cardg_check_spec(const ExtSpec& sp) {
  if (sp.nblk > 1) throw std::runtime_error(CARDG_ONE_BLOCK);
  if (sp.mode != SIPX_MODE_FIBER && sp.mode != SIPX_MODE_SLICE) throw std::runtime_error(CARDG_NEEDS_MODE);
  if (sp.ndim == 2 && sp.mode == SIPX_MODE_SLICE) throw std::runtime_error(CARDG_2D_SLICE);
  if (sp.lb || sp.ub) throw std::runtime_error(CARDG_NO_VECTORS);
  if (sp.G.N >= (1ll << 31)) throw std::runtime_error(CARDG_TOO_LARGE);
}
// The selection of the k-th place of the stable descending order of n keys g, for the projectors that keep the k largest groups
// (CardGroupsProj, L20Proj): the route, fixed when the projector is built, the search's states, the two launches.  The result is the
// need / tau / quota of the ProjScalars run() returns (card_groups.h RULE, SELECTION).
template <typename T>
struct CardgSelect {
  long long n = 0, k = 0;              // keys; places, k < n wherever run() is called
  bool small = false;
  SearchState<T> search;               // search route: both states; small route: ps alone holds the result
  void build(DeviceMemory& mem, hipStream_t s, long long n_, long long k_) {
    n = n_;
    k = k_;
    const int route = g_cardg_route.load(std::memory_order_relaxed);
    if (route == 1 && n > CARDG_SMALL_MAX)
      throw std::runtime_error("sipx_card_groups_route: the small route holds at most " + std::to_string(CARDG_SMALL_MAX) + " segments, this set has " +
                               std::to_string(n));
    small = route == 1 || (route == 0 && n <= CARDG_SMALL_MAX);
    search.build(mem, s, small ? 0 : n);      // cidx: the tie cut of the search
  }
  void reinit(hipStream_t s) { search.reinit(s); }
  ProjScalars<T>* run(hipStream_t stream, const T* g, bool feas, double* partials, T* maxpart, T* compact) {
    ProjScalars<T>* ps = small ? search.ps : search.pick(feas);
    if (small) {
      ObsScope obs(KID_CARDG_RANK, stream, (double)n * sizeof(T));
      hipLaunchKernelGGL((k_cardg_rank<T>), dim3(1), dim3(CARDG_SMALL_MAX), 0, stream, (int)n, (int)k, g, ps);
    } else {
      K<T>::proj_scalars_arr(stream, n, g, PX_CARD, T(0), (T)k, ps, partials, maxpart, compact, n);
    }
    return ps;
  }
};
template <typename T>
struct CardGroupsProj : ExtImpl<T> {
  using ExtImpl<T>::sp;
  using ExtImpl<T>::stream;
  GroupNorms<T> nm;
  long long n = 0, k = 0;              // segments; segments kept, clamped to n
  CardgSelect<T> sel;
  long long calls = 0, selections = 0;      // projections since the reset; those that ran a selection (k < nseg)
  CardGroupsProj(const ExtSpec& spec, hipStream_t s) : ExtImpl<T>(spec, s) {
    cardg_check_spec(sp);
    nm.build(*this, "group cardinality (card_groups): empty segments");
    n = nm.n;
    cardg_check_k<T>(sp.pmax, n);
    k = sp.pmax >= (double)n ? n : (long long)sp.pmax;
    sel.build(this->mem, s, n, k);
  }
  void reset() override { sel.reinit(stream); calls = selections = 0; }
  void project(T* v, bool feas, double* partials, T* maxpart, T* compact) override {
    ++calls;
    if (k >= n) return;                // every segment stays: nothing to select, nothing to write
    ++selections;
    nm.run(stream, sp, v);
    ProjScalars<T>* ps = sel.run(stream, nm.g, feas, partials, maxpart, compact);
    constexpr int W = l21_vec_width<T>();
    const bool wide = sp.G.n[0] % 4 == 0 && aligned16(v);
    ObsScope obs(KID_CARDG_ZERO, stream, (double)sp.G.N * sizeof(T), ((double)nm.map.nseg * nm.map.L + n) * sizeof(T));
    hipLaunchKernelGGL((wide ? k_cardg_zero<T, W> : k_cardg_zero<T, 1>), dim3(fit_grid(sp.G.N / (wide ? W : 1), NB)), dim3(BLOCK), 0, stream,
                       l21g_args(sp), v, nm.g, ps);
    SIPX_HIP(hipGetLastError());
  }
  // out[s] <- g_s (nseg entries): the norms launch of project() into its own g, copied out; v is not written
  void observe(const T* v, T* out, double*, T*, T*) override {
    nm.run(stream, sp, v);
    SIPX_HIP(hipMemcpyAsync(out, nm.g, sizeof(T) * (size_t)n, hipMemcpyDeviceToDevice, stream));
  }
  void set_data(const T*, const T*, bool) override { throw std::runtime_error(CARDG_NO_SET_DATA); }
  // projections since the reset, the selections the small route ran, those the search route ran (a projection with k >= nseg runs
  // none), the segments
  void route_counts(long long out[4]) const override {
    out[0] = calls; out[1] = sel.small ? selections : 0; out[2] = sel.small ? 0 : selections; out[3] = n;
  }
};

// ---- EXT_L20, EXT_L20_JOINT: at most k grid points (pixels) with a non-zero gradient vector (l20.h) ------------------------------------------
// BallProj's norms launch into a g of its own -- N entries, or the L pixels of the joint set with its chunk plan --, CardGroupsProj's
// selection (CardgSelect: sipx_card_groups_route forces the route of both), k_l20_zero.  k >= the number of groups launches nothing.
static void l20_check_spec(const ExtSpec& sp, bool frames) {
  if (sp.G.N >= (1ll << 31)) throw std::runtime_error(L20_TOO_LARGE);
  if (sp.nblk < 2) throw std::runtime_error(L20_NEEDS_TV);
  l21_check_spec(sp);
  if (sp.lb || sp.weighted) throw std::runtime_error(L20_NO_WEIGHTS);
  if (frames) {
    if (sp.ndim != 3 || sp.nblk != 2 || sp.bdir[0] != 1 || sp.bdir[1] != 0 || sp.mode != SIPX_MODE_SLICE || sp.dir != 2)
      throw std::runtime_error(L20_MODES);
    return;
  }
  if (sp.mode != SIPX_MODE_WHOLE) throw std::runtime_error(L20_MODES);
  if (sp.ub) throw std::runtime_error(L20_K_VECTOR);
  if (sp.kind == EXT_L20_JOINT && (sp.ndim != 3 || sp.nblk != 2 || sp.bdir[0] != 1 || sp.bdir[1] != 0)) throw std::runtime_error(L20_JOINT_ROUTE);
}
// v <- the members of the dropped groups set to +0, for the three sets: (ps) the one selection, or (need, tau, cut) per frame
template <typename T>
static void l20_zero(hipStream_t s, const ExtSpec& sp, T* v, const T* g, long long ngroups, const ProjScalars<T>* ps, const int* need,
                     const T* tau, const int* cut) {
  constexpr int W = l21_vec_width<T>();
  const bool wide = l21_wide(sp, v, g);
  void (*const k)(L21Args, T*, const T*, const ProjScalars<T>*, const int*, const T*, const int*) =
      sp.kind == EXT_L20_SEG     ? (wide ? k_l20_zero<T, 2, W, true, false> : k_l20_zero<T, 2, 1, true, false>)
      : sp.kind == EXT_L20_JOINT ? (wide ? k_l20_zero<T, 2, W, false, true> : k_l20_zero<T, 2, 1, false, true>)
      : sp.nblk == 2             ? (wide ? k_l20_zero<T, 2, W, false, false> : k_l20_zero<T, 2, 1, false, false>)
                                 : (wide ? k_l20_zero<T, 3, W, false, false> : k_l20_zero<T, 3, 1, false, false>);
  ObsScope obs(KID_L20_ZERO, s, (double)ngroups * sizeof(T), (double)sp.nblk * sp.G.N * sizeof(T));
  hipLaunchKernelGGL(k, dim3(fit_grid(sp.G.N / (wide ? W : 1), NB)), dim3(BLOCK), 0, s, l21_args(sp), v, g, ps, need, tau, cut);
  SIPX_HIP(hipGetLastError());
}
template <typename T>
struct L20Proj : ExtImpl<T> {
  using ExtImpl<T>::sp;
  using ExtImpl<T>::stream;
  const bool joint;
  long long n = 0, k = 0;              // groups: the entries of g; groups kept, clamped to n
  T* g = nullptr;                      // the keys
  double* part = nullptr;              // EXT_L20_JOINT: the chunk sums, nchunk L entries, when the plan chunks
  CardgSelect<T> sel;
  long long calls = 0, selections = 0;      // projections since the reset; those that ran a selection (k < n)
  L20Proj(const ExtSpec& spec, hipStream_t s) : ExtImpl<T>(spec, s), joint(spec.kind == EXT_L20_JOINT) {
    l20_check_spec(sp, false);
    n = joint ? sp.G.st[2] : sp.G.N;
    l20_check_k<T>(sp.pmax, n);
    k = sp.pmax >= (double)n ? n : (long long)sp.pmax;
    g = this->template alloc<T>(n);
    const int nchunk = joint ? l21_joint_plan(n, sp.G.n[2], (int)sizeof(T)).nchunk : 1;
    if (nchunk > 1) part = this->template alloc<double>((size_t)nchunk * n);
    sel.build(this->mem, s, n, k);
  }
  void reset() override { sel.reinit(stream); calls = selections = 0; }
  void project(T* v, bool feas, double* partials, T* maxpart, T* compact) override {
    ++calls;
    if (k >= n) return;                // every group stays: nothing to select, nothing to write
    ++selections;
    l21_norms<T>(stream, sp, v, g, part);
    const ProjScalars<T>* ps = sel.run(stream, g, feas, partials, maxpart, compact);
    l20_zero<T>(stream, sp, v, g, n, ps, nullptr, nullptr, nullptr);
  }
  // out[p] <- g_p (n entries): the norms launch of project() into its own g, copied out; v is not written
  void observe(const T* v, T* out, double*, T*, T*) override {
    l21_norms<T>(stream, sp, v, g, part);
    SIPX_HIP(hipMemcpyAsync(out, g, sizeof(T) * (size_t)n, hipMemcpyDeviceToDevice, stream));
  }
  void set_data(const T*, const T*, bool) override { throw std::runtime_error(L20_NO_SET_DATA); }
  // projections since the reset, the selections the small route ran, those the search route ran (k >= n runs none), the groups
  void route_counts(long long out[4]) const override {
    out[0] = calls; out[1] = sel.small ? selections : 0; out[2] = sel.small ? 0 : selections; out[3] = n;
  }
};

// ---- EXT_L20_SEG: at most k (or k[frame]) pixels with a non-zero gradient vector in every z-slice, on the range of TV_xy (l20.h) ------------
//     k_l21_norms     as FrameProj launches it                                            reads 2 N words, writes N
//     k_l20_frames    one workgroup per frame on g alone: (need, tau, cut) of the frame   reads N (LDS) or (2 + bytes of T) N
//     k_l20_zero      the per-frame form; frames without need are skipped                 reads up to N, writes up to 2 N
// Nothing is kept between calls.  Built with ExtSpec::ub every frame has its own budget (kvec, n3 entries of T), sipx_set_data replaces them.
template <typename T>
struct L20FrameProj : ExtImpl<T> {
  using ExtImpl<T>::sp;
  using ExtImpl<T>::stream;
  T *g = nullptr, *tau = nullptr, *kvec = nullptr;
  int *need = nullptr, *cut = nullptr;
  long long nf = 0, L = 0;
  long long calls = 0, selections = 0;
  L20FrameProj(const ExtSpec& spec, hipStream_t s) : ExtImpl<T>(spec, s) {
    l20_check_spec(sp, true);
    nf = sp.G.n[2];
    L = sp.G.n[0] * sp.G.n[1];
    if (sp.ub) l20_check_k_vector<T>((const T*)sp.ub, nf, L);
    else l20_check_k<T>(sp.pmax, L);
    g = this->template alloc<T>(sp.G.N);
    tau = this->template alloc<T>(nf);
    need = this->template alloc<int>(2 * nf);
    cut = need + nf;
    if (sp.ub) {
      kvec = this->template alloc<T>(nf);
      SIPX_HIP(hipMemcpy(kvec, sp.ub, sizeof(T) * (size_t)nf, hipMemcpyHostToDevice));
    }
  }
  void reset() override { calls = selections = 0; }
  void project(T* v, bool, double*, T*, T*) override {
    ++calls;
    if (!kvec && sp.pmax >= (double)L) return;      // every group of every frame stays: nothing to select, nothing to write
    ++selections;
    l21_norms<T>(stream, sp, v, g);
    const L21SegPlan plan = l21_seg_plan(L, nf, (int)sizeof(T));
    {
      ObsScope obs(KID_L20_FRAMES, stream, (double)sp.G.N * sizeof(T));
      if (kvec)
        hipLaunchKernelGGL((k_l20_frames<T, true>), dim3(plan.grid), dim3(BLOCK), plan.lds_bytes, stream, plan, (unsigned)L, (unsigned)nf, g,
                           T(0), kvec, need, tau, cut);
      else
        hipLaunchKernelGGL((k_l20_frames<T, false>), dim3(plan.grid), dim3(BLOCK), plan.lds_bytes, stream, plan, (unsigned)L, (unsigned)nf, g,
                           (T)sp.pmax, (const T*)nullptr, need, tau, cut);
      SIPX_HIP(hipGetLastError());
    }
    l20_zero<T>(stream, sp, v, g, sp.G.N, nullptr, need, tau, cut);
  }
  // out[p] <- g_p (N entries, point order): the norms launch of project() into its own g, copied out; v is not written
  void observe(const T* v, T* out, double*, T*, T*) override {
    l21_norms<T>(stream, sp, v, g);
    SIPX_HIP(hipMemcpyAsync(out, g, sizeof(T) * (size_t)sp.G.N, hipMemcpyDeviceToDevice, stream));
  }
  void set_data(const T* new_lb, const T* new_ub, bool on_device) override {
    if (!kvec) throw std::runtime_error(L20_NO_SET_DATA);
    if (new_lb) throw std::runtime_error(L20_SET_DATA_UB);
    if (new_ub)
      SIPX_HIP(hipMemcpyAsync(kvec, new_ub, sizeof(T) * (size_t)nf, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
  }
  // projections since the reset, none by the small route, those that ran the per-frame selection, the groups of a frame
  void route_counts(long long out[4]) const override { out[0] = calls; out[1] = 0; out[2] = selections; out[3] = L; }
};

// ---- EXT_L1_WEIGHTED: the weighted l1 ball on the rows of identity, D_x, D_y, D_z, TV or TV_xy (l1_weighted.h) ------------------------------
// The iteration of the weighted route with k_l1w_part as its pass on the flat pair (v, w), then k_l1w_apply.  w lives in the padded layout of
// the operator: the weights arrive in the reference's row order (spec.lb, set_data) and go through the transfer kernel of the y_i / l_i
// (kernels_io.hip), which writes the rows a block has and nothing else -- the pads keep the zeros w was allocated with.  Nothing is kept
// between calls.
static void l1w_check_spec(const ExtSpec& sp) {
  if (sp.mode != SIPX_MODE_WHOLE) throw std::runtime_error(L1W_NO_MODE);
  if (!sp.weighted) throw std::runtime_error(L1W_NEEDS_WEIGHTS);
  if (sp.ub) throw std::runtime_error(L1W_NO_UB);
  if (sp.nblk < 0 || sp.nblk > 3 || sp.nblk > sp.ndim) throw std::runtime_error("the weighted l1 ball: 0 to 3 operator blocks, no more than grid dimensions");
  for (int q = 0; q < sp.nblk; ++q) {
    if (sp.bdir[q] < 0 || sp.bdir[q] >= sp.ndim) throw std::runtime_error("the weighted l1 ball: block direction out of range");
    if (sp.G.n[sp.bdir[q]] < 2) throw std::runtime_error("the weighted l1 ball: difference along a dimension of size 1");
    for (int r = 0; r < q; ++r)
      if (sp.bdir[q] == sp.bdir[r]) throw std::runtime_error("the weighted l1 ball: two blocks along one direction");
  }
  if (sp.nblk > 1 && sp.bstride != sp.G.N) throw std::runtime_error("the weighted l1 ball: the blocks must lie side by side (bstride == N)");
  if ((long long)std::max(sp.nblk, 1) * sp.G.N >= (1ll << 31)) throw std::runtime_error("the weighted l1 ball: the operator needs fewer than 2^31 padded rows");
}
template <typename T>
struct L1WProj : ExtImpl<T> {
  using ExtImpl<T>::sp;
  using ExtImpl<T>::stream;
  long long n = 0;                     // entries of the padded layout: max(nblk, 1) N, the length of the search
  long long rows = 0;                  // rows of the operator (Mtrue): the weights a caller hands over
  long long blk_rows[3] = {0, 0, 0};
  T* w = nullptr;                      // the weights in the padded layout, 0 at every pad
  T* wrows = nullptr;                  // where host weights land in row order before they are expanded
  L21WSearch<T, true> ws;
  L1WProj(const ExtSpec& spec, hipStream_t s) : ExtImpl<T>(spec, s) {
    l1w_check_spec(sp);
    if (!(sp.pmax > 0)) throw std::runtime_error("Radius of L1 ball is negative");
    n = (long long)std::max(sp.nblk, 1) * sp.G.N;
    for (int q = 0; q < sp.nblk; ++q) {
      blk_rows[q] = sp.G.N / sp.G.n[sp.bdir[q]] * (sp.G.n[sp.bdir[q]] - 1);
      rows += blk_rows[q];
    }
    if (sp.nblk == 0) rows = sp.G.N;
    w = this->mem.template alloc<T>((size_t)n, Mem::Zeroed);      // (until weights arrive no row is constrained; the pads stay 0 for good)
    wrows = this->template alloc<T>((size_t)rows);
    ws.build(*this);
    if (sp.lb) expand((const T*)sp.lb, false);
  }
  // w <- the weights given in row order, host or device memory, block by block into the rows each block has
  void expand(const T* src, bool on_device) {
    if (!on_device) {
      SIPX_HIP(hipMemcpyAsync(wrows, src, sizeof(T) * (size_t)rows, hipMemcpyHostToDevice, stream));
      src = wrows;
    }
    IoArgs<T> A;
    if (sp.nblk == 0) io_seg_shape<T>(A.seg[A.nseg++], sp.G, -1, rows, src, w);
    long long r0 = 0;
    for (int q = 0; q < sp.nblk; ++q) {
      io_seg_shape<T>(A.seg[A.nseg++], sp.G, sp.bdir[q], blk_rows[q], src + r0, w + (long long)q * sp.G.N);
      r0 += blk_rows[q];
    }
    io_rows<T>(stream, A, false, NB);
    if (!on_device) SIPX_HIP(hipStreamSynchronize(stream));      // (the caller's host vector may go once the call returns)
  }
  bool wide(const T* v) const { return sp.G.n[0] % 4 == 0 && aligned16(v, w); }
  void apply(T* v) {
    constexpr int W = l21_vec_width<T>();
    const bool wd = wide(v);
    ObsScope obs(KID_L1W_APPLY, stream, 3.0 * n * sizeof(T));
    hipLaunchKernelGGL((wd ? k_l1w_apply<T, W> : k_l1w_apply<T, 1>), dim3(fit_grid(n / (wd ? W : 1), NB)), dim3(BLOCK), 0, stream, (unsigned)n, v, w,
                       ws.st, ws.theta);
    SIPX_HIP(hipGetLastError());
  }
  void project(T* v, bool, double*, T*, T*) override {
    ws.run(stream, n, v, w, wide(v), (T)sp.pmax);
    apply(v);
  }
  // out[0] <- (T)asum as project decides on it: the first pass of its iteration with an infinite radius
  void observe(const T* v, T* out, double*, T*, T*) override {
    ws.template pass<true>(stream, n, v, w, wide(v), (T)INFINITY);
    ws.pick(stream, out);
  }
  void set_data(const T* new_lb, const T* new_ub, bool on_device) override {
    if (new_ub) throw std::runtime_error(L1W_SET_DATA_UB);
    if (new_lb) expand(new_lb, on_device);
  }
  // the passes of the last call (the first included), the reads of the flag it took, the calls so far, the padded rows
  void route_counts(long long out[4]) const override {
    out[0] = ws.last_passes; out[1] = ws.last_reads; out[2] = ws.calls; out[3] = n;
  }
};

// ---- EXT_L2INF, EXT_L2INF_JOINT, EXT_L2INF_STACKED: the group norms bounded one by one (l2inf.h) --------------------------------------------
// One sweep (k_l2inf_clip, k_l2infs_clip), or for the joint set the z-march of the l2,1 ball into g and k_l2inf_scale.  No search, no warm
// start, nothing kept between calls.  Built with ExtSpec::ub every group has its own bound (cvec, n entries of T), sipx_set_data replaces
// them.  g and the partial maxima exist for the joint set and, from its first call on, for the observer.
static void l2inf_check_spec(const ExtSpec& sp) {
  if (sp.kind == EXT_L2INF_STACKED) {
    const long long G = l2infs_check_shape(sp.G.N, sp.nblk);
    if (sp.bstride != G) throw std::runtime_error("the stacked l2,inf ball: the block stride must be the rows of one block");
  } else {
    if (sp.nblk < 2) throw std::runtime_error(L2INF_NEEDS_TV);
    l21_check_spec(sp);
    if (sp.kind == EXT_L2INF_JOINT && (sp.ndim != 3 || sp.nblk != 2 || sp.bdir[0] != 1 || sp.bdir[1] != 0)) throw std::runtime_error(L2INF_JOINT_ROUTE);
  }
  if (sp.mode != SIPX_MODE_WHOLE) throw std::runtime_error(L2INF_MODES);
  if (sp.lb || sp.weighted) throw std::runtime_error(L2INF_NO_WEIGHTS);
  if (!sp.ub) l2inf_check_c(sp.pmax);
}
// the groups of a spec: the entries of a vector of bounds and of g
static long long l2inf_groups(const ExtSpec& sp) {
  return sp.kind == EXT_L2INF_STACKED ? sp.bstride : (sp.kind == EXT_L2INF_JOINT ? sp.G.st[2] : sp.G.N);
}
template <typename T>
struct L2InfProj : ExtImpl<T> {
  using ExtImpl<T>::sp;
  using ExtImpl<T>::stream;
  const bool joint, stacked;
  long long n = 0;                     // groups: the entries of cvec and of g
  T* cvec = nullptr;                   // one bound per group, or none: the scalar sp.pmax
  T* g = nullptr;                      // the group norms: the joint set's, and the observer's
  double* part = nullptr;              // EXT_L2INF_JOINT: the chunk sums, nchunk L entries, when the plan chunks
  T* mpart = nullptr;                  // the observer's maxima of the workgroups, NB entries
  long long calls = 0;
  L2InfProj(const ExtSpec& spec, hipStream_t s)
      : ExtImpl<T>(spec, s), joint(spec.kind == EXT_L2INF_JOINT), stacked(spec.kind == EXT_L2INF_STACKED) {
    l2inf_check_spec(sp);
    n = l2inf_groups(sp);
    if (sp.ub) {
      cvec = this->template alloc<T>(n);
      SIPX_HIP(hipMemcpy(cvec, sp.ub, sizeof(T) * (size_t)n, hipMemcpyHostToDevice));
    }
    if (joint) norms_memory();
  }
  void norms_memory() {
    if (g) return;
    g = this->template alloc<T>(n);
    const int nchunk = joint ? l21_joint_plan(n, sp.G.n[2], (int)sizeof(T)).nchunk : 1;
    if (nchunk > 1) part = this->template alloc<double>((size_t)nchunk * n);
  }
  // g <- the group norms of v by the norms launch of the l2,1 ball on the same operator
  void norms(const T* v) {
    norms_memory();
    if (stacked) l21s_norms<T>(stream, sp, v, g);
    else l21_norms<T>(stream, sp, v, g, part);
  }
  void reset() override { calls = 0; }
  void project(T* v, bool, double*, T*, T*) override {
    ++calls;
    constexpr int W = l21_vec_width<T>();
    const T c = (T)sp.pmax;
    const double cw = cvec ? 1.0 : 0.0;      // (the words of c a group reads; the booked traffic is that of a call that clips everywhere)
    if (stacked) {
      const bool wide = l21s_wide(sp, v, cvec);
      const long long G = sp.bstride;
      void (*const k)(unsigned, int, T*, const T*, T) =
          sp.nblk == 3   ? (cvec ? (wide ? k_l2infs_clip<T, 3, W, true> : k_l2infs_clip<T, 3, 1, true>)
                                 : (wide ? k_l2infs_clip<T, 3, W, false> : k_l2infs_clip<T, 3, 1, false>))
          : sp.nblk == 6 ? (cvec ? (wide ? k_l2infs_clip<T, 6, W, true> : k_l2infs_clip<T, 6, 1, true>)
                                 : (wide ? k_l2infs_clip<T, 6, W, false> : k_l2infs_clip<T, 6, 1, false>))
                         : (cvec ? (wide ? k_l2infs_clip<T, 0, W, true> : k_l2infs_clip<T, 0, 1, true>)
                                 : (wide ? k_l2infs_clip<T, 0, W, false> : k_l2infs_clip<T, 0, 1, false>));
      ObsScope obs(KID_L2INFS_CLIP, stream, (double)(2 * sp.nblk + cw) * G * sizeof(T));
      hipLaunchKernelGGL(k, dim3(fit_grid(G / (wide ? W : 1), NB)), dim3(BLOCK), 0, stream, (unsigned)G, sp.nblk, v, (const T*)cvec, c);
      SIPX_HIP(hipGetLastError());
      return;
    }
    const bool wide = l21_wide(sp, v, cvec);
    const long long N = sp.G.N;
    const int grid = fit_grid(N / (wide ? W : 1), NB);
    if (joint) {
      norms(v);
      void (*const k)(L21Args, T*, const T*, const T*, T) =
          cvec ? (wide ? k_l2inf_scale<T, 2, W, true, true> : k_l2inf_scale<T, 2, 1, true, true>)
               : (wide ? k_l2inf_scale<T, 2, W, false, true> : k_l2inf_scale<T, 2, 1, false, true>);
      ObsScope obs(KID_L2INF_SCALE, stream, (4.0 * N + (1 + cw) * n) * sizeof(T));
      hipLaunchKernelGGL(k, dim3(grid), dim3(BLOCK), 0, stream, l21_args(sp), v, (const T*)g, (const T*)cvec, c);
      SIPX_HIP(hipGetLastError());
      return;
    }
    void (*const k)(L21Args, T*, const T*, T) =
        sp.nblk == 2 ? (cvec ? (wide ? k_l2inf_clip<T, 2, W, true> : k_l2inf_clip<T, 2, 1, true>)
                             : (wide ? k_l2inf_clip<T, 2, W, false> : k_l2inf_clip<T, 2, 1, false>))
                     : (cvec ? (wide ? k_l2inf_clip<T, 3, W, true> : k_l2inf_clip<T, 3, 1, true>)
                             : (wide ? k_l2inf_clip<T, 3, W, false> : k_l2inf_clip<T, 3, 1, false>));
    ObsScope obs(KID_L2INF_CLIP, stream, (double)(2 * sp.nblk + cw) * N * sizeof(T));
    hipLaunchKernelGGL(k, dim3(grid), dim3(BLOCK), 0, stream, l21_args(sp), v, (const T*)cvec, c);
    SIPX_HIP(hipGetLastError());
  }
  // out[0] <- max_p g_p: the norms launch on the operator of the set -- the arithmetic of the clip kernels, bit for bit -- and the
  // maximum of g in two stages; v is not written
  void observe(const T* v, T* out, double*, T*, T*) override {
    norms(v);
    if (!mpart) mpart = this->template alloc<T>(NB);
    const int grid = fit_grid(n, NB);
    hipLaunchKernelGGL((k_l2inf_max_part<T>), dim3(grid), dim3(BLOCK), 0, stream, (unsigned)n, (const T*)g, mpart);
    SIPX_HIP(hipGetLastError());
    hipLaunchKernelGGL((k_l2inf_max_final<T>), dim3(1), dim3(BLOCK), 0, stream, grid, (const T*)mpart, out);
    SIPX_HIP(hipGetLastError());
  }
  void set_data(const T* new_lb, const T* new_ub, bool on_device) override {
    if (new_lb) throw std::runtime_error(L2INF_NO_WEIGHTS);
    if (!cvec) throw std::runtime_error(L2INF_NO_SET_DATA);
    if (new_ub)
      SIPX_HIP(hipMemcpyAsync(cvec, new_ub, sizeof(T) * (size_t)n, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
  }
  // projections since the reset; the groups
  void route_counts(long long out[4]) const override { out[0] = calls; out[1] = out[2] = 0; out[3] = n; }
};

template <typename T>
ExtImpl<T>* make_group_family(const ExtSpec& spec, hipStream_t stream) {
  if (spec.kind == EXT_L2INF || spec.kind == EXT_L2INF_JOINT || spec.kind == EXT_L2INF_STACKED) return new L2InfProj<T>(spec, stream);
  if (spec.kind == EXT_L1_WEIGHTED) return new L1WProj<T>(spec, stream);
  if (spec.kind == EXT_L21_GROUPS) return new GroupsProj<T>(spec, stream);
  if (spec.kind == EXT_CARD_GROUPS) return new CardGroupsProj<T>(spec, stream);
  if (spec.kind == EXT_L20 || spec.kind == EXT_L20_JOINT) return new L20Proj<T>(spec, stream);
  if (spec.kind == EXT_L20_SEG) return new L20FrameProj<T>(spec, stream);
  if (spec.kind == EXT_TNV) return new TnvProj<T>(spec, stream);
  if (spec.kind == EXT_L21_SEG) return new FrameProj<T>(spec, stream);
  if (spec.kind != EXT_L21 && spec.kind != EXT_L21_JOINT && spec.kind != EXT_L21_STACKED) throw std::runtime_error("unknown external projector");
  return new BallProj<T>(spec, stream);
}

template ExtImpl<float>* make_group_family<float>(const ExtSpec&, hipStream_t);
template ExtImpl<double>* make_group_family<double>(const ExtSpec&, hipStream_t);

}  // namespace sipx
