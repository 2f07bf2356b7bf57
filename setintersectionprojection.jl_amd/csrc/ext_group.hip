// Group norms across the blocks of a multi-block operator: the l2,1 ball on the range of the TV operator (isotropic total
// variation, EXT_L21).  The rule is written down in l21.h; here are the two streaming kernels and the projector
//     k_l21_norms     g[p] <- the l2 norm of the group of grid point p              reads nblk N words, writes N
//     the engine's l1 threshold search on the array g (K<T>::proj_scalars_arr)     its passes over N words
//     k_l21_scale     v_q[p] <- v_q[p] * f_p unless the search found v inside     reads (nblk + 1) N words, writes nblk N
// -- (2 nblk + 2) N words plus the search per projection outside the set.  The reference package has no such projector.
// Float64 only: between the search and k_l21_scale, k_l21_theta_part / k_l21_theta_final re-evaluate the threshold on the search's
// active set in twice the working precision (one more pass over g, N words; l21.h THRESHOLD IN FLOAT64).
//
// Both kernels are grid-stride over the N grid points with 32-bit index arithmetic (N < 2^31 is checked when the projector is
// built), use no LDS, and take VW points per thread: 16 bytes of every array when n1 % 4 == 0 (then N and every block base
// are 16-byte aligned and the VW points lie on one grid line), one point otherwise.  g lives in the projector's own memory.
#include "ext_family.h"
#include "l21.h"

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

template <typename T, int NBLK, int VW>
__global__ __launch_bounds__(BLOCK) void k_l21_scale(L21Args a, T* __restrict__ v, const T* __restrict__ g,
                                                     const ProjScalars<T>* __restrict__ ps, const T* __restrict__ theta) {
  if (!ps->need) return;
  const T th = theta ? theta[0] : ps->theta;          // (Float64: the threshold k_l21_theta_final left)
  const unsigned nvec = (unsigned)(a.G.N / VW), step = gridDim.x * BLOCK;
  for (unsigned vi = blockIdx.x * BLOCK + threadIdx.x; vi < nvec; vi += step) {
    const unsigned p = vi * VW;
    const Coord c = coords(a.G, (long long)p);
    const Vec<T, VW> gv = ldv<T, VW>(g + p);
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
      for (int k = 0; k < VW; ++k) x.v[k] = x.v[k] * f[k];
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
  __shared__ double sh[BLOCK], sl[BLOCK], sc[BLOCK];
  const double th = ps->theta;
  L21Sum acc{0.0, 0.0};
  double cnt = 0.0;
  for (unsigned p = blockIdx.x * BLOCK + threadIdx.x; p < N; p += gridDim.x * BLOCK) {
    const double a = g[p];
    if (a > th) { l21_sum_add(acc, a); cnt += 1.0; }
  }
  sh[threadIdx.x] = acc.hi; sl[threadIdx.x] = acc.lo; sc[threadIdx.x] = cnt;
  __syncthreads();
  for (int w = BLOCK / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      L21Sum a{sh[threadIdx.x], sl[threadIdx.x]};
      l21_sum_merge(a, L21Sum{sh[threadIdx.x + w], sl[threadIdx.x + w]});
      sh[threadIdx.x] = a.hi; sl[threadIdx.x] = a.lo; sc[threadIdx.x] += sc[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { part[3 * blockIdx.x] = sh[0]; part[3 * blockIdx.x + 1] = sl[0]; part[3 * blockIdx.x + 2] = sc[0]; }
}
__global__ __launch_bounds__(BLOCK) void k_l21_theta_final(int nparts, unsigned N, double tau, const double* __restrict__ part,
                                                           const ProjScalars<double>* __restrict__ ps, double* __restrict__ theta) {
  __shared__ double sh[BLOCK], sl[BLOCK], sc[BLOCK];
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
  sh[threadIdx.x] = acc.hi; sl[threadIdx.x] = acc.lo; sc[threadIdx.x] = cnt;
  __syncthreads();
  for (int w = BLOCK / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      L21Sum a{sh[threadIdx.x], sl[threadIdx.x]};
      l21_sum_merge(a, L21Sum{sh[threadIdx.x + w], sl[threadIdx.x + w]});
      sh[threadIdx.x] = a.hi; sl[threadIdx.x] = a.lo; sc[threadIdx.x] += sc[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) theta[0] = l21_theta_refined(L21Sum{sh[0], sl[0]}, sc[0], tau, (double)N, ps->theta);
}

// out[0] <- (T) ||g||_1 as the search's first pass summed it: the number its decision compares with the radius
template <typename T>
__global__ void k_l21_pick(const ProjScalars<T>* __restrict__ ps, T* __restrict__ out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) out[0] = (T)ps->asum;
}

static void l21_check_spec(const ExtSpec& sp) {
  if (sp.nblk != 2 && sp.nblk != 3) throw std::runtime_error("the l2,1 ball needs the 2 or 3 blocks of the TV operator");
  if (sp.nblk != sp.ndim) throw std::runtime_error("the l2,1 ball: one block per grid dimension");
  if (sp.G.N >= (1ll << 31)) throw std::runtime_error("the l2,1 ball: the grid needs fewer than 2^31 points");
  if (sp.bstride < sp.G.N) throw std::runtime_error("the l2,1 ball: the blocks overlap");
  for (int q = 0; q < sp.nblk; ++q)
    if (sp.bdir[q] < 0 || sp.bdir[q] >= sp.ndim) throw std::runtime_error("the l2,1 ball: block direction out of range");
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
template <typename T>
static void l21_norms(hipStream_t s, const ExtSpec& sp, const T* v, T* g) {
  constexpr int W = l21_vec_width<T>();
  const L21Args a = l21_args(sp);
  const bool wide = l21_wide(sp, v, g);
  const int grid = fit_grid(sp.G.N / (wide ? W : 1), NB);
  if (sp.nblk == 2 && wide) hipLaunchKernelGGL((k_l21_norms<T, 2, W>), dim3(grid), dim3(BLOCK), 0, s, a, v, g);
  else if (sp.nblk == 2) hipLaunchKernelGGL((k_l21_norms<T, 2, 1>), dim3(grid), dim3(BLOCK), 0, s, a, v, g);
  else if (wide) hipLaunchKernelGGL((k_l21_norms<T, 3, W>), dim3(grid), dim3(BLOCK), 0, s, a, v, g);
  else hipLaunchKernelGGL((k_l21_norms<T, 3, 1>), dim3(grid), dim3(BLOCK), 0, s, a, v, g);
  SIPX_HIP(hipGetLastError());
}
template <typename T>
static void l21_scale(hipStream_t s, const ExtSpec& sp, T* v, const T* g, const ProjScalars<T>* ps, const T* theta) {
  constexpr int W = l21_vec_width<T>();
  const L21Args a = l21_args(sp);
  const bool wide = l21_wide(sp, v, g);
  const int grid = fit_grid(sp.G.N / (wide ? W : 1), NB);
  if (sp.nblk == 2 && wide) hipLaunchKernelGGL((k_l21_scale<T, 2, W>), dim3(grid), dim3(BLOCK), 0, s, a, v, g, ps, theta);
  else if (sp.nblk == 2) hipLaunchKernelGGL((k_l21_scale<T, 2, 1>), dim3(grid), dim3(BLOCK), 0, s, a, v, g, ps, theta);
  else if (wide) hipLaunchKernelGGL((k_l21_scale<T, 3, W>), dim3(grid), dim3(BLOCK), 0, s, a, v, g, ps, theta);
  else hipLaunchKernelGGL((k_l21_scale<T, 3, 1>), dim3(grid), dim3(BLOCK), 0, s, a, v, g, ps, theta);
  SIPX_HIP(hipGetLastError());
}

template <typename T>
struct GroupProj : ExtImpl<T> {
  using ExtImpl<T>::sp;
  using ExtImpl<T>::stream;
  T* g = nullptr;                      // the group norms, N entries
  double* tpart = nullptr;             // Float64: the partial sums of k_l21_theta_part
  T* theta = nullptr;                  // Float64: the threshold k_l21_scale applies
  SearchState<T> search;
  void reset() override { search.reinit(stream); }
  GroupProj(const ExtSpec& spec, hipStream_t s) : ExtImpl<T>(spec, s) {
    l21_check_spec(sp);
    if (!(sp.pmax > 0)) throw std::runtime_error("Radius of L1 ball is negative");
    g = this->template alloc<T>(sp.G.N);
    if (sizeof(T) == 8) {
      tpart = this->template alloc<double>(3 * L21_THETA_GRID);
      theta = this->template alloc<T>(1);
    }
    search.build(this->mem, s, 0);
  }
  void project(T* v, bool feas, double* partials, T* maxpart, T* compact) override {
    const long long N = sp.G.N;
    ProjScalars<T>* ps = search.pick(feas);
    l21_norms<T>(stream, sp, v, g);
    K<T>::proj_scalars_arr(stream, N, g, PX_L1, T(0), (T)sp.pmax, ps, partials, maxpart, compact, N);
    if constexpr (sizeof(T) == 8) {
      const int grid = fit_grid(N, L21_THETA_GRID);
      hipLaunchKernelGGL(k_l21_theta_part, dim3(grid), dim3(BLOCK), 0, stream, (unsigned)N, g, ps, tpart);
      hipLaunchKernelGGL(k_l21_theta_final, dim3(1), dim3(BLOCK), 0, stream, grid, (unsigned)N, (double)sp.pmax, tpart, ps, theta);
      SIPX_HIP(hipGetLastError());
    }
    l21_scale<T>(stream, sp, v, g, ps, theta);
  }
};

template <typename T>
ExtImpl<T>* make_group_family(const ExtSpec& spec, hipStream_t stream) {
  if (spec.kind != EXT_L21) throw std::runtime_error("unknown external projector");
  return new GroupProj<T>(spec, stream);
}

// out[0] (device) <- ||v||_2,1 of a materialised vector in the layout of spec: k_l21_norms into g (N entries), then the first pass
// of a search with a new state and an infinite radius -- the sum, and the rounding to T, of the projector's own decision
template <typename T>
void l21_observe(const ExtSpec& spec, const T* v, T* g, ProjScalars<T>* ps, double* partials, T* maxpart, T* compact, T* out,
                 hipStream_t stream) {
  l21_check_spec(spec);
  const long long N = spec.G.N;
  l21_norms<T>(stream, spec, v, g);
  K<T>::ps_init(stream, ps, nullptr);
  K<T>::proj_scalars_arr(stream, N, g, PX_L1, T(0), (T)INFINITY, ps, partials, maxpart, compact, N);
  hipLaunchKernelGGL((k_l21_pick<T>), dim3(1), dim3(64), 0, stream, ps, out);
  SIPX_HIP(hipGetLastError());
}

template ExtImpl<float>* make_group_family<float>(const ExtSpec&, hipStream_t);
template ExtImpl<double>* make_group_family<double>(const ExtSpec&, hipStream_t);
template void l21_observe<float>(const ExtSpec&, const float*, float*, ProjScalars<float>*, double*, float*, float*, float*, hipStream_t);
template void l21_observe<double>(const ExtSpec&, const double*, double*, ProjScalars<double>*, double*, double*, double*, double*,
                                  hipStream_t);

}  // namespace sipx
