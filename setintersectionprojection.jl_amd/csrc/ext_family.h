// Private to the ext_*.hip units: what ExtProj<T> (ext_proj.h) forwards to, one object per family of projectors --
//   ext_transform.hip  DFT mask, l1 and cardinality behind the DFT, DCT, DWT
//   ext_rank.hip       slice / matrix rank, nuclear norm
//   ext_segments.hip   cardinality, l1, l2 and annulus per fiber / slice (seg_norm.h), the simplex per fiber / slice (seg_simplex.h),
//                      relaxed histogram, subspace
//   ext_group.hip      the l2,1 ball across the blocks of the TV / TV_xy operator: BallProj on the whole array (l21.h) or with groups
//                      across the frames (l21_joint.h) or across the equal-sized blocks of a caller-supplied stacked operator (l21_stacked.h),
//                      FrameProj per z-slice (l21_seg.h); GroupsProj: the l2,1 ball whose groups are the
//                      fibers or slices of a one-block operator's range (l21_groups.h); CardGroupsProj: at most k non-zero ones (card_groups.h); L20Proj / L20FrameProj: at most k non-zero gradient groups of TV / TV_xy (l20.h); L1WProj: the weighted l1 ball on the rows of an
//                      operator (l1_weighted.h); L2InfProj: every group norm of TV / TV_xy, of the joint groups or of a stacked operator
//                      bounded on its own (l2inf.h)
// -- and what more than one family uses.
#pragma once
#define ROCBLAS_BETA_FEATURES_API 1
#define ROCBLAS_NO_DEPRECATED_WARNINGS 1
#include <hipfft/hipfft.h>
#include <rocblas/rocblas.h>

#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/sipx.h"
#include "device_memory.h"
#include "ext_proj.h"
#include "sipx_device.h"

namespace sipx {

// One projector.  A family's constructor that throws halfway releases what it had taken: handles live in members that destroy
// themselves (BlasHandle, and the like in the units), device memory in `mem`, which frees it with the projector.
template <typename T>
struct ExtImpl {
  ExtSpec sp;
  hipStream_t stream;
  DeviceMemory mem;
  ExtImpl(const ExtSpec& spec, hipStream_t s) : sp(spec), stream(s) {}
  virtual ~ExtImpl() {}
  // v <- P(v) in place; feas selects the warm-start state of the feasibility estimate
  virtual void project(T* v, bool feas, double* partials, T* maxpart, T* compact) = 0;
  virtual void set_stream(hipStream_t s) { stream = s; }
  virtual void reset() {}
  // sipx_set_data: new lb / ub (nullptr keeps one), host or device memory
  virtual void set_data(const T*, const T*, bool) { throw std::runtime_error("this projector holds no replaceable vectors (build a new context)"); }
  virtual void route_counts(long long out[4]) const { out[0] = out[1] = out[2] = out[3] = 0; }
  // out (device) <- the number(s) project(v, ...) would compare with the radius; v is not written (ext_proj.h)
  virtual void observe(const T*, T*, double*, T*, T*) { throw std::runtime_error("this projector has no observer"); }
  template <typename Q>
  Q* alloc(size_t count) { return mem.template alloc<Q>(count ? count : 1, Mem::NoFill); }
};
template <typename T> ExtImpl<T>* make_transform_family(const ExtSpec& spec, hipStream_t stream);
template <typename T> ExtImpl<T>* make_rank_family(const ExtSpec& spec, hipStream_t stream);
template <typename T> ExtImpl<T>* make_segment_family(const ExtSpec& spec, hipStream_t stream);
template <typename T> ExtImpl<T>* make_group_family(const ExtSpec& spec, hipStream_t stream);

inline void fft_check(hipfftResult r, const char* what) {
  if (r != HIPFFT_SUCCESS) throw std::runtime_error(std::string("hipFFT: ") + what + " failed (" + std::to_string((int)r) + ")");
}
inline void blas_check(rocblas_status r, const char* what) {
  if (r != rocblas_status_success) throw std::runtime_error(std::string("rocBLAS/rocSOLVER: ") + what + " failed (" + std::to_string((int)r) + ")");
}
// a rocBLAS handle on the projector's stream
struct BlasHandle {
  rocblas_handle h = nullptr;
  void create(hipStream_t s) {
    blas_check(rocblas_create_handle(&h), "create handle");
    blas_check(rocblas_set_stream(h, s), "set stream");
  }
  void set_stream(hipStream_t s) { if (h) blas_check(rocblas_set_stream(h, s), "set stream"); }
  operator rocblas_handle() const { return h; }
  ~BlasHandle() { if (h) (void)rocblas_destroy_handle(h); }
};
inline rocblas_status gemm_T(rocblas_handle h, rocblas_operation ta, rocblas_operation tb, int m, int n, int k, const float* A,
                             int lda, const float* B, int ldb, float* C, int ldc) {
  const float one = 1.f, zero = 0.f;
  return rocblas_sgemm(h, ta, tb, m, n, k, &one, A, lda, B, ldb, &zero, C, ldc);
}
inline rocblas_status gemm_T(rocblas_handle h, rocblas_operation ta, rocblas_operation tb, int m, int n, int k, const double* A,
                             int lda, const double* B, int ldb, double* C, int ldc) {
  const double one = 1.0, zero = 0.0;
  return rocblas_dgemm(h, ta, tb, m, n, k, &one, A, lda, B, ldb, &zero, C, ldc);
}

// The state of the engine's threshold searches (l1, cardinality), one for the y update and one for the feasibility estimate;
// cidx: the indices of the gathered magnitudes (the tie cut of a cardinality search), n_idx entries or none.
template <typename T>
struct SearchState {
  ProjScalars<T>*ps = nullptr, *psf = nullptr;
  long long* cidx = nullptr;
  void build(DeviceMemory& mem, hipStream_t s, long long n_idx) {
    ps = mem.template alloc<ProjScalars<T>>(1, Mem::NoFill);
    psf = mem.template alloc<ProjScalars<T>>(1, Mem::NoFill);
    if (n_idx) cidx = mem.template alloc<long long>(n_idx, Mem::NoFill);
    reinit(s);
  }
  void reinit(hipStream_t s) {       // a projector without a search (never built) has nothing to forget
    if (ps) K<T>::ps_init(s, ps, cidx);
    if (psf) K<T>::ps_init(s, psf, cidx);
  }
  ProjScalars<T>* pick(bool feas) const { return feas ? psf : ps; }
};

// ------------------------------------------------------------------------------------------------
// Segments of the padded array: the whole valid block, its fibers along one direction, or its slices.
// Element t of segment s lives at seg_addr(s, t); t runs in the reference's order (lower dimension fastest:
// reshape / permutedims of project_cardinality!.jl:111-120, project_subspace!.jl:91-100, view(x,i,:,:) etc.).
struct SegMap {
  long long nseg, L;
  long long SA, sSa, sSb;            // s -> (s % SA) * sSa + (s / SA) * sSb
  long long LA, LB, sTa, sTb, sTc;   // t = ta + LA * (tb + LB * tc) -> ta * sTa + tb * sTb + tc * sTc
};
__host__ __device__ __forceinline__ long long seg_addr(const SegMap& m, long long s, long long t) {
  const long long ta = t % m.LA, r = t / m.LA, tb = r % m.LB, tc = r / m.LB;
  return (s % m.SA) * m.sSa + (s / m.SA) * m.sSb + ta * m.sTa + tb * m.sTb + tc * m.sTc;
}
inline SegMap make_segmap(const ExtSpec& sp) {
  SegMap m{};
  const long long* d = sp.dims;
  const long long* st = sp.G.st;
  m.SA = 1; m.LA = 1; m.LB = 1;
  if (sp.mode == SIPX_MODE_WHOLE) {
    m.nseg = 1; m.L = d[0] * d[1] * d[2];
    m.LA = d[0]; m.LB = d[1]; m.sTa = st[0]; m.sTb = st[1]; m.sTc = st[2];
  } else {
    const int dir = sp.dir;
    if (dir < 0 || dir > 2) throw std::runtime_error("application mode: direction out of range");
    const int a = dir == 0 ? 1 : 0, b = dir == 2 ? 1 : 2;
    if (sp.mode == SIPX_MODE_FIBER) {
      m.L = d[dir]; m.LA = d[dir]; m.sTa = st[dir];
      m.SA = d[a]; m.sSa = st[a]; m.sSb = st[b]; m.nseg = d[a] * d[b];
    } else if (sp.mode == SIPX_MODE_SLICE) {
      m.LA = d[a]; m.LB = d[b]; m.sTa = st[a]; m.sTb = st[b]; m.L = d[a] * d[b];
      m.SA = d[dir]; m.sSa = st[dir]; m.nseg = d[dir];
    } else {
      throw std::runtime_error("unknown application mode");
    }
  }
  return m;
}
// segments of a spec: the entries of seg_observe's output and of a vector of per-segment radii
inline long long seg_count(const ExtSpec& spec) { return make_segmap(spec).nseg; }

// dense[s * L + t] <- v[seg_addr(s, t)] and back (U = double for the SVD path, T otherwise).  `flag` (optional):
// segments with flag[s] == 0 are left untouched by the scatter.
template <typename T, typename U>
__global__ __launch_bounds__(BLOCK) void k_seg_gather(SegMap m, const T* __restrict__ v, U* __restrict__ dense) {
  const long long tot = m.nseg * m.L;
  for (long long e = (long long)blockIdx.x * BLOCK + threadIdx.x; e < tot; e += (long long)gridDim.x * BLOCK) {
    const long long s = e / m.L, t = e - s * m.L;
    dense[e] = (U)v[seg_addr(m, s, t)];
  }
}
template <typename T, typename U>
__global__ __launch_bounds__(BLOCK) void k_seg_scatter(SegMap m, const U* __restrict__ dense, T* __restrict__ v,
                                                       const int* __restrict__ flag) {
  const long long tot = m.nseg * m.L;
  for (long long e = (long long)blockIdx.x * BLOCK + threadIdx.x; e < tot; e += (long long)gridDim.x * BLOCK) {
    const long long s = e / m.L, t = e - s * m.L;
    if (flag && !flag[s]) continue;
    v[seg_addr(m, s, t)] = (T)dense[e];
  }
}

}  // namespace sipx
