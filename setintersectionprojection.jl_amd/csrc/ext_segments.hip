// Projectors on the fibers, the slices or the whole of a materialised vector v that need no transform:
//   cardinality per fiber / slice (one kernel), the l1 ball, the l2 ball and the annulus per fiber / slice (one kernel,
//   seg_norm.h), the simplex per fiber / slice (two kernels, seg_simplex.h), the relaxed histogram (hipCUB sort), the subspace
//   projection (rocBLAS).
#include <hipcub/hipcub.hpp>

#include <cmath>

#include "ext_family.h"
#include "seg_norm.h"
#include "seg_simplex.h"

namespace sipx {

// ------------------------------------------------------------------------------------------------
// Cardinality per segment (project_cardinality!.jl:23-146): keep the k entries of largest magnitude of every fiber /
// slice, zero the rest; equal magnitudes keep the earlier entry (sortperm(by=abs, rev=true) is stable).
// One workgroup per segment: radix select on the magnitude bit pattern (8 bits a pass, histogram in LDS),
// then one ordered pass that resolves the tie cut with wave ballots.
template <typename T> struct KeyOf;
template <> struct KeyOf<float> { using U = unsigned int; };
template <> struct KeyOf<double> { using U = unsigned long long; };
__device__ __forceinline__ unsigned int abs_key(float v) { return __float_as_uint(v) & 0x7fffffffu; }
__device__ __forceinline__ unsigned long long abs_key(double v) {
  return (unsigned long long)__double_as_longlong(v) & 0x7fffffffffffffffull;
}
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_seg_card(SegMap m, T* __restrict__ v, long long k) {
  using U = typename KeyOf<T>::U;
  constexpr int BITS = (int)sizeof(U) * 8;
  __shared__ unsigned int hist[256];
  __shared__ U s_prefix;
  __shared__ long long s_kk, s_run;
  __shared__ unsigned int s_wtot[BLOCK / 64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (k >= m.L) return;                                   // sort_ind[k+1:end] is empty
  for (long long s = blockIdx.x; s < m.nseg; s += gridDim.x) {
    U prefix = 0, mask = 0;
    long long kk = k;
    if (k > 0) {
      for (int shift = BITS - 8; shift >= 0; shift -= 8) {
        hist[tid] = 0;                                    // BLOCK == 256 bins
        __syncthreads();
        for (long long t = tid; t < m.L; t += BLOCK) {
          const U key = abs_key(v[seg_addr(m, s, t)]);
          if ((key & mask) == prefix) atomicAdd(&hist[(unsigned)(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
          long long cum = 0;
          int b = 255;
          for (; b > 0; --b) {
            if (cum + hist[b] >= kk) break;
            cum += hist[b];
          }
          s_prefix = prefix | ((U)b << shift);
          s_kk = kk - cum;
        }
        __syncthreads();
        prefix = s_prefix;
        kk = s_kk;
        mask |= (U)255 << shift;
      }
    }
    // prefix = k-th largest magnitude, kk = how many entries equal to it survive (the earliest ones)
    if (tid == 0) s_run = 0;
    __syncthreads();
    for (long long c0 = 0; c0 < m.L; c0 += BLOCK) {
      const long long t = c0 + tid;
      const bool live = t < m.L;
      const long long addr = live ? seg_addr(m, s, t) : 0;
      const U key = live ? abs_key(v[addr]) : 0;
      const bool eq = live && k > 0 && key == prefix, gt = live && k > 0 && key > prefix;
      const unsigned long long bal = __ballot(eq);
      const unsigned rank = __popcll(bal & ((1ull << lane) - 1ull));
      if (lane == 0) s_wtot[w] = (unsigned)__popcll(bal);
      __syncthreads();
      long long off = s_run;
      for (int i = 0; i < w; ++i) off += s_wtot[i];
      const bool keep = gt || (eq && off + rank < kk);
      if (live && !keep) v[addr] = T(0);
      __syncthreads();
      if (tid == 0) {
        long long tot = 0;
        for (int i = 0; i < BLOCK / 64; ++i) tot += s_wtot[i];
        s_run += tot;
      }
      __syncthreads();
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Relaxed histogram (project_histogram_relaxed.jl:9-27): the j-th smallest entry is clipped to [LB[j], UB[j]].
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_hist_gather(SegMap m, const T* __restrict__ v, T* __restrict__ keys,
                                                       unsigned int* __restrict__ idx) {
  for (long long t = (long long)blockIdx.x * BLOCK + threadIdx.x; t < m.L; t += (long long)gridDim.x * BLOCK) {
    keys[t] = v[seg_addr(m, 0, t)];
    idx[t] = (unsigned int)t;
  }
}
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_hist_apply(SegMap m, const T* __restrict__ keys, const unsigned int* __restrict__ idx,
                                                      const T* __restrict__ lb, const T* __restrict__ ub, T* __restrict__ v) {
  for (long long j = (long long)blockIdx.x * BLOCK + threadIdx.x; j < m.L; j += (long long)gridDim.x * BLOCK) {
    T x = keys[j];
    x = x < ub[j] ? x : ub[j];              // min(x, UB) first, then max(LB, x)
    x = lb[j] > x ? lb[j] : x;
    v[seg_addr(m, 0, (long long)idx[j])] = x;
  }
}

// inverse of the r x r Gram matrix A'A in float64 (Gauss-Jordan, partial pivoting); A is L x r column-major
template <typename T>
static std::vector<double> gram_inverse(const T* A, long long L, int r) {
  std::vector<double> G((size_t)r * r, 0.0), I((size_t)r * r, 0.0);
  for (int i = 0; i < r; ++i)
    for (int j = i; j < r; ++j) {
      double acc = 0;
      const T *ai = A + (size_t)i * L, *aj = A + (size_t)j * L;
      for (long long k = 0; k < L; ++k) acc += (double)ai[k] * (double)aj[k];
      G[(size_t)i * r + j] = G[(size_t)j * r + i] = acc;
    }
  for (int i = 0; i < r; ++i) I[(size_t)i * r + i] = 1.0;
  for (int c = 0; c < r; ++c) {
    int piv = c;
    for (int i = c + 1; i < r; ++i)
      if (std::fabs(G[(size_t)i * r + c]) > std::fabs(G[(size_t)piv * r + c])) piv = i;
    if (G[(size_t)piv * r + c] == 0.0) throw std::runtime_error("subspace: the columns of A are linearly dependent");
    if (piv != c)
      for (int j = 0; j < r; ++j) {
        std::swap(G[(size_t)piv * r + j], G[(size_t)c * r + j]);
        std::swap(I[(size_t)piv * r + j], I[(size_t)c * r + j]);
      }
    const double d = 1.0 / G[(size_t)c * r + c];
    for (int j = 0; j < r; ++j) { G[(size_t)c * r + j] *= d; I[(size_t)c * r + j] *= d; }
    for (int i = 0; i < r; ++i) {
      if (i == c) continue;
      const double f = G[(size_t)i * r + c];
      if (f == 0.0) continue;
      for (int j = 0; j < r; ++j) { G[(size_t)i * r + j] -= f * G[(size_t)c * r + j]; I[(size_t)i * r + j] -= f * I[(size_t)c * r + j]; }
    }
  }
  return I;     // symmetric: row- and column-major coincide up to rounding; used as column-major below
}

template <typename T>
struct CardSegProj : ExtImpl<T> {
  SegMap map{};
  CardSegProj(const ExtSpec& spec, hipStream_t s) : ExtImpl<T>(spec, s) {
    if (spec.mode != SIPX_MODE_FIBER && spec.mode != SIPX_MODE_SLICE)
      throw std::runtime_error("segmented cardinality needs a fiber or slice mode");
    if (spec.ndim == 2 && spec.mode != SIPX_MODE_FIBER)
      throw std::runtime_error("for 2D models, the mode of application for project_cardinality! needs to be (fiber,x) or "
                               "(fiber,z). Or, provide the model as a vector");       // project_cardinality!.jl:57
    if (spec.pmax < 0) throw std::runtime_error("cardinality must be non-negative");
    map = make_segmap(spec);
  }
  void project(T* v, bool, double*, T*, T*) override {
    const long long nb = map.nseg < (long long)NB * 4 ? map.nseg : (long long)NB * 4;
    hipLaunchKernelGGL((k_seg_card<T>), dim3((unsigned)nb), dim3(BLOCK), 0, this->stream, map, v, (long long)this->sp.pmax);
    SIPX_HIP(hipGetLastError());
  }
};

// l1 ball, l2 ball or annulus of every fiber / slice (seg_norm.h): all segments share the scalar min / max, or -- built with
// ExtSpec::lb / ub -- each has its own (rmin / rmax, nseg entries in SegMap's order; one vector given for an annulus, the other one
// repeats its scalar).  Nothing is kept between calls: the call of the feasibility estimate and the one of the y update are
// independent, reset() has nothing to forget.
template <typename T>
struct NormSegProj : ExtImpl<T> {
  SegMap map{};
  SegNormPlan plan{};
  T *rmin = nullptr, *rmax = nullptr;
  NormSegProj(const ExtSpec& spec, hipStream_t s) : ExtImpl<T>(spec, s) {
    if (spec.mode != SIPX_MODE_FIBER && spec.mode != SIPX_MODE_SLICE)
      throw std::runtime_error("segmented l1 / l2 / annulus sets need a fiber or slice mode");
    if (spec.ndim == 2 && spec.mode != SIPX_MODE_FIBER)
      throw std::runtime_error("for 2D models, the mode of application for l1, l2 and annulus sets needs to be (fiber,x) or "
                               "(fiber,z), or matrix for the whole array");
    const bool vec = spec.ub || (spec.kind == EXT_ANNULUS_SEG && spec.lb);
    if (spec.kind == EXT_L1_SEG && !vec && !((T)spec.pmax > T(0))) throw std::runtime_error("Radius of L1 ball is negative");   // project_l1_Duchi!.jl:22
    map = make_segmap(spec);
    if (map.nseg < 1 || map.L < 1 || map.L >= (1ll << 31)) throw std::runtime_error("segmented l1 / l2 / annulus sets: empty or oversize segments");
    plan = seg_norm_plan(map, (int)sizeof(T));
    if (!vec) return;
    auto fill = [&](const void* host, double scalar) {
      std::vector<T> h((size_t)map.nseg, (T)scalar);
      if (host) h.assign((const T*)host, (const T*)host + map.nseg);
      if (spec.kind == EXT_L1_SEG)
        for (T r : h)
          if (!(r > T(0))) throw std::runtime_error("Radius of L1 ball is negative");
      T* d = this->template alloc<T>((size_t)map.nseg);
      SIPX_HIP(hipMemcpy(d, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice));
      return d;
    };
    rmax = fill(spec.ub, spec.pmax);
    if (spec.kind == EXT_ANNULUS_SEG) rmin = fill(spec.lb, spec.pmin);
  }
  template <int KIND>
  void launch(T* v) {
    if (rmax)
      hipLaunchKernelGGL((k_seg_norm<T, KIND, true>), dim3(plan.grid), dim3(BLOCK), plan.lds_bytes, this->stream, map, plan, v,
                         (T)this->sp.pmin, (T)this->sp.pmax, rmin, rmax);
    else
      hipLaunchKernelGGL((k_seg_norm<T, KIND, false>), dim3(plan.grid), dim3(BLOCK), plan.lds_bytes, this->stream, map, plan, v,
                         (T)this->sp.pmin, (T)this->sp.pmax, (const T*)nullptr, (const T*)nullptr);
  }
  void project(T* v, bool, double*, T*, T*) override {
    if (this->sp.kind == EXT_L1_SEG) launch<SEGN_L1>(v);
    else if (this->sp.kind == EXT_L2_SEG) launch<SEGN_L2>(v);
    else launch<SEGN_ANNULUS>(v);
    SIPX_HIP(hipGetLastError());
  }
  // new radii into the arrays of the old ones: one copy each on the set's stream (lb: the annulus' inner radii)
  void set_data(const T* new_lb, const T* new_ub, bool on_device) override {
    if (!rmax) ExtImpl<T>::set_data(new_lb, new_ub, on_device);
    if (new_lb && !rmin) throw std::runtime_error("only the annulus has inner radii: pass the radii of this set as ub");
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const size_t bytes = sizeof(T) * (size_t)map.nseg;
    if (new_lb) SIPX_HIP(hipMemcpyAsync(rmin, new_lb, bytes, kind, this->stream));
    if (new_ub) SIPX_HIP(hipMemcpyAsync(rmax, new_ub, bytes, kind, this->stream));
  }
};

// The norms of the fibers / slices of a materialised vector (sipx_segment_norms): one launch of k_seg_observe with the projector's
// own tile mapping, nothing resident.
template <typename T>
void seg_observe(const ExtSpec& spec, int norm_l2, const T* v, T* out, hipStream_t stream) {
  if (spec.mode != SIPX_MODE_FIBER && spec.mode != SIPX_MODE_SLICE) throw std::runtime_error("segment norms need a fiber or slice mode");
  if (spec.ndim == 2 && spec.mode != SIPX_MODE_FIBER)
    throw std::runtime_error("for 2D models, the mode of application for l1, l2 and annulus sets needs to be (fiber,x) or "
                             "(fiber,z), or matrix for the whole array");
  const SegMap map = make_segmap(spec);
  if (map.nseg < 1 || map.L < 1 || map.L >= (1ll << 31)) throw std::runtime_error("segment norms: empty or oversize segments");
  SegNormPlan plan = seg_norm_plan(map, (int)sizeof(T));
  plan.lds = 0;
  plan.lds_bytes = 0;
  if (norm_l2) hipLaunchKernelGGL((k_seg_observe<T, SEGN_L2>), dim3(plan.grid), dim3(BLOCK), 0, stream, map, plan, v, out);
  else hipLaunchKernelGGL((k_seg_observe<T, SEGN_L1>), dim3(plan.grid), dim3(BLOCK), 0, stream, map, plan, v, out);
  SIPX_HIP(hipGetLastError());
}
template void seg_observe<float>(const ExtSpec&, int, const float*, float*, hipStream_t);
template void seg_observe<double>(const ExtSpec&, int, const double*, double*, hipStream_t);

// The simplex of every fiber / slice (seg_simplex.h): nonnegative entries with a sum in [pmin, pmax], one pair of scalars for all
// segments.  Short fibers with contiguous neighbours go through the lane route, one lane a segment; everything else through the tile
// mapping of the norm sets.  Nothing is kept between calls; the counters are for sipx_kernel_stats.
template <typename T>
struct SimplexSegProj : ExtImpl<T> {
  SegMap map{};
  SegNormPlan plan{};
  int bucket = 0;                     // simplex_lane_bucket: 0: the tile route
  long long nchunk = 0, ntile = 0;    // lane route: tiles of 64 segments a row, in all
  unsigned lane_grid = 1;
  long long calls = 0;
  SimplexSegProj(const ExtSpec& spec, hipStream_t s) : ExtImpl<T>(spec, s) {
    if (spec.mode != SIPX_MODE_FIBER && spec.mode != SIPX_MODE_SLICE) throw std::runtime_error(SIMPLEX_NEEDS_MODE);
    if (spec.ndim == 2 && spec.mode != SIPX_MODE_FIBER) throw std::runtime_error(SIMPLEX_2D_SLICE);
    if (spec.lb || spec.ub) throw std::runtime_error(SIMPLEX_NO_VECTORS);
    simplex_check_bounds<T>(spec.pmin, spec.pmax);
    map = make_segmap(spec);
    if (map.nseg < 1 || map.L < 1 || map.L >= (1ll << 31)) throw std::runtime_error("simplex sets: empty or oversize segments");
    plan = seg_norm_plan(map, (int)sizeof(T));
    bucket = simplex_lane_bucket(map);
    nchunk = (map.SA + 63) / 64;
    ntile = nchunk * (map.nseg / map.SA);
    const long long nb = (ntile + BLOCK / 64 - 1) / (BLOCK / 64);
    lane_grid = (unsigned)(nb < SEGN_MAX_GRID ? (nb < 1 ? 1 : nb) : SEGN_MAX_GRID);
  }
  template <int LB, bool OBS>
  void lane(T* v, T* out) {
    hipLaunchKernelGGL((k_simplex_lane<T, LB, OBS>), dim3(lane_grid), dim3(BLOCK), 0, this->stream, map, nchunk, ntile, v,
                       (T)this->sp.pmin, (T)this->sp.pmax, out);
  }
  template <bool OBS>
  void launch(T* v, T* out) {
    if (bucket == 4) lane<4, OBS>(v, out);
    else if (bucket == 8) lane<8, OBS>(v, out);
    else if (bucket == 16) lane<16, OBS>(v, out);
    else
      hipLaunchKernelGGL((k_simplex_tile<T, OBS>), dim3(plan.grid), dim3(BLOCK), OBS ? 0u : plan.lds_bytes, this->stream, map, plan, v,
                         (T)this->sp.pmin, (T)this->sp.pmax, out);
    SIPX_HIP(hipGetLastError());
  }
  void project(T* v, bool, double*, T*, T*) override {
    ++calls;
    launch<false>(v, (T*)nullptr);
  }
  // out[s] <- (T)spos of segment s (nseg entries): pass 1 of the projector's own route; v is not written
  void observe(const T* v, T* out, double*, T*, T*) override { launch<true>(const_cast<T*>(v), out); }
  void reset() override { calls = 0; }
  // calls, those of the lane route, those of the tile route, the segments
  void route_counts(long long out[4]) const override {
    out[0] = calls; out[1] = bucket ? calls : 0; out[2] = bucket ? 0 : calls; out[3] = map.nseg;
  }
};

template <typename T>
struct HistogramProj : ExtImpl<T> {
  SegMap map{};
  T *keys_in = nullptr, *keys_out = nullptr, *lb = nullptr, *ub = nullptr;
  unsigned int *idx_in = nullptr, *idx_out = nullptr;
  void* sort_tmp = nullptr;
  size_t sort_bytes = 0;
  HistogramProj(const ExtSpec& spec, hipStream_t s) : ExtImpl<T>(spec, s) {
    if (spec.mode != SIPX_MODE_WHOLE) throw std::runtime_error("histogram constraints act on the whole vector");
    if (!spec.lb || !spec.ub) throw std::runtime_error("histogram constraints need sorted lb and ub vectors");
    map = make_segmap(spec);
    const long long M = map.L;
    keys_in = this->template alloc<T>(M); keys_out = this->template alloc<T>(M);
    idx_in = this->template alloc<unsigned int>(M); idx_out = this->template alloc<unsigned int>(M);
    lb = this->template alloc<T>(M); ub = this->template alloc<T>(M);
    SIPX_HIP(hipMemcpy(lb, spec.lb, sizeof(T) * M, hipMemcpyHostToDevice));
    SIPX_HIP(hipMemcpy(ub, spec.ub, sizeof(T) * M, hipMemcpyHostToDevice));
    SIPX_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, keys_in, keys_out, idx_in, idx_out, (int)M, 0, (int)sizeof(T) * 8, s));
    sort_tmp = this->template alloc<char>(sort_bytes);
  }
  void project(T* v, bool, double*, T*, T*) override {
    hipStream_t s = this->stream;
    hipLaunchKernelGGL((k_hist_gather<T>), dim3(NB), dim3(BLOCK), 0, s, map, v, keys_in, idx_in);
    SIPX_HIP(hipcub::DeviceRadixSort::SortPairs(sort_tmp, sort_bytes, keys_in, keys_out, idx_in, idx_out, (int)map.L, 0, (int)sizeof(T) * 8, s));
    hipLaunchKernelGGL((k_hist_apply<T>), dim3(NB), dim3(BLOCK), 0, s, map, keys_out, idx_out, lb, ub, v);
    SIPX_HIP(hipGetLastError());
  }
  // new bound vectors into the arrays of the old ones: one copy each, behind whatever the stream still does with them
  void set_data(const T* new_lb, const T* new_ub, bool on_device) override {
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const size_t bytes = sizeof(T) * (size_t)map.L;
    if (new_lb) SIPX_HIP(hipMemcpyAsync(lb, new_lb, bytes, kind, this->stream));
    if (new_ub) SIPX_HIP(hipMemcpyAsync(ub, new_ub, bytes, kind, this->stream));
  }
};

// x .= A*(A'*x)  or  A*((A'*A)\(A'*x))   project_subspace!.jl:15-19
template <typename T>
struct SubspaceProj : ExtImpl<T> {
  SegMap map{};
  BlasHandle blas;
  T *basis = nullptr, *gram_inv = nullptr, *X = nullptr, *t1 = nullptr, *t2 = nullptr;
  int cols = 0;
  SubspaceProj(const ExtSpec& spec, hipStream_t s) : ExtImpl<T>(spec, s) {
    if (spec.ndim == 2 && spec.mode == SIPX_MODE_SLICE) throw std::runtime_error("mode[1] for project_subspace! must be: fiber");
    if (spec.ndim == 3 && spec.mode == SIPX_MODE_FIBER)
      throw std::runtime_error("for 3D models, the mode of application for project_subspace! needs to be (slice,x) or "
                               "(slice,y) or (slice,z)");                              // project_subspace!.jl:121
    map = make_segmap(spec);
    if (!spec.basis || spec.basis_cols < 1) throw std::runtime_error("subspace constraints need the matrix A");
    if (spec.basis_rows != map.L) throw std::runtime_error("subspace: rows of A do not match the length of what it projects");
    cols = spec.basis_cols;
    const long long L = map.L;
    basis = this->template alloc<T>((size_t)L * cols);
    SIPX_HIP(hipMemcpy(basis, spec.basis, sizeof(T) * (size_t)L * cols, hipMemcpyHostToDevice));
    if (!spec.basis_orth) {
      std::vector<double> Gi = gram_inverse<T>((const T*)spec.basis, L, cols);
      std::vector<T> Gt(Gi.begin(), Gi.end());
      gram_inv = this->template alloc<T>((size_t)cols * cols);
      SIPX_HIP(hipMemcpy(gram_inv, Gt.data(), sizeof(T) * Gt.size(), hipMemcpyHostToDevice));
    }
    X = this->template alloc<T>((size_t)L * map.nseg);
    t1 = this->template alloc<T>((size_t)cols * map.nseg);
    t2 = this->template alloc<T>((size_t)cols * map.nseg);
    blas.create(s);
  }
  void project(T* v, bool, double*, T*, T*) override {
    hipStream_t s = this->stream;
    const auto N_ = rocblas_operation_none, T_ = rocblas_operation_transpose;
    const int L = (int)map.L, ns = (int)map.nseg, r = cols;
    hipLaunchKernelGGL((k_seg_gather<T, T>), dim3(NB), dim3(BLOCK), 0, s, map, v, X);
    blas_check(gemm_T(blas, T_, N_, r, ns, L, basis, L, X, L, t1, r), "gemm A'x");
    T* t = t1;
    if (gram_inv) {
      blas_check(gemm_T(blas, N_, N_, r, ns, r, gram_inv, r, t1, r, t2, r), "gemm G t");
      t = t2;
    }
    blas_check(gemm_T(blas, N_, N_, L, ns, r, basis, L, t, r, X, L), "gemm A t");
    hipLaunchKernelGGL((k_seg_scatter<T, T>), dim3(NB), dim3(BLOCK), 0, s, map, X, v, (const int*)nullptr);
    SIPX_HIP(hipGetLastError());
  }
  void set_stream(hipStream_t s) override {
    if (this->stream == s) return;
    this->stream = s;
    blas.set_stream(s);
  }
};

template <typename T>
ExtImpl<T>* make_segment_family(const ExtSpec& spec, hipStream_t stream) {
  if (spec.kind == EXT_CARD_SEG) return new CardSegProj<T>(spec, stream);
  if (spec.kind == EXT_L1_SEG || spec.kind == EXT_L2_SEG || spec.kind == EXT_ANNULUS_SEG) return new NormSegProj<T>(spec, stream);
  if (spec.kind == EXT_SIMPLEX_SEG) return new SimplexSegProj<T>(spec, stream);
  if (spec.kind == EXT_HISTOGRAM) return new HistogramProj<T>(spec, stream);
  return new SubspaceProj<T>(spec, stream);
}
template ExtImpl<float>* make_segment_family<float>(const ExtSpec&, hipStream_t);
template ExtImpl<double>* make_segment_family<double>(const ExtSpec&, hipStream_t);

}  // namespace sipx
