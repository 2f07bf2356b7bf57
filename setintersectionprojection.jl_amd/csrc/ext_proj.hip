// Projectors that lean on a library (hipFFT, rocSOLVER / rocBLAS, hipCUB) or select per fiber / slice: they act on a materialised
// vector v (N reals).  ExtProj<T> picks the family of spec.kind and forwards to it (ext_family.h):
//   ext_transform.hip  DFT mask, l1 and cardinality behind the DFT, DCT, DWT
//   ext_rank.hip       slice / matrix rank, nuclear norm
//   ext_segments.hip   cardinality, l1, l2, annulus and the simplex per fiber / slice, relaxed histogram, subspace
//   ext_group.hip      the l2,1 ball across the blocks of the TV / TV_xy operator, whole array, per z-slice or jointly across the frames;
//                      the l2,1 ball over the fibers or slices of a one-block operator's range and group cardinality on the same segments; the l2,0 sets on the groups of TV / TV_xy; the weighted l1 ball on the rows of an operator
#include "ext_family.h"

namespace sipx {

// sum (a-b)^2 and sum b^2 into partial slots 0,1
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_dist2(long long N, const T* __restrict__ a, const T* __restrict__ b,
                                                 double* __restrict__ partials) {
  double acc[2] = {0, 0};
  for (long long e = (long long)blockIdx.x * BLOCK + threadIdx.x; e < N; e += (long long)gridDim.x * BLOCK) {
    const T d = a[e] - b[e];
    acc[0] += (double)d * (double)d;
    acc[1] += (double)b[e] * (double)b[e];
  }
  block_reduce_store<2>(acc, partials, 0);
}
template <typename T>
void ext_dist2(hipStream_t s, long long N, const T* projected, const T* original, double* dst) {
  hipLaunchKernelGGL((k_dist2<T>), dim3(NB), dim3(BLOCK), 0, s, N, projected, original, dst);
  SIPX_HIP(hipGetLastError());
}

template <typename T>
ExtProj<T>::ExtProj(const ExtSpec& spec, hipStream_t stream) : impl_(nullptr) {
  switch (spec.kind) {
    case EXT_DFT_MASK: case EXT_L1_DFT: case EXT_CARD_DFT: case EXT_DCT: case EXT_DWT: impl_ = make_transform_family<T>(spec, stream); break;
    case EXT_RANK: case EXT_NUCLEAR: impl_ = make_rank_family<T>(spec, stream); break;
    case EXT_CARD_SEG: case EXT_L1_SEG: case EXT_L2_SEG: case EXT_ANNULUS_SEG: case EXT_SIMPLEX_SEG: case EXT_HISTOGRAM: case EXT_SUBSPACE:
      impl_ = make_segment_family<T>(spec, stream); break;
    case EXT_L21: case EXT_L21_SEG: case EXT_L21_JOINT: case EXT_L21_GROUPS: case EXT_CARD_GROUPS: case EXT_L20: case EXT_L20_SEG: case EXT_L20_JOINT: case EXT_TNV: case EXT_L1_WEIGHTED: case EXT_L21_STACKED: case EXT_L2INF: case EXT_L2INF_JOINT: case EXT_L2INF_STACKED: impl_ = make_group_family<T>(spec, stream); break;
    default: throw std::runtime_error("unknown external projector");
  }
}
template <typename T>
ExtProj<T>::~ExtProj() {
  delete impl_;
  impl_ = nullptr;
}

// v <- P(v) in place.  `feas` selects the independent warm-start state used for the feasibility estimate.
template <typename T>
void ExtProj<T>::project(T* v, bool feas, double* partials, T* maxpart, T* compact) {
  impl_->project(v, feas, partials, maxpart, compact);
}
template <typename T>
void ExtProj<T>::observe(const T* v, T* out, double* partials, T* maxpart, T* compact) {
  impl_->observe(v, out, partials, maxpart, compact);
}
template <typename T>
void ExtProj<T>::set_stream(hipStream_t s) { impl_->set_stream(s); }
// Back to the state of a freshly built projector (sipx_reset): no warm start of any kind, no pending status, counters at zero.
// A reused context then walks through exactly the calls of a new one -- same bits -- without its allocations, plans and handles.
template <typename T>
void ExtProj<T>::reset() { if (impl_) impl_->reset(); }
template <typename T>
void ExtProj<T>::set_data(const T* lb, const T* ub, bool on_device) {
  if (!impl_) throw std::runtime_error("this projector holds no replaceable vectors (build a new context)");
  impl_->set_data(lb, ub, on_device);
}
template <typename T>
long long ExtProj<T>::device_bytes() const { return impl_ ? impl_->mem.bytes() : 0; }
template <typename T>
void ExtProj<T>::route_counts(long long out[4]) const {
  out[0] = out[1] = out[2] = out[3] = 0;
  if (impl_) impl_->route_counts(out);
}

template class ExtProj<float>;
template class ExtProj<double>;
template void ext_dist2<float>(hipStream_t, long long, const float*, const float*, double*);
template void ext_dist2<double>(hipStream_t, long long, const double*, const double*, double*);

}  // namespace sipx
