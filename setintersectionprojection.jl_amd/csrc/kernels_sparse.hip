// Matrix-free term of Q: the two products of a caller-supplied sparse operator whose A'A is not kept as CDS bands
// (the reference keeps such a Q sparse: PARSDMM_precompute_distribute.jl:51-59, argmin_x.jl:42-51).
//   k_mf_fwd:  t = A p            over the CSR copy
//   k_mf_adj:  out += alpha A' w   over the CSC arrays, optionally with the block partials of a dot product of the result
// 32-bit indices.  A row (column) of the compressed view belongs to a power-of-two group of G lanes, G = 1 .. 64 chosen per
// view from its row lengths: lane g of the group takes the entries g, g + G, g + 2G, ... of the row, so one wave reads
// values and indices as contiguous runs; rows longer than the group are walked in strides of the group.  The sum of a row is
// taken in that fixed order inside a lane and through a fixed xor tree across the group (both operands of every node are
// exchanged, so every lane of the group ends with the same bits); nothing is accumulated with atomics: two runs give the
// same bits.  Sums are in the working precision, products unfused like everywhere else in this library.
#include <stdexcept>
#include <string>

#include "sipx_device.h"

namespace sipx {

template <typename T, int G>
__device__ __forceinline__ T group_sum(T v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
  return v;
}

template <typename T, int G>
__global__ __launch_bounds__(BLOCK) void k_mf_fwd(MfOp<T> A, const T* __restrict__ x, T* __restrict__ out,
                                                  const int* __restrict__ done) {
  if (done && *done) return;
  constexpr int RPB = BLOCK / G;                  // rows a workgroup takes per step
  const unsigned g = threadIdx.x & (G - 1);
  const int q = threadIdx.x / G;
  // (the step is uniform over the workgroup: every lane of a wave reaches the exchange of group_sum)
  for (long long rb = (long long)blockIdx.x * RPB; rb < A.rows; rb += (long long)gridDim.x * RPB) {
    const long long r = rb + q;
    const bool ok = r < A.rows;
    const unsigned k0 = ok ? (unsigned)A.ptr[r] : 0u, k1 = ok ? (unsigned)A.ptr[r + 1] : 0u;
    T acc = T(0);
    for (unsigned k = k0 + g; k < k1; k += G) acc = acc + A.val[k] * x[A.idx[k]];
    acc = group_sum<T, G>(acc);
    if (ok && g == 0) out[r] = acc;
  }
}

template <typename T, int G>
__global__ __launch_bounds__(BLOCK) void k_mf_adj(MfOp<T> A, MfAdj<T> a) {
  if (a.done && *a.done) return;
  constexpr int RPB = BLOCK / G;
  const unsigned g = threadIdx.x & (G - 1);
  const int q = threadIdx.x / G;
  double acc = 0;
  for (long long rb = (long long)blockIdx.x * RPB; rb < A.rows; rb += (long long)gridDim.x * RPB) {
    const long long j = rb + q;
    const bool ok = j < A.rows;
    const unsigned k0 = ok ? (unsigned)A.ptr[j] : 0u, k1 = ok ? (unsigned)A.ptr[j + 1] : 0u;
    T t = T(0);
    if (a.in_mode == 0) {
      for (unsigned k = k0 + g; k < k1; k += G) t = t + A.val[k] * a.y[A.idx[k]];
    } else {
      for (unsigned k = k0 + g; k < k1; k += G) {
        const int r = A.idx[k];
        t = t + A.val[k] * (a.rho * a.y[r] + a.l[r]);
      }
    }
    t = group_sum<T, G>(t);
    if (ok && g == 0) {
      T v = t;
      if (a.out) {
        v = a.out[j] + a.alpha * t;
        a.out[j] = v;
      }
      if (a.dot == 1) acc += (double)a.p[j] * (double)v;
      else if (a.dot == 2) acc += (double)v * (double)v;
    }
  }
  if (a.dot) {
    double ac[1] = {acc};
    block_reduce_store<1>(ac, a.partials, a.slot);
  }
}

// workgroups of a launch: one group of `lanes` per row, no more than the partial arrays hold
static inline int mf_grid(int rows, int lanes) { return fit_grid((long long)rows * lanes, NB); }

template <typename T>
static inline double mf_bytes(const MfOp<T>& A, double vectors) {      // nnz (w + 4) for values and indices, the row pointers, the vectors
  return (double)A.nnz * (sizeof(T) + 4.0) + 4.0 * ((double)A.rows + 1.0) + vectors * sizeof(T);
}

#define SIPX_MF_DISPATCH(KERNEL, ...)                                                                                  \
  switch (A.lanes) {                                                                                                   \
    case 1: hipLaunchKernelGGL((KERNEL<T, 1>), dim3(nb), dim3(BLOCK), 0, s, __VA_ARGS__); break;                       \
    case 2: hipLaunchKernelGGL((KERNEL<T, 2>), dim3(nb), dim3(BLOCK), 0, s, __VA_ARGS__); break;                       \
    case 4: hipLaunchKernelGGL((KERNEL<T, 4>), dim3(nb), dim3(BLOCK), 0, s, __VA_ARGS__); break;                       \
    case 8: hipLaunchKernelGGL((KERNEL<T, 8>), dim3(nb), dim3(BLOCK), 0, s, __VA_ARGS__); break;                       \
    case 16: hipLaunchKernelGGL((KERNEL<T, 16>), dim3(nb), dim3(BLOCK), 0, s, __VA_ARGS__); break;                     \
    case 32: hipLaunchKernelGGL((KERNEL<T, 32>), dim3(nb), dim3(BLOCK), 0, s, __VA_ARGS__); break;                     \
    case 64: hipLaunchKernelGGL((KERNEL<T, 64>), dim3(nb), dim3(BLOCK), 0, s, __VA_ARGS__); break;                     \
    default: throw std::runtime_error("matrix-free operator: the lane group must be a power of two from 1 to 64");     \
  }

template <typename T>
void K<T>::mf_fwd(hipStream_t s, const MfOp<T>& A, const T* x, T* out, const int* done) {
  // (the gathered vector is read nnz times through the caches; booked once per distinct row of it at most: rows entries)
  ObsScope obs(KID_MF_FWD, s, mf_bytes(A, 2.0 * A.rows));
  const int nb = mf_grid(A.rows, A.lanes);
  SIPX_MF_DISPATCH(k_mf_fwd, A, x, out, done)
  SIPX_HIP(hipGetLastError());
}

template <typename T>
void K<T>::mf_adj(hipStream_t s, const MfOp<T>& A, const MfAdj<T>& a) {
  ObsScope obs(KID_MF_ADJ, s, mf_bytes(A, (a.out ? 3.0 : 1.0) * A.rows + (a.dot == 1 ? A.rows : 0.0) + (a.in_mode ? A.rows : 0.0)));
  const int nb = mf_grid(A.rows, A.lanes);
  SIPX_MF_DISPATCH(k_mf_adj, A, a)
  SIPX_HIP(hipGetLastError());
}

template void K<float>::mf_fwd(hipStream_t, const MfOp<float>&, const float*, float*, const int*);
template void K<double>::mf_fwd(hipStream_t, const MfOp<double>&, const double*, double*, const int*);
template void K<float>::mf_adj(hipStream_t, const MfOp<float>&, const MfAdj<float>&);
template void K<double>::mf_adj(hipStream_t, const MfOp<double>&, const MfAdj<double>&);

}  // namespace sipx
