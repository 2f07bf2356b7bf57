// Orthonormal periodic multilevel separable DWT with the Daubechies filter of 4 vanishing moments (db4, 8 taps) on 2-D and
// 3-D grids: the transform behind TD_OP = "wavelet" (joDWT(n1, n2, wavelet(WT.db4); L = maxtransformlevels(min(n))),
// reference src/get_TD_operator.jl:86-88).  Convention (sipx.h, SIPX_TRANSFORM_WAVELET): one level along an axis of length m
//   a[k] = sum_j lo[j] x[(2k + 4 - j) mod m],  d[k] = sum_j hi[j] x[(2k + 4 - j) mod m],  k < m/2,
// a to [0, m/2), d to [m/2, m); level l transforms every axis of the box n / 2^(l-1), in place in the array (Mallat layout).
// See kernels_dwt.hip.
#pragma once
#include "sipx_common.h"

namespace sipx {

// L: the largest integer with 2^L dividing min(n) over the ndim leading dimensions (maxtransformlevels); 0 = identity
int dwt_levels(int ndim, const long long* n);
// throws, naming the grid, unless ndim is 2 or 3 and every dimension is divisible by 2^L
void dwt_check_grid(int ndim, const long long* n);

// out <- W in.  in and out are distinct device arrays of prod(n) entries (column-major, dim 0 fastest); scratch holds
// prod(n) entries.  Deterministic: no atomics.
template <typename T>
void dwt_forward(hipStream_t s, int ndim, const long long* n, const T* in, T* out, T* scratch);

// out <- W' in.  in is CLOBBERED (used as a work array); in, out and scratch are distinct.  With gate != nullptr every launch
// returns at once when gate->need == 0, so out keeps its bits (the l1 ball behind the transform, inside the ball).
template <typename T>
void dwt_inverse(hipStream_t s, int ndim, const long long* n, T* in, T* out, T* scratch, const ProjScalars<T>* gate = nullptr);

}  // namespace sipx
