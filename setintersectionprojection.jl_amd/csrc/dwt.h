// Orthonormal periodic multilevel separable DWT with the Daubechies filter of 4 vanishing moments (db4, 8 taps) on 2-D and
// 3-D grids: the transform behind TD_OP = "wavelet" (joDWT(n1, n2, wavelet(WT.db4); L = maxtransformlevels(min(n))),
// reference src/get_TD_operator.jl:86-88).  Convention (sipx.h, SIPX_TRANSFORM_WAVELET): one level along an axis of length m
//   a[k] = sum_j lo[j] x[(2k + 4 - j) mod m],  d[k] = sum_j hi[j] x[(2k + 4 - j) mod m],  k < m/2,
// a to [0, m/2), d to [m/2, m); level l transforms every axis of the box n / 2^(l-1), in place in the array (Mallat layout).
// See kernels_dwt.hip.
#pragma once
#include <stdexcept>
#include <string>

#include "sipx_common.h"

namespace sipx {

// L: the largest integer with 2^L dividing min(n) over the ndim leading dimensions (maxtransformlevels); 0 = identity
inline int dwt_levels(int ndim, const long long* n) {
  long long m = n[0];
  for (int a = 1; a < ndim; ++a) m = n[a] < m ? n[a] : m;
  int L = 0;
  while (m > 0 && m % 2 == 0) { m /= 2; ++L; }
  return L;
}
// throws, naming the grid, unless ndim is 2 or 3 and every dimension is divisible by 2^L
inline void dwt_check_grid(int ndim, const long long* n) {
  if (ndim != 2 && ndim != 3) throw std::runtime_error("wavelet transform: 2-D and 3-D grids only");
  const long long n2 = ndim == 3 ? n[2] : 1;
  if (n[0] < 1 || n[1] < 1 || n2 < 1) throw std::runtime_error("wavelet transform: empty grid");
  if (n[0] * n[1] * n2 >= (1LL << 31)) throw std::runtime_error("wavelet transform: grids of 2^31 points and more are not supported");
  const int L = dwt_levels(ndim, n);
  for (int a = 0; a < ndim; ++a)
    if (n[a] % (1LL << L) != 0) {
      std::string g = std::to_string(n[0]);
      for (int q = 1; q < ndim; ++q) g += " x " + std::to_string(n[q]);
      throw std::runtime_error("wavelet transform: the grid " + g + " has " + std::to_string(L) + " levels (2^L divides the smallest "
                               "dimension) but dimension " + std::to_string(a + 1) + " is not divisible by 2^" + std::to_string(L));
    }
}

// out <- W in.  in and out are distinct device arrays of prod(n) entries (column-major, dim 0 fastest); scratch holds
// prod(n) entries.  Deterministic: no atomics.
template <typename T>
void dwt_forward(hipStream_t s, int ndim, const long long* n, const T* in, T* out, T* scratch);

// out <- W' in.  in is CLOBBERED (used as a work array); in, out and scratch are distinct.  With gate != nullptr every launch
// returns at once when gate->need == 0, so out keeps its bits (the l1 ball behind the transform, inside the ball).
template <typename T>
void dwt_inverse(hipStream_t s, int ndim, const long long* n, T* in, T* out, T* scratch, const ProjScalars<T>* gate = nullptr);

}  // namespace sipx
