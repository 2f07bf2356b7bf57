// db4 wavelet transform (dwt.h): one axis of one level per launch while the box is large, all remaining levels and axes of a
// small box in one workgroup through LDS.  Memory-bound: a level reads and writes its box once per axis.
//
// Axis passes.  Along the contiguous axis lanes take consecutive runs of RC outputs, so the reads of a wave and the two
// output halves are contiguous.  Along a strided axis lanes run along dim 0 (every tap is a coalesced row) and each thread
// walks a run of RS consecutive outputs with a sliding register window of the 8 taps (forward) or of the 5 + 5 coefficients
// (inverse): every input is loaded once per thread, not four times.  Indices wrap modulo the axis length m, also where m
// (2 or 4 at the deepest levels) is shorter than the filter.
//
// Buffers (n = prod(dims)).  Forward, level 1: in -> out -> scratch -> out (3-D) or in -> scratch -> out (2-D); levels >= 2
// work on the leading box of out through two compact boxes at the front of scratch (box <= n/8 in 3-D, n/4 in 2-D).
// Inverse, levels >= 2 in place on in (the same compact boxes), level 1: in -> scratch -> in -> out (3-D) or
// in -> scratch -> out (2-D): out is written by the last launch only.
#include <stdexcept>
#include <string>

#include "dwt.h"

namespace sipx {

namespace {

// db4 decomposition low-pass (orthonormal, sum = sqrt(2)); hi[j] = (-1)^(j+1) lo[7-j]
__host__ __device__ constexpr double db4_lo(int j) {
  return j == 0 ? -0.010597401785069032 : j == 1 ? 0.0328830116668852 : j == 2 ? 0.030841381835560764 :
         j == 3 ? -0.18703481171909309 : j == 4 ? -0.027983769416859854 : j == 5 ? 0.6308807679298589 :
         j == 6 ? 0.7148465705529157 : 0.2303778133088965;
}
__host__ __device__ constexpr double db4_hi(int j) { return (j & 1) ? db4_lo(7 - j) : -db4_lo(7 - j); }

constexpr int RC = 2;           // outputs per thread along the contiguous axis
constexpr int RS = 8;           // outputs per thread along a strided axis
constexpr int SMALL = 4096;     // boxes of at most this many entries: every remaining level in one workgroup (16^3, 64^2)
constexpr int SMALL_BLOCK = 256;

__host__ __device__ inline int wrap(long long p, int m) {
  long long r = p % m;
  return (int)(r < 0 ? r + m : r);
}

// forward, one line: outputs k0 .. k0+cnt-1 of a line of length m (src / dst point at its element 0, sst / dstd the strides)
template <typename T, int R>
__host__ __device__ __forceinline__ void fwd_run(const T* src, long long sst, T* dst, long long dstd, int m, int k0, int cnt) {
  const int h = m >> 1;
  int p = wrap(2LL * k0 - 3, m);
  T w[8];                                   // w[q] = x[2k - 3 + q]:  a[k] = sum_q lo[7-q] w[q]
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    w[q] = src[p * sst];
    p = p + 1 == m ? 0 : p + 1;
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (r < cnt) {
      T a = T(0), d = T(0);
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        a += (T)db4_lo(7 - q) * w[q];
        d += (T)db4_hi(7 - q) * w[q];
      }
      dst[(long long)(k0 + r) * dstd] = a;
      dst[(long long)(h + k0 + r) * dstd] = d;
      if (r + 1 < cnt) {
#pragma unroll
        for (int q = 0; q < 6; ++q) w[q] = w[q + 2];
        w[6] = src[p * sst];
        p = p + 1 == m ? 0 : p + 1;
        w[7] = src[p * sst];
        p = p + 1 == m ? 0 : p + 1;
      }
    }
  }
}

// inverse (the transpose), one line: output pairs x[2p], x[2p+1] for p = p0 .. p0+cnt-1 from a[p-2 .. p+2], d[p-2 .. p+2]
template <typename T, int R>
__host__ __device__ __forceinline__ void inv_run(const T* src, long long sst, T* dst, long long dstd, int m, int p0, int cnt) {
  const int h = m >> 1;
  int q = wrap((long long)p0 - 2, h);
  T A[5], D[5];
#pragma unroll
  for (int u = 0; u < 5; ++u) {
    A[u] = src[(long long)q * sst];
    D[u] = src[(long long)(h + q) * sst];
    q = q + 1 == h ? 0 : q + 1;
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (r < cnt) {
      // x[2p] collects the even taps (k = p-2+j/2), x[2p+1] the odd ones (k = p+(j-3)/2)
      T x0 = T(0), x1 = T(0);
#pragma unroll
      for (int u = 0; u < 4; ++u) x0 += (T)db4_lo(2 * u) * A[u];
#pragma unroll
      for (int u = 0; u < 4; ++u) x0 += (T)db4_hi(2 * u) * D[u];
#pragma unroll
      for (int u = 0; u < 4; ++u) x1 += (T)db4_lo(2 * u + 1) * A[u + 1];
#pragma unroll
      for (int u = 0; u < 4; ++u) x1 += (T)db4_hi(2 * u + 1) * D[u + 1];
      dst[(long long)(2 * (p0 + r)) * dstd] = x0;
      dst[(long long)(2 * (p0 + r) + 1) * dstd] = x1;
      if (r + 1 < cnt) {
#pragma unroll
        for (int u = 0; u < 4; ++u) { A[u] = A[u + 1]; D[u] = D[u + 1]; }
        A[4] = src[(long long)q * sst];
        D[4] = src[(long long)(h + q) * sst];
        q = q + 1 == h ? 0 : q + 1;
      }
    }
  }
}

// One axis of one level on the box b of src (strides 1, s1, s2) into dst (strides 1, d1, d2).
struct PassArgs {
  long long s1, s2, d1, d2;
  int b0, b1, b2, axis;
};

// work items of a pass: runs of R outputs per line, lines of the box
template <int R>
__host__ __device__ inline unsigned pass_items(const PassArgs& a) {
  const int m = a.axis == 0 ? a.b0 : (a.axis == 1 ? a.b1 : a.b2);
  const unsigned nr = (unsigned)((m / 2 + R - 1) / R);
  return nr * (unsigned)(a.b0 * a.b1 * a.b2 / m);
}

template <typename T, bool INV, int R>
__host__ __device__ __forceinline__ void pass_item(const T* src, T* dst, const PassArgs& a, unsigned t) {
  int m, run;
  long long so, dof, sst, dstd;
  if (a.axis == 0) {              // lanes along consecutive runs of one line
    m = a.b0;
    const unsigned nr = (unsigned)((m / 2 + R - 1) / R);
    run = (int)(t % nr);
    const unsigned rest = t / nr;
    const int i1 = (int)(rest % (unsigned)a.b1), i2 = (int)(rest / (unsigned)a.b1);
    so = i1 * a.s1 + i2 * a.s2;
    dof = i1 * a.d1 + i2 * a.d2;
    sst = dstd = 1;
  } else {                        // lanes along dim 0, a run of one line each
    m = a.axis == 1 ? a.b1 : a.b2;
    const unsigned nr = (unsigned)((m / 2 + R - 1) / R);
    const int i0 = (int)(t % (unsigned)a.b0);
    const unsigned rest = t / (unsigned)a.b0;
    run = (int)(rest % nr);
    const int o = (int)(rest / nr);            // the remaining coordinate: i2 (axis 1) or i1 (axis 2)
    if (a.axis == 1) {
      so = i0 + o * a.s2; dof = i0 + o * a.d2; sst = a.s1; dstd = a.d1;
    } else {
      so = i0 + o * a.s1; dof = i0 + o * a.d1; sst = a.s2; dstd = a.d2;
    }
  }
  const int h = m / 2, k0 = run * R;
  const int cnt = h - k0 < R ? h - k0 : R;
  if (INV) inv_run<T, R>(src + so, sst, dst + dof, dstd, m, k0, cnt);
  else fwd_run<T, R>(src + so, sst, dst + dof, dstd, m, k0, cnt);
}

template <typename T, bool INV, int R>
__global__ __launch_bounds__(BLOCK) void k_dwt_pass(const T* __restrict__ src, T* __restrict__ dst, PassArgs a, unsigned items,
                                                    const ProjScalars<T>* __restrict__ gate) {
  if (gate && !gate->need) return;
  const unsigned t = blockIdx.x * BLOCK + threadIdx.x;
  if (t >= items) return;
  pass_item<T, INV, R>(src, dst, a, t);
}

// every level of a box of at most SMALL entries, by threads tid, tid + nth, ... of one workgroup: box of src (strides 1, s1, s2)
// -> buf[0] / buf[1] (compact) -> box of dst.  sync() separates the steps.
template <typename T, bool INV, typename Sync>
__host__ __device__ inline void small_box(const T* src, T* dst, long long s1, long long s2, int b0, int b1, int b2, int ndim, int nlev,
                                          T* buf0, T* buf1, int tid, int nth, Sync sync) {
  const int nb = b0 * b1 * b2;
  for (int e = tid; e < nb; e += nth) {
    const int i0 = e % b0, r = e / b0;
    buf0[e] = src[i0 + (r % b1) * s1 + (r / b1) * s2];
  }
  sync();
  for (int v = 0; v < nlev; ++v) {
    const int lev = INV ? nlev - 1 - v : v;
    PassArgs a;
    a.s1 = a.d1 = b0;
    a.s2 = a.d2 = (long long)b0 * b1;
    a.b0 = b0 >> lev;
    a.b1 = b1 >> lev;
    a.b2 = ndim == 3 ? b2 >> lev : 1;
    int cur = 0;
    for (int q = 0; q < ndim; ++q) {
      a.axis = INV ? ndim - 1 - q : q;
      const unsigned items = pass_items<1>(a);
      for (unsigned t = tid; t < items; t += nth) pass_item<T, INV, 1>(cur ? buf1 : buf0, cur ? buf0 : buf1, a, t);
      sync();
      cur ^= 1;
    }
    if (cur) {                                 // the level ended in buf[1]: its box back to buf[0]
      const int bn = a.b0 * a.b1 * a.b2;
      for (int e = tid; e < bn; e += nth) {
        const int i0 = e % a.b0, r = e / a.b0;
        const int o = i0 + (r % a.b1) * b0 + (r / a.b1) * b0 * b1;
        buf0[o] = buf1[o];
      }
      sync();
    }
  }
  for (int e = tid; e < nb; e += nth) {
    const int i0 = e % b0, r = e / b0;
    dst[i0 + (r % b1) * s1 + (r / b1) * s2] = buf0[e];
  }
}

struct BlockSync {
  __device__ void operator()() const { __syncthreads(); }
};

template <typename T, bool INV>
__global__ __launch_bounds__(SMALL_BLOCK) void k_dwt_small(const T* src, T* dst, long long s1, long long s2, int b0, int b1, int b2,
                                                           int ndim, int nlev, const ProjScalars<T>* __restrict__ gate) {
  if (gate && !gate->need) return;
  __shared__ T buf[2][SMALL];
  small_box<T, INV>(src, dst, s1, s2, b0, b1, b2, ndim, nlev, buf[0], buf[1], (int)threadIdx.x, SMALL_BLOCK, BlockSync());
}

template <typename T, bool INV>
void launch_pass(hipStream_t s, const T* src, long long s1, long long s2, T* dst, long long d1, long long d2, const long long* b,
                 int axis, const ProjScalars<T>* gate) {
  PassArgs a;
  a.s1 = s1; a.s2 = s2; a.d1 = d1; a.d2 = d2;
  a.b0 = (int)b[0]; a.b1 = (int)b[1]; a.b2 = (int)b[2]; a.axis = axis;
  if (axis == 0) {
    const unsigned items = pass_items<RC>(a);
    hipLaunchKernelGGL((k_dwt_pass<T, INV, RC>), dim3((items + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, src, dst, a, items, gate);
  } else {
    const unsigned items = pass_items<RS>(a);
    hipLaunchKernelGGL((k_dwt_pass<T, INV, RS>), dim3((items + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, src, dst, a, items, gate);
  }
  SIPX_HIP(hipGetLastError());
}

template <typename T>
__global__ __launch_bounds__(BLOCK) void k_dwt_copy(long long N, const T* __restrict__ src, T* __restrict__ dst,
                                                    const ProjScalars<T>* __restrict__ gate) {
  if (gate && !gate->need) return;
  for (long long e = (long long)blockIdx.x * BLOCK + threadIdx.x; e < N; e += (long long)gridDim.x * BLOCK) dst[e] = src[e];
}

struct Shape {
  int ndim, L;
  long long n[3], N;
};

Shape shape_of(int ndim, const long long* n) {
  dwt_check_grid(ndim, n);
  Shape sh;
  sh.ndim = ndim;
  sh.n[0] = n[0]; sh.n[1] = n[1]; sh.n[2] = ndim == 3 ? n[2] : 1;
  sh.N = sh.n[0] * sh.n[1] * sh.n[2];
  sh.L = dwt_levels(ndim, n);
  return sh;
}

// first level whose box fits one workgroup (L + 1: none)
int first_small(const Shape& sh, long long* b) {
  for (int a = 0; a < 3; ++a) b[a] = sh.n[a];
  int l = 1;
  while (l <= sh.L && b[0] * b[1] * b[2] > SMALL) {
    b[0] /= 2; b[1] /= 2;
    if (sh.ndim == 3) b[2] /= 2;
    ++l;
  }
  return l;
}

void level_box(const Shape& sh, int l, long long* b) {
  for (int a = 0; a < 3; ++a) b[a] = sh.n[a];
  for (int q = 1; q < l; ++q) {
    b[0] /= 2; b[1] /= 2;
    if (sh.ndim == 3) b[2] /= 2;
  }
}

}  // namespace

template <typename T>
void dwt_forward(hipStream_t s, int ndim, const long long* n, const T* in, T* out, T* scratch) {
  const Shape sh = shape_of(ndim, n);
  const long long f1 = sh.n[0], f2 = sh.n[0] * sh.n[1];
  if (sh.L == 0) {
    SIPX_HIP(hipMemcpyAsync(out, in, sizeof(T) * sh.N, hipMemcpyDeviceToDevice, s));
    return;
  }
  long long bs[3];
  const int ls = first_small(sh, bs);
  for (int l = 1; l < ls; ++l) {
    long long b[3];
    level_box(sh, l, b);
    if (l == 1) {                    // in -> (out | scratch) ... -> out, full strides
      const T* src = in;
      for (int q = 0; q < ndim; ++q) {
        T* dst = (ndim - 1 - q) % 2 == 0 ? out : scratch;
        launch_pass<T, false>(s, src, f1, f2, dst, f1, f2, b, q, nullptr);
        src = dst;
      }
    } else {                         // box of out -> compact boxes at the front of scratch -> box of out
      const long long bn = b[0] * b[1] * b[2];
      T* cb[2] = {scratch, scratch + bn};
      const long long c1 = b[0], c2 = b[0] * b[1];
      const T* src = out;
      long long sa = f1, sb = f2;
      for (int q = 0; q < ndim; ++q) {
        const bool last = q == ndim - 1;
        T* dst = last ? out : cb[q % 2];
        const long long da = last ? f1 : c1, db = last ? f2 : c2;
        launch_pass<T, false>(s, src, sa, sb, dst, da, db, b, q, nullptr);
        src = dst; sa = da; sb = db;
      }
    }
  }
  if (ls <= sh.L) {
    hipLaunchKernelGGL((k_dwt_small<T, false>), dim3(1), dim3(SMALL_BLOCK), 0, s, ls == 1 ? in : (const T*)out, out, f1, f2,
                       (int)bs[0], (int)bs[1], (int)bs[2], ndim, sh.L - ls + 1, (const ProjScalars<T>*)nullptr);
    SIPX_HIP(hipGetLastError());
  }
}

template <typename T>
void dwt_inverse(hipStream_t s, int ndim, const long long* n, T* in, T* out, T* scratch, const ProjScalars<T>* gate) {
  const Shape sh = shape_of(ndim, n);
  const long long f1 = sh.n[0], f2 = sh.n[0] * sh.n[1];
  if (sh.L == 0) {
    hipLaunchKernelGGL((k_dwt_copy<T>), dim3(fit_grid(sh.N, NB)), dim3(BLOCK), 0, s, sh.N, (const T*)in, out, gate);
    SIPX_HIP(hipGetLastError());
    return;
  }
  long long bs[3];
  const int ls = first_small(sh, bs);
  if (ls <= sh.L) {                  // the deepest levels: in place on in, or straight into out when the whole grid is small
    hipLaunchKernelGGL((k_dwt_small<T, true>), dim3(1), dim3(SMALL_BLOCK), 0, s, (const T*)in, ls == 1 ? out : in, f1, f2,
                       (int)bs[0], (int)bs[1], (int)bs[2], ndim, sh.L - ls + 1, gate);
    SIPX_HIP(hipGetLastError());
    if (ls == 1) return;
  }
  for (int l = ls - 1; l >= 1; --l) {
    long long b[3];
    level_box(sh, l, b);
    if (l == 1) {                    // in -> scratch -> in -> out (3-D), in -> scratch -> out (2-D)
      T* src = in;
      for (int q = 0; q < ndim; ++q) {
        const bool last = q == ndim - 1;
        T* dst = last ? out : (q % 2 == 0 ? scratch : in);
        launch_pass<T, true>(s, src, f1, f2, dst, f1, f2, b, ndim - 1 - q, gate);
        src = dst;
      }
    } else {                         // box of in -> compact boxes -> box of in
      const long long bn = b[0] * b[1] * b[2];
      T* cb[2] = {scratch, scratch + bn};
      const long long c1 = b[0], c2 = b[0] * b[1];
      const T* src = in;
      long long sa = f1, sb = f2;
      for (int q = 0; q < ndim; ++q) {
        const bool last = q == ndim - 1;
        T* dst = last ? in : cb[q % 2];
        const long long da = last ? f1 : c1, db = last ? f2 : c2;
        launch_pass<T, true>(s, src, sa, sb, dst, da, db, b, ndim - 1 - q, gate);
        src = dst; sa = da; sb = db;
      }
    }
  }
}

template void dwt_forward<float>(hipStream_t, int, const long long*, const float*, float*, float*);
template void dwt_forward<double>(hipStream_t, int, const long long*, const double*, double*, double*);
template void dwt_inverse<float>(hipStream_t, int, const long long*, float*, float*, float*, const ProjScalars<float>*);
template void dwt_inverse<double>(hipStream_t, int, const long long*, double*, double*, double*, const ProjScalars<double>*);

}  // namespace sipx
