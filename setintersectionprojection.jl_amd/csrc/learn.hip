// Constraint learning from training images (sipx_learn_observations, include/sipx.h; the reference's
// constraint_learning_by_obseration, src/constraint_learning_by_observation.jl:8-163), batched over chunks of B images.
//
// Per chunk: one strided copy of the caller's images -> k_learn_repack (image-major, column-major TF) -> k_learn_diff (D_x, D_z
// in the TDOperator's bits, the TV rows and float64 partials) -> optional hipFFT / DWT / DCT GEMM / SVD stages -> segmented radix
// sorts folded by k_learn_fold (histograms) and scanned by k_learn_card (cardinalities).
//
// Determinism: every per-image sum is a fixed two-stage tree.  Stage 1 splits each image into tiles of TILE elements (one
// workgroup per tile and image, a fixed per-thread order, then a fixed LDS tree); stage 2 (k_learn_finish) sums an image's tiles
// in a fixed order.  Neither the chunk size nor the launch grid enters that tree, so every chunking gives the same bits.
// Min / max folds are exact and order-free.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <hipfft/hipfft.h>
#include <rocblas/rocblas.h>
#include <rocsolver/rocsolver.h>

#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "device_memory.h"
#include "dwt.h"
#include "learn.h"
#include "sipx_common.h"

namespace sipx {
namespace {

constexpr int LB = 256;                 // threads per workgroup
constexpr int PER_THREAD = 16;
constexpr int TILE = LB * PER_THREAD;   // elements per stage-1 tile: part of the determinism contract
constexpr int CARD_ITEMS = 4;

// per-image float64 statistics: slots [0, NP) come from tile partials, the rest are written per image
enum {
  S_ABS_DX, S_ABS_DZ, S_SQ_DX, S_SQ_DZ, S_SQ_IMG, S_MIN_DX, S_MAX_DX, S_MIN_DZ, S_MAX_DZ, S_ABS_F, S_ABS_W, NP,
  S_NUC = NP, S_NUC_DX, S_NUC_DZ, S_RANK, S_CARD_F, S_CARD_TV, NS
};
__host__ __device__ constexpr int slot_op(int s) {     // 0 = sum, 1 = min, 2 = max
  return (s == S_MIN_DX || s == S_MIN_DZ) ? 1 : (s == S_MAX_DX || s == S_MAX_DZ) ? 2 : 0;
}
__device__ __forceinline__ double slot_init(int s) {
  return slot_op(s) == 1 ? INFINITY : slot_op(s) == 2 ? -INFINITY : 0.0;
}
__device__ __forceinline__ double slot_comb(int s, double a, double b) {
  return slot_op(s) == 1 ? fmin(a, b) : slot_op(s) == 2 ? fmax(a, b) : a + b;
}

// fixed LDS tree over the LB threads of a workgroup for slots [s0, s1); the result is valid in thread 0
template <int S0, int S1>
__device__ void block_reduce(double (&v)[NP], double (*sh)[LB]) {
#pragma unroll
  for (int s = S0; s < S1; ++s) sh[s][threadIdx.x] = v[s];
  __syncthreads();
  for (int w = LB / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
#pragma unroll
      for (int s = S0; s < S1; ++s) sh[s][threadIdx.x] = slot_comb(s, sh[s][threadIdx.x], sh[s][threadIdx.x + w]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int s = S0; s < S1; ++s) v[s] = sh[s][0];
}

// img[b N + a + n1 c] <- raw[b sb + a s1 + c s2]
template <typename T>
__global__ void k_learn_repack(const T* __restrict__ raw, int n1, long long N, long long B, long long sb, long long s1, long long s2,
                               T* __restrict__ img) {
  const long long total = B * N;
  for (long long g = blockIdx.x * (long long)LB + threadIdx.x; g < total; g += (long long)gridDim.x * LB) {
    const long long b = g / N, e = g - b * N;
    const long long a = e % n1, c = e / n1;
    img[g] = raw[b * sb + a * s1 + c * s2];
  }
}

// One read of each image: D_x (along dim 1) and D_z (along dim 2) as the TDOperator forms them, (-ih) x + ih x_next in TF with
// no FMA.  Writes the TV rows [D_z; D_x] (tv, atv = |TV|) and the float64 matrices of D_x / D_z when asked, and the tile partials
// of slots [S_ABS_DX, S_MAX_DZ].  grid = (tiles per image, images).
template <typename T>
__global__ __launch_bounds__(LB) void k_learn_diff(const T* __restrict__ img, int n1, int n2, T ih1, T ih2, T* __restrict__ tv,
                                                   T* __restrict__ atv, double* __restrict__ dxm, double* __restrict__ dzm,
                                                   double* __restrict__ part) {
  __shared__ double sh[NP][LB];
  const unsigned N = (unsigned)n1 * (unsigned)n2, Mz = (unsigned)n1 * (unsigned)(n2 - 1), Mx = (unsigned)(n1 - 1) * (unsigned)n2;
  const long long b = blockIdx.y;
  const int ntile = gridDim.x;
  const T* x = img + b * N;
  const T nih1 = -ih1, nih2 = -ih2;
  double v[NP];
#pragma unroll
  for (int s = 0; s < NP; ++s) v[s] = slot_init(s);
  for (int k = 0; k < PER_THREAD; ++k) {
    const unsigned e = blockIdx.x * (unsigned)TILE + k * LB + threadIdx.x;
    if (e >= N) break;
    const unsigned c = e / (unsigned)n1, a = e - c * (unsigned)n1;
    const T xe = x[e];
    v[S_SQ_IMG] += (double)xe * (double)xe;
    if (a + 1 < (unsigned)n1) {
      const T p = nih1 * xe, q = ih1 * x[e + 1];
      const T d = p + q;
      const double dd = d;
      const unsigned r = a + (unsigned)(n1 - 1) * c;
      v[S_ABS_DX] += fabs(dd);
      v[S_SQ_DX] += dd * dd;
      v[S_MIN_DX] = fmin(v[S_MIN_DX], dd);
      v[S_MAX_DX] = fmax(v[S_MAX_DX], dd);
      if (tv) tv[b * (Mz + Mx) + Mz + r] = d;
      if (atv) atv[b * (Mz + Mx) + Mz + r] = d < T(0) ? -d : d;
      if (dxm) dxm[b * Mx + r] = dd;
    }
    if (c + 1 < (unsigned)n2) {
      const T p = nih2 * xe, q = ih2 * x[e + n1];
      const T d = p + q;
      const double dd = d;
      v[S_ABS_DZ] += fabs(dd);
      v[S_SQ_DZ] += dd * dd;
      v[S_MIN_DZ] = fmin(v[S_MIN_DZ], dd);
      v[S_MAX_DZ] = fmax(v[S_MAX_DZ], dd);
      if (tv) tv[b * (Mz + Mx) + e] = d;
      if (atv) atv[b * (Mz + Mx) + e] = d < T(0) ? -d : d;
      if (dzm) dzm[b * Mz + e] = dd;
    }
  }
  block_reduce<0, S_ABS_F>(v, sh);
  if (threadIdx.x == 0) {
    double* o = part + (b * ntile + blockIdx.x) * NP;
    for (int s = 0; s < S_ABS_F; ++s) o[s] = v[s];
  }
}

// |F img| of a C2C spectrum scaled by 1/sqrt(N): tile partials of slot S_ABS_F, magnitudes in TF for the sort when mag != null
template <typename T, typename C2>
__global__ __launch_bounds__(LB) void k_learn_dft_abs(const C2* __restrict__ f, long long N, double scale, T* __restrict__ mag,
                                                      double* __restrict__ part) {
  __shared__ double sh[NP][LB];
  const long long b = blockIdx.y;
  double v[NP];
  v[S_ABS_F] = 0.0;
  for (int k = 0; k < PER_THREAD; ++k) {
    const long long e = (long long)blockIdx.x * TILE + k * LB + threadIdx.x;
    if (e >= N) break;
    const C2 z = f[b * N + e];
    const double m = std::sqrt((double)z.x * (double)z.x + (double)z.y * (double)z.y) * scale;
    v[S_ABS_F] += m;
    if (mag) mag[b * N + e] = (T)m;
  }
  block_reduce<S_ABS_F, S_ABS_F + 1>(v, sh);
  if (threadIdx.x == 0) part[(b * gridDim.x + blockIdx.x) * NP + S_ABS_F] = v[S_ABS_F];
}

// tile partials of sum |w| into slot S_ABS_W
template <typename T>
__global__ __launch_bounds__(LB) void k_learn_l1(const T* __restrict__ w, long long N, double* __restrict__ part) {
  __shared__ double sh[NP][LB];
  const long long b = blockIdx.y;
  double v[NP];
  v[S_ABS_W] = 0.0;
  for (int k = 0; k < PER_THREAD; ++k) {
    const long long e = (long long)blockIdx.x * TILE + k * LB + threadIdx.x;
    if (e >= N) break;
    v[S_ABS_W] += fabs((double)w[b * N + e]);
  }
  block_reduce<S_ABS_W, S_ABS_W + 1>(v, sh);
  if (threadIdx.x == 0) part[(b * gridDim.x + blockIdx.x) * NP + S_ABS_W] = v[S_ABS_W];
}

// stage 2: one workgroup per image sums its tiles in a fixed order into stats[b NS + s], s < NP
__global__ __launch_bounds__(LB) void k_learn_finish(const double* __restrict__ part, int ntile, double* __restrict__ stats) {
  __shared__ double sh[NP][LB];
  const long long b = blockIdx.x;
  double v[NP];
#pragma unroll
  for (int s = 0; s < NP; ++s) v[s] = slot_init(s);
  for (int t = threadIdx.x; t < ntile; t += LB) {
    const double* p = part + (b * ntile + t) * NP;
#pragma unroll
    for (int s = 0; s < NP; ++s) v[s] = slot_comb(s, v[s], p[s]);
  }
  block_reduce<0, NP>(v, sh);
  if (threadIdx.x == 0)
    for (int s = 0; s < NP; ++s) stats[b * NS + s] = v[s];
}

// running element-wise min (float64) / max (TF) over B sorted rows of length L
template <typename T>
__global__ void k_learn_fold(const T* __restrict__ rows, int B, long long L, double* __restrict__ mn, T* __restrict__ mx) {
  for (long long p = blockIdx.x * (long long)LB + threadIdx.x; p < L; p += (long long)gridDim.x * LB) {
    double lo = mn[p];
    T hi = mx[p];
    for (int b = 0; b < B; ++b) {
      const T r = rows[(long long)b * L + p];
      lo = fmin(lo, (double)r);
      hi = r > hi ? r : hi;
    }
    mn[p] = lo;
    mx[p] = hi;
  }
}

// One workgroup per image over an ascending row of magnitudes: k = first 0-based index with cumsum[k] / total > 0.05 (float64
// block scan, stops at the first chunk that crosses), stats[b NS + out] = L - (k + 1); 0 when total == 0.  total is the sum of
// stats slots t0 and t1 (t1 < 0: none).
template <typename T>
__global__ __launch_bounds__(LB) void k_learn_card(const T* __restrict__ rows, long long L, double* __restrict__ stats, int t0, int t1,
                                                   int out) {
  __shared__ double scan[LB];
  __shared__ unsigned long long found;
  const long long b = blockIdx.x;
  const T* r = rows + b * L;
  const double total = stats[b * NS + t0] + (t1 >= 0 ? stats[b * NS + t1] : 0.0);
  if (threadIdx.x == 0) found = (unsigned long long)L;
  __syncthreads();
  double carry = 0.0;
  for (long long base = 0; total > 0.0 && base < L; base += (long long)LB * CARD_ITEMS) {
    double x[CARD_ITEMS], s = 0.0;
    const long long i0 = base + (long long)threadIdx.x * CARD_ITEMS;
#pragma unroll
    for (int q = 0; q < CARD_ITEMS; ++q) {
      x[q] = i0 + q < L ? (double)r[i0 + q] : 0.0;
      s += x[q];
    }
    scan[threadIdx.x] = s;
    __syncthreads();
    for (int w = 1; w < LB; w <<= 1) {          // Hillis-Steele inclusive scan: a fixed order
      const double add = (int)threadIdx.x >= w ? scan[threadIdx.x - w] : 0.0;
      __syncthreads();
      scan[threadIdx.x] += add;
      __syncthreads();
    }
    double run = carry + (scan[threadIdx.x] - s);
    for (int q = 0; q < CARD_ITEMS; ++q) {
      run += x[q];
      if (i0 + q < L && run / total > 0.05) {
        atomicMin(&found, (unsigned long long)(i0 + q));
        break;
      }
    }
    carry += scan[LB - 1];
    __syncthreads();
    if (found < (unsigned long long)L) break;
  }
  if (threadIdx.x == 0) stats[b * NS + out] = (total > 0.0 && found < (unsigned long long)L) ? (double)(L - ((long long)found + 1)) : 0.0;
}

// per image: sum of sigma in descending order and rank_095.  w holds nv values per image at stride ws: eigenvalues of the Gram
// matrix in ascending order (eig = 1, sigma = sqrt(max(lambda, 0))) or singular values in descending order (eig = 0).
__global__ void k_learn_sv(const double* __restrict__ w, int nv, long long ws, int eig, int B, double* __restrict__ stats, int nuc,
                           int rank) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double* p = w + (long long)b * ws;
  auto sig = [&](int q) { return eig ? std::sqrt(fmax(p[nv - 1 - q], 0.0)) : p[q]; };
  double sum = 0.0;
  for (int q = 0; q < nv; ++q) sum += sig(q);
  stats[(long long)b * NS + nuc] = sum;
  if (rank >= 0) {
    double cum = 0.0;
    int k = 0;
    for (int q = 0; q < nv && sum > 0.0; ++q) {
      cum += sig(q);
      if (cum / sum > 0.95) { k = q + 1; break; }
    }
    stats[(long long)b * NS + rank] = k;
  }
}

// Y is K x J column-major (rows = DCT index): partial min / max of row k over the columns j = g, g + G, ...  grid = (K / LB, G)
template <typename T>
__global__ void k_learn_dct_minmax(const T* __restrict__ Y, int K, long long J, T* __restrict__ pmin, T* __restrict__ pmax) {
  const int k = blockIdx.x * LB + threadIdx.x;
  if (k >= K) return;
  T lo = INFINITY, hi = -INFINITY;
  for (long long j = blockIdx.y; j < J; j += gridDim.y) {
    const T y = Y[k + j * K];
    lo = y < lo ? y : lo;
    hi = y > hi ? y : hi;
  }
  pmin[(long long)blockIdx.y * K + k] = lo;
  pmax[(long long)blockIdx.y * K + k] = hi;
}
template <typename T>
__global__ void k_learn_dct_fold(const T* __restrict__ pmin, const T* __restrict__ pmax, int K, int G, double* __restrict__ lb,
                                 T* __restrict__ ub) {
  const int k = blockIdx.x * LB + threadIdx.x;
  if (k >= K) return;
  double lo = lb[k];
  T hi = ub[k];
  for (int g = 0; g < G; ++g) {
    lo = fmin(lo, (double)pmin[(long long)g * K + k]);
    const T m = pmax[(long long)g * K + k];
    hi = m > hi ? m : hi;
  }
  lb[k] = lo;
  ub[k] = hi;
}

template <typename T, typename C2>
__global__ void k_learn_to_complex(const T* __restrict__ x, long long n, C2* __restrict__ z) {
  for (long long g = blockIdx.x * (long long)LB + threadIdx.x; g < n; g += (long long)gridDim.x * LB) z[g] = C2{x[g], T(0)};
}
template <typename T>
__global__ void k_learn_to_f64(const T* __restrict__ x, long long n, double* __restrict__ y) {
  for (long long g = blockIdx.x * (long long)LB + threadIdx.x; g < n; g += (long long)gridDim.x * LB) y[g] = x[g];
}
template <typename T>
__global__ void k_learn_fill(T* __restrict__ x, long long n, T v) {
  for (long long g = blockIdx.x * (long long)LB + threadIdx.x; g < n; g += (long long)gridDim.x * LB) x[g] = v;
}

inline unsigned grid_for(long long n) { return (unsigned)std::min<long long>(std::max<long long>((n + LB - 1) / LB, 1), 8192); }

void fft_ok(hipfftResult r, const char* what) {
  if (r != HIPFFT_SUCCESS) throw std::runtime_error(std::string("learn: hipFFT ") + what + " failed (" + std::to_string((int)r) + ")");
}
void blas_ok(rocblas_status r, const char* what) {
  if (r != rocblas_status_success)
    throw std::runtime_error(std::string("learn: rocBLAS/rocSOLVER ") + what + " failed (" + std::to_string((int)r) + ")");
}

// every device buffer and library handle of one call, released on any exit
struct Arena {
  DeviceMemory mem;      // (first: freed after the handles below are gone)
  rocblas_handle blas = nullptr;
  hipfftHandle plan = 0;
  bool has_plan = false;
  template <typename Q>
  Q* get(long long count) {
    return mem.alloc<Q>((size_t)std::max<long long>(count, 1), Mem::NoFill);
  }
  ~Arena() {
    (void)hipDeviceSynchronize();
    if (has_plan) hipfftDestroy(plan);
    if (blas) rocblas_destroy_handle(blas);
  }
};

template <typename T> struct Cplx;
template <> struct Cplx<float> { using type = hipfftComplex; static constexpr hipfftType ty = HIPFFT_C2C; };
template <> struct Cplx<double> { using type = hipfftDoubleComplex; static constexpr hipfftType ty = HIPFFT_Z2Z; };

hipfftResult fft_exec(hipfftHandle p, hipfftComplex* z) { return hipfftExecC2C(p, z, z, HIPFFT_FORWARD); }
hipfftResult fft_exec(hipfftHandle p, hipfftDoubleComplex* z) { return hipfftExecZ2Z(p, z, z, HIPFFT_FORWARD); }
rocblas_status gemm(rocblas_handle h, rocblas_operation ta, rocblas_operation tb, int m, int n, int k, const float* A, int lda,
                    long long sa, const float* B, int ldb, long long sb, float* C, int ldc, long long sc, int batch) {
  const float one = 1.f, zero = 0.f;
  return rocblas_sgemm_strided_batched(h, ta, tb, m, n, k, &one, A, lda, sa, B, ldb, sb, &zero, C, ldc, sc, batch);
}
rocblas_status gemm(rocblas_handle h, rocblas_operation ta, rocblas_operation tb, int m, int n, int k, const double* A, int lda,
                    long long sa, const double* B, int ldb, long long sb, double* C, int ldc, long long sc, int batch) {
  const double one = 1.0, zero = 0.0;
  return rocblas_dgemm_strided_batched(h, ta, tb, m, n, k, &one, A, lda, sa, B, ldb, sb, &zero, C, ldc, sc, batch);
}

// orthonormal DCT-II as a dense n x n column-major matrix, built in float64 and rounded to TF once (as EXT_DCT builds it)
template <typename T>
std::vector<T> dct_matrix(int n) {
  const double PI = 3.14159265358979323846;
  std::vector<T> C((size_t)n * n);
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < n; ++k)
      C[(size_t)i * n + k] = (T)((k == 0 ? std::sqrt(1.0 / n) : std::sqrt(2.0 / n)) * std::cos(PI * (2.0 * i + 1.0) * k / (2.0 * n)));
  return C;
}

template <typename T>
void learn_T(const long long n1, const long long n2, const double* h, long long n_train, const T* host, const int64_t* st,
             long long max_batch, sipx_observations* o) {
  using C2 = typename Cplx<T>::type;
  const bool f64 = sizeof(T) == 8;
  const long long N = n1 * n2, Mx = (n1 - 1) * n2, Mz = n1 * (n2 - 1), M = Mx + Mz, L = std::max(N, M);
  const long long ntile = (N + TILE - 1) / TILE;

  // what is wanted decides what runs
  const bool w_hist = o->hist_min || o->hist_max, w_htv = o->hist_TV_min || o->hist_TV_max, w_ctv = o->TV_card_095 != nullptr;
  const bool w_cf = o->DFT_card_095 != nullptr, w_dft = w_cf || o->DFT_l1;
  const bool w_dwt = o->wavelet_l1 && n1 == n2;
  const bool w_dx = o->DCT_x_LB || o->DCT_x_UB, w_dy = o->DCT_y_LB || o->DCT_y_UB;
  const bool w_svi = o->nuclear_norm || o->rank_095, w_svx = o->nuclear_Dx != nullptr, w_svz = o->nuclear_Dz != nullptr;
  const bool w_sort = w_hist || w_htv || w_ctv || w_cf;

  // the caller's layout: image-major blocks (s0 >= span) or image fastest over a uniform pitch P = min(s1, s2)
  const long long s0 = n_train == 1 ? 0 : st[0], s1 = st[1], s2 = st[2];
  if (s1 <= 0 || s2 <= 0 || s0 < 0) throw std::runtime_error("learn: strides must be positive");
  const long long span = (n1 - 1) * s1 + (n2 - 1) * s2 + 1;
  bool outer;
  long long P = 1;
  if (n_train == 1 || s0 >= span) {
    outer = true;
  } else if (s0 == 1) {
    P = std::min(s1, s2);
    if (P < n_train || std::max(s1, s2) % P) throw std::runtime_error("learn: unsupported m_train layout (pass a contiguous array)");
    outer = false;
  } else {
    throw std::runtime_error("learn: unsupported m_train layout (pass a contiguous array)");
  }
  const long long rows = outer ? span : (span - 1) / P + 1;      // elements (outer) or pitch rows (image fastest) per chunk unit

  // bytes per image of one chunk
  const long long w = sizeof(T);
  long long per = rows * w + N * w + ntile * NP * 8 + NS * 8;
  if (w_htv || w_ctv) per += M * w;
  if (w_ctv) per += M * w;
  if (w_sort) per += 2 * L * w + 64;                  // sorted row and radix-sort temporary storage (estimate)
  if (w_dft) per += 4 * N * w + (w_cf ? N * w : 0);   // spectrum, FFT work area (estimate), magnitudes
  if (w_dwt) per += N * w;
  if (w_dx || w_dy) per += N * w;
  const long long mi = std::min(n1, n2), mx_ = std::min(n1 - 1, n2), mz_ = std::min(n1, n2 - 1);
  if (w_svi) per += N * 8 + (mi * mi + 2 * mi) * 8;
  if (w_svx) per += Mx * 8 + (mx_ * mx_ + 2 * mx_) * 8;
  if (w_svz) per += Mz * 8 + (mz_ * mz_ + 2 * mz_) * 8;
  long long B = max_batch;
  if (B <= 0) {
    size_t fr = 0, tot = 0;
    SIPX_HIP(hipMemGetInfo(&fr, &tot));
    B = (long long)(0.4 * (double)fr) / per;
    if (B < 1) throw std::runtime_error("learn: one image does not fit in 40 % of the free device memory");
  }
  B = std::min(B, n_train);
  B = std::min(B, (long long)(INT32_MAX / std::max<long long>(L, 2 * N)));   // segmented-sort offsets and FFT sizes are int
  B = std::min(B, 65535LL);                          // grid.y of the per-tile kernels
  if (B < 1) throw std::runtime_error("learn: image too large");

  Arena A;
  T* raw = A.get<T>(B * rows);
  T* img = A.get<T>(B * N);
  double* part = A.get<double>(B * ntile * NP);
  double* stats = A.get<double>(B * NS);
  T* tv = (w_htv || w_ctv) ? A.get<T>(B * M) : nullptr;
  T* atv = w_ctv ? A.get<T>(B * M) : nullptr;
  T* sbuf = w_sort ? A.get<T>(B * L) : nullptr;
  C2* spec = w_dft ? A.get<C2>(B * N) : nullptr;
  T* mag = w_cf ? A.get<T>(B * N) : nullptr;
  T* wout = w_dwt ? A.get<T>(B * N) : nullptr;
  T* wscr = w_dwt ? A.get<T>(N) : nullptr;
  T* Y = (w_dx || w_dy) ? A.get<T>(B * N) : nullptr;
  double* dimg = w_svi ? A.get<double>(B * N) : nullptr;
  double* dxm = w_svx ? A.get<double>(B * Mx) : nullptr;
  double* dzm = w_svz ? A.get<double>(B * Mz) : nullptr;

  // accumulators with the reference's starting values: 1e8 (float64) for the minima, 0 (TF) for the maxima
  auto acc = [&](bool want, long long len, double*& lo, T*& hi) {
    if (!want) return;
    lo = A.get<double>(len);
    hi = A.get<T>(len);
    k_learn_fill<double><<<grid_for(len), LB>>>(lo, len, 1e8);
    SIPX_HIP(hipMemset(hi, 0, sizeof(T) * len));
  };
  double *hmin = nullptr, *htmin = nullptr, *cxlo = nullptr, *cylo = nullptr;
  T *hmax = nullptr, *htmax = nullptr, *cxhi = nullptr, *cyhi = nullptr;
  acc(w_hist, N, hmin, hmax);
  acc(w_htv, M, htmin, htmax);
  acc(w_dx, n1, cxlo, cxhi);
  acc(w_dy, n2, cylo, cyhi);

  constexpr int DCT_G = 256;
  T *Cx = nullptr, *Cy = nullptr, *pmin = nullptr, *pmax = nullptr;
  if (w_dx || w_dy) {
    pmin = A.get<T>(DCT_G * std::max(n1, n2));
    pmax = A.get<T>(DCT_G * std::max(n1, n2));
  }
  if (w_dx) {
    std::vector<T> c = dct_matrix<T>((int)n1);
    Cx = A.get<T>(n1 * n1);
    SIPX_HIP(hipMemcpy(Cx, c.data(), sizeof(T) * c.size(), hipMemcpyHostToDevice));
  }
  if (w_dy) {
    std::vector<T> c = dct_matrix<T>((int)n2);
    Cy = A.get<T>(n2 * n2);
    SIPX_HIP(hipMemcpy(Cy, c.data(), sizeof(T) * c.size(), hipMemcpyHostToDevice));
  }

  // segment offsets b L for b <= B (rows of length N, M or L start at b N, b M: separate tables)
  int *offN = nullptr, *offM = nullptr;
  void* sort_tmp = nullptr;
  size_t sort_bytes = 0;
  if (w_sort) {
    std::vector<int> oN(B + 1), oM(B + 1);
    for (long long b = 0; b <= B; ++b) { oN[b] = (int)(b * N); oM[b] = (int)(b * M); }
    offN = A.get<int>(B + 1);
    offM = A.get<int>(B + 1);
    SIPX_HIP(hipMemcpy(offN, oN.data(), sizeof(int) * (B + 1), hipMemcpyHostToDevice));
    SIPX_HIP(hipMemcpy(offM, oM.data(), sizeof(int) * (B + 1), hipMemcpyHostToDevice));
    size_t bn = 0, bm = 0;
    SIPX_HIP(hipcub::DeviceSegmentedRadixSort::SortKeys(nullptr, bn, (const T*)img, sbuf, (int)(B * N), (int)B, offN, offN + 1));
    SIPX_HIP(hipcub::DeviceSegmentedRadixSort::SortKeys(nullptr, bm, (const T*)sbuf, sbuf, (int)(B * M), (int)B, offM, offM + 1));
    sort_bytes = std::max(bn, bm);
    sort_tmp = A.get<char>((long long)sort_bytes);
  }
  auto sort_rows = [&](const T* in, long long len, const int* off, int Bc) {
    size_t bytes = sort_bytes;
    SIPX_HIP(hipcub::DeviceSegmentedRadixSort::SortKeys(sort_tmp, bytes, in, sbuf, (int)(Bc * len), Bc, off, off + 1));
  };

  double *sv_w = nullptr, *sv_e = nullptr, *sv_g = nullptr, *sv_res = nullptr;
  rocblas_int *sv_info = nullptr, *sv_sweeps = nullptr;
  if (w_dx || w_dy || w_svi || w_svx || w_svz) blas_ok(rocblas_create_handle(&A.blas), "create handle");
  if (w_svi || w_svx || w_svz) {
    const long long mm = std::max({w_svi ? mi : 0, w_svx ? mx_ : 0, w_svz ? mz_ : 0});
    sv_w = A.get<double>(B * mm);
    sv_e = A.get<double>(B * mm);
    if (!f64) sv_g = A.get<double>(B * mm * mm);
    sv_res = A.get<double>(B);
    sv_info = A.get<rocblas_int>(B);
    sv_sweeps = A.get<rocblas_int>(B);
  }
  // sum sigma (and rank) of B r x c float64 matrices at stride r c; a is destroyed on the gesvdj route
  auto svd = [&](double* a, long long r, long long c, int Bc, int nuc, int rank) {
    const long long k = std::min(r, c);
    if (f64) {
      blas_ok(rocsolver_dgesvdj_strided_batched(A.blas, rocblas_svect_none, rocblas_svect_none, (int)r, (int)c, a, (int)r, r * c, 0.0,
                                                sv_res, 100, sv_sweeps, sv_w, k, nullptr, (int)r, 0, nullptr, (int)c, 0, sv_info, Bc),
              "dgesvdj_strided_batched");
    } else {
      if (r >= c)
        blas_ok(gemm(A.blas, rocblas_operation_transpose, rocblas_operation_none, (int)c, (int)c, (int)r, a, (int)r, r * c, a, (int)r,
                     r * c, sv_g, (int)k, k * k, Bc), "Gram");
      else
        blas_ok(gemm(A.blas, rocblas_operation_none, rocblas_operation_transpose, (int)r, (int)r, (int)c, a, (int)r, r * c, a, (int)r,
                     r * c, sv_g, (int)k, k * k, Bc), "Gram");
      blas_ok(rocsolver_dsyevd_strided_batched(A.blas, rocblas_evect_none, rocblas_fill_upper, (int)k, sv_g, (int)k, k * k, sv_w, k,
                                               sv_e, k, sv_info, Bc), "dsyevd_strided_batched");
    }
    k_learn_sv<<<(Bc + LB - 1) / LB, LB>>>(sv_w, (int)k, k, f64 ? 0 : 1, Bc, stats, nuc, rank);
  };

  const T ih1 = T(1) / T(h[0]), ih2 = T(1) / T(h[1]);
  int plan_batch = 0;
  std::vector<double> hs;
  for (long long i0 = 0; i0 < n_train; i0 += B) {
    const int Bc = (int)std::min(B, n_train - i0);
    // upload: one strided copy, then the device repack to image-major column-major
    const T* src = host + i0 * s0;
    if (outer) {
      if (n_train == 1 || s0 == span) SIPX_HIP(hipMemcpy(raw, src, sizeof(T) * (Bc * span), hipMemcpyHostToDevice));
      else SIPX_HIP(hipMemcpy2D(raw, sizeof(T) * span, src, sizeof(T) * s0, sizeof(T) * span, Bc, hipMemcpyHostToDevice));
      k_learn_repack<T><<<grid_for(Bc * N), LB>>>(raw, (int)n1, N, Bc, span, s1, s2, img);
    } else {
      SIPX_HIP(hipMemcpy2D(raw, sizeof(T) * Bc, src, sizeof(T) * P, sizeof(T) * Bc, rows, hipMemcpyHostToDevice));
      k_learn_repack<T><<<grid_for(Bc * N), LB>>>(raw, (int)n1, N, Bc, 1, s1 / P * Bc, s2 / P * Bc, img);
    }
    SIPX_HIP(hipMemsetAsync(part, 0, sizeof(double) * Bc * ntile * NP));
    SIPX_HIP(hipMemsetAsync(stats, 0, sizeof(double) * Bc * NS));

    k_learn_diff<T><<<dim3((unsigned)ntile, Bc), LB>>>(img, (int)n1, (int)n2, ih1, ih2, tv, atv, dxm, dzm, part);
    if (w_dft) {
      if (plan_batch != Bc) {
        if (A.has_plan) fft_ok(hipfftDestroy(A.plan), "destroy");
        A.has_plan = false;
        int dims[2] = {(int)n2, (int)n1};
        fft_ok(hipfftPlanMany(&A.plan, 2, dims, nullptr, 1, (int)N, nullptr, 1, (int)N, Cplx<T>::ty, Bc), "plan");
        A.has_plan = true;
        plan_batch = Bc;
      }
      k_learn_to_complex<T, C2><<<grid_for(Bc * N), LB>>>(img, Bc * N, spec);
      fft_ok(fft_exec(A.plan, spec), "exec");
      k_learn_dft_abs<T, C2><<<dim3((unsigned)ntile, Bc), LB>>>(spec, N, 1.0 / std::sqrt((double)N), mag, part);
    }
    if (w_dwt) {
      const long long nn[3] = {n1, n2, 1};
      for (int b = 0; b < Bc; ++b) dwt_forward<T>(nullptr, 2, nn, img + b * N, wout + b * N, wscr);
      k_learn_l1<T><<<dim3((unsigned)ntile, Bc), LB>>>(wout, N, part);
    }
    k_learn_finish<<<Bc, LB>>>(part, (int)ntile, stats);

    if (w_hist) {
      sort_rows(img, N, offN, Bc);
      k_learn_fold<T><<<grid_for(N), LB>>>(sbuf, Bc, N, hmin, hmax);
    }
    if (w_htv) {
      sort_rows(tv, M, offM, Bc);
      k_learn_fold<T><<<grid_for(M), LB>>>(sbuf, Bc, M, htmin, htmax);
    }
    if (w_ctv) {
      sort_rows(atv, M, offM, Bc);
      k_learn_card<T><<<Bc, LB>>>(sbuf, M, stats, S_ABS_DX, S_ABS_DZ, S_CARD_TV);
    }
    if (w_cf) {
      sort_rows(mag, N, offN, Bc);
      k_learn_card<T><<<Bc, LB>>>(sbuf, N, stats, S_ABS_F, -1, S_CARD_F);
    }
    // The DCT GEMMs run one image per call: a GEMM's result can depend on its problem size (the library picks the kernel from
    // it), so a size that grows with the chunk would break the bits-for-every-chunking contract.
    if (w_dx) {         // Y_b = C1 img_b: n1 x n2 per image; rows k over all columns of every image
      for (int b = 0; b < Bc; ++b)
        blas_ok(gemm(A.blas, rocblas_operation_none, rocblas_operation_none, (int)n1, (int)n2, (int)n1, Cx, (int)n1, 0, img + b * N,
                     (int)n1, 0, Y + b * N, (int)n1, 0, 1), "DCT dim 1");
      const int G = (int)std::min<long long>(DCT_G, n2 * Bc);
      k_learn_dct_minmax<T><<<dim3((unsigned)((n1 + LB - 1) / LB), G), LB>>>(Y, (int)n1, n2 * Bc, pmin, pmax);
      k_learn_dct_fold<T><<<(unsigned)((n1 + LB - 1) / LB), LB>>>(pmin, pmax, (int)n1, G, cxlo, cxhi);
    }
    if (w_dy) {         // Z_b' = C2 img_b': n2 x n1 per image, so the DCT index is again the row
      for (int b = 0; b < Bc; ++b)
        blas_ok(gemm(A.blas, rocblas_operation_none, rocblas_operation_transpose, (int)n2, (int)n1, (int)n2, Cy, (int)n2, 0,
                     img + b * N, (int)n1, 0, Y + b * N, (int)n2, 0, 1), "DCT dim 2");
      const int G = (int)std::min<long long>(DCT_G, n1 * Bc);
      k_learn_dct_minmax<T><<<dim3((unsigned)((n2 + LB - 1) / LB), G), LB>>>(Y, (int)n2, n1 * Bc, pmin, pmax);
      k_learn_dct_fold<T><<<(unsigned)((n2 + LB - 1) / LB), LB>>>(pmin, pmax, (int)n2, G, cylo, cyhi);
    }
    if (w_svi) {
      k_learn_to_f64<T><<<grid_for(Bc * N), LB>>>(img, Bc * N, dimg);
      svd(dimg, n1, n2, Bc, S_NUC, S_RANK);
    }
    if (w_svx) svd(dxm, n1 - 1, n2, Bc, S_NUC_DX, -1);
    if (w_svz) svd(dzm, n1, n2 - 1, Bc, S_NUC_DZ, -1);
    SIPX_HIP(hipGetLastError());

    hs.resize((size_t)Bc * NS);
    SIPX_HIP(hipMemcpy(hs.data(), stats, sizeof(double) * Bc * NS, hipMemcpyDeviceToHost));
    using TI = typename std::conditional<sizeof(T) == 8, int64_t, int32_t>::type;
    auto put = [&](void* dst, auto f) {
      if (!dst) return;
      for (int b = 0; b < Bc; ++b) ((T*)dst)[i0 + b] = (T)f(&hs[(size_t)b * NS]);
    };
    auto put_i = [&](void* dst, int s) {
      if (!dst) return;
      for (int b = 0; b < Bc; ++b) ((TI*)dst)[i0 + b] = (TI)hs[(size_t)b * NS + s];
    };
    put(o->nuclear_norm, [](const double* s) { return s[S_NUC]; });
    put(o->nuclear_Dx, [](const double* s) { return s[S_NUC_DX]; });
    put(o->nuclear_Dz, [](const double* s) { return s[S_NUC_DZ]; });
    put_i(o->rank_095, S_RANK);
    put(o->TV, [](const double* s) { return s[S_ABS_DX] + s[S_ABS_DZ]; });
    put(o->wavelet_l1, [&](const double* s) { return w_dwt ? s[S_ABS_W] : 0.0; });
    put(o->Dx_l1, [](const double* s) { return s[S_ABS_DX]; });
    put(o->Dz_l1, [](const double* s) { return s[S_ABS_DZ]; });
    put(o->DFT_l1, [](const double* s) { return s[S_ABS_F]; });
    put_i(o->DFT_card_095, S_CARD_F);
    put_i(o->TV_card_095, S_CARD_TV);
    put(o->annulus, [](const double* s) { return std::sqrt(s[S_SQ_IMG]); });
    put(o->TV_annulus, [](const double* s) { return std::sqrt(s[S_SQ_DX] + s[S_SQ_DZ]); });
    put(o->D_l2, [](const double* s) { return std::sqrt(s[S_SQ_DX] + s[S_SQ_DZ]); });
    put(o->D_x_min, [](const double* s) { return s[S_MIN_DX]; });
    put(o->D_x_max, [](const double* s) { return s[S_MAX_DX]; });
    put(o->D_z_min, [](const double* s) { return s[S_MIN_DZ]; });
    put(o->D_z_max, [](const double* s) { return s[S_MAX_DZ]; });
  }
  auto down = [&](void* dst, const void* src, long long bytes) {
    if (dst) SIPX_HIP(hipMemcpy(dst, src, (size_t)bytes, hipMemcpyDeviceToHost));
  };
  if (w_hist) { down(o->hist_min, hmin, 8 * N); down(o->hist_max, hmax, w * N); }
  if (w_htv) { down(o->hist_TV_min, htmin, 8 * M); down(o->hist_TV_max, htmax, w * M); }
  if (w_dx) { down(o->DCT_x_LB, cxlo, 8 * n1); down(o->DCT_x_UB, cxhi, w * n1); }
  if (w_dy) { down(o->DCT_y_LB, cylo, 8 * n2); down(o->DCT_y_UB, cyhi, w * n2); }
}

}  // namespace

void learn_observations_host(int dtype, const int64_t* n, const double* h, int64_t n_train, const void* m_train,
                             const int64_t* strides, int64_t max_batch, sipx_observations* out, int device) {
  if (!n || !h || !m_train || !strides || !out) throw std::runtime_error("learn: null argument");
  if (n[0] < 2 || n[1] < 2) throw std::runtime_error("learn: the grid needs n1 >= 2 and n2 >= 2");
  if (n[0] * n[1] >= (int64_t)INT32_MAX / 2) throw std::runtime_error("learn: image too large");
  if (n_train < 1) throw std::runtime_error("learn: no training images");
  if (!(h[0] > 0) || !(h[1] > 0)) throw std::runtime_error("learn: grid spacings must be positive");
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
    throw std::runtime_error("libsipx: no HIP device visible -- this engine has no CPU fallback");
  SIPX_HIP(hipSetDevice(device));
  if (dtype == SIPX_F32) learn_T<float>(n[0], n[1], h, n_train, (const float*)m_train, strides, max_batch, out);
  else if (dtype == SIPX_F64) learn_T<double>(n[0], n[1], h, n_train, (const double*)m_train, strides, max_batch, out);
  else throw std::runtime_error("dtype must be SIPX_F32 or SIPX_F64");
}

}  // namespace sipx
