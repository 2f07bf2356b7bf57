// Projectors behind a transform of the whole model: they act on a materialised vector v (N reals).
//
//   DFT-folded l1 ball  x -> Re( F^H P_l1( F x ) ), F the unitary 3-D/2-D DFT
//       reference: get_projector.jl:29-35 with A = joDFT(...) (get_TD_operator.jl:45-47,80-82),
//       project_l1_Duchi! on Complex{TF} (project_l1_Duchi!.jl:29-32,49).  hipFFT does the
//       (unnormalised) transforms; the unitary 1/sqrt(N) factors are folded into the radius
//       (b*sqrt(N) on the raw spectrum) and into the inverse (1/N); the threshold search is the
//       engine's own l1 machinery on the magnitudes.  The joDFT normalisation is NOT pinned by
//       any reference test: unitary is assumed because the operator declares AtA_diag.
//   the DFT mask and cardinality behind the DFT on the same plans; DCT (dense matrices through rocBLAS) and
//   DWT (kernels_dwt.hip) with the engine's own projectors on the coefficient array.
#include <algorithm>
#include <cmath>

#include "dwt.h"
#include "ext_family.h"

namespace sipx {

template <typename T>
struct Cplx {
  T re, im;
};

template <typename T>
__global__ __launch_bounds__(BLOCK) void k_pack(long long N, const T* __restrict__ v, Cplx<T>* __restrict__ z) {
  for (long long e = (long long)blockIdx.x * BLOCK + threadIdx.x; e < N; e += (long long)gridDim.x * BLOCK) {
    Cplx<T> c;
    c.re = v[e];
    c.im = T(0);
    z[e] = c;
  }
}
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_cabs(long long N, const Cplx<T>* __restrict__ z, T* __restrict__ mag) {
  for (long long e = (long long)blockIdx.x * BLOCK + threadIdx.x; e < N; e += (long long)gridDim.x * BLOCK)
    mag[e] = (T)hypot((double)z[e].re, (double)z[e].im);
}
// z <- sign(z) * max(|z| - theta, 0), sign(z) = z/|z|   (project_l1_Duchi!.jl:49 on complex input)
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_csoft(long long N, Cplx<T>* __restrict__ z, const T* __restrict__ mag,
                                                 const ProjScalars<T>* __restrict__ ps) {
  const T th = ps->theta;
  for (long long e = (long long)blockIdx.x * BLOCK + threadIdx.x; e < N; e += (long long)gridDim.x * BLOCK) {
    const T a = mag[e];
    T t = a - th;
    t = t > T(0) ? t : T(0);
    const T f = a > T(0) ? t / a : T(0);
    Cplx<T> c = z[e];
    c.re = c.re * f;
    c.im = c.im * f;
    z[e] = c;
  }
}
// z <- z .* mask: project_bounds! on a complex vector with binary bounds (project_bounds!.jl:27-36: x .= x .* UB)
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_cmask(long long N, Cplx<T>* __restrict__ z, const T* __restrict__ mask) {
  for (long long e = (long long)blockIdx.x * BLOCK + threadIdx.x; e < N; e += (long long)gridDim.x * BLOCK) {
    Cplx<T> c = z[e];
    c.re = c.re * mask[e];
    c.im = c.im * mask[e];
    z[e] = c;
  }
}
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_unpack_all(long long N, const Cplx<T>* __restrict__ z, T* __restrict__ v, T scale) {
  for (long long e = (long long)blockIdx.x * BLOCK + threadIdx.x; e < N; e += (long long)gridDim.x * BLOCK)
    v[e] = z[e].re * scale;
}
// v <- Re(z)/N -- skipped when v already lies inside the ball: F'F = I, so the reference's round trip
// A'*(A*x) (get_projector.jl:31) only adds FFT rounding noise there; v is returned bit for bit instead
// (the noise would otherwise be amplified by the BB rule: l = rho*(y - s) would be pure rounding error).
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_unpack(long long N, const Cplx<T>* __restrict__ z, T* __restrict__ v, T scale,
                                                  const ProjScalars<T>* __restrict__ ps) {
  if (!ps->need) return;
  for (long long e = (long long)blockIdx.x * BLOCK + threadIdx.x; e < N; e += (long long)gridDim.x * BLOCK)
    v[e] = z[e].re * scale;
}
// The same set through the REAL transform (round 4): the model is real, so the hipFFT R2C transform returns the nh1 = n1/2 + 1
// planes k1 = 0 .. n1/2 of the spectrum and the other n1 - nh1 are their conjugates -- half the transform, no packing.  The l1 norm
// runs over ALL N coefficients: the magnitudes of the stored ones fill mag[0, Nh), those of the planes 1 .. n1 - nh1 (whose
// conjugates are not stored) are written a second time behind them, N entries in all, and the search sees the vector it always saw.
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_cabs_half(long long Nh, int nh1, int ndup, const Cplx<T>* __restrict__ z, T* __restrict__ mag) {
  for (long long e = (long long)blockIdx.x * BLOCK + threadIdx.x; e < Nh; e += (long long)gridDim.x * BLOCK) {
    const T m = (T)hypot((double)z[e].re, (double)z[e].im);
    mag[e] = m;
    const long long row = e / nh1;
    const int k1 = (int)(e - row * nh1);
    if (k1 >= 1 && k1 <= ndup) mag[Nh + row * ndup + (k1 - 1)] = m;
  }
}
// v <- w * scale (w: the output of the C2R transform) unless v already lies inside the ball (see k_unpack)
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_unpack_real(long long N, const T* __restrict__ w, T* __restrict__ v, T scale,
                                                       const ProjScalars<T>* __restrict__ ps) {
  if (!ps->need) return;
  for (long long e = (long long)blockIdx.x * BLOCK + threadIdx.x; e < N; e += (long long)gridDim.x * BLOCK) v[e] = w[e] * scale;
}
// ------------------------------------------------------------------------------------------------
// Cardinality behind the DFT (EXT_CARD_DFT): keep the k Fourier coefficients of largest magnitude, x -> Re(F' (K .* F x))
//     reference: get_projector.jl:85-89 with A = joDFT, project_cardinality! on Complex{TF} (project_cardinality!.jl:3-21).
// The order is the stable one by descending |Z| on the natural column-major index e = k1 + n1 (k2 + n2 k3) of the full spectrum.
// For a real model |Z[e]| = |Z[e*]|, e* = the index with every coordinate negated modulo n: the magnitudes are TAKEN as exactly
// symmetric (max of the two where both are computed) and the tie goes to the lower index, where the reference leaves it to the
// rounding noise of its FFT.  A pair the cut separates keeps its lower-index member only; Re(F' .) of that is the inverse
// transform of the pair with weight 1/2 on both members -- in general Re(F'(K .* Z)) = F'(w .* Z), w[e] = (keep[e] + keep[e*]) / 2,
// which is Hermitian and is what the real transform is handed.  IT: unsigned below 2^31 entries (32-bit divisions), else long long.
template <typename IT>
struct DftIdx {
  IT n1, n2, n3, nh1;              // nh1 = n1/2 + 1: stored planes of the real transform
};
template <typename T>
__device__ __forceinline__ T cplx_abs(T re, T im);
template <>
__device__ __forceinline__ float cplx_abs<float>(float re, float im) {      // (the squares of floats are exact in double, their sum cannot overflow)
  const double r = (double)re, i = (double)im;
  return (float)sqrt(r * r + i * i);
}
template <>
__device__ __forceinline__ double cplx_abs<double>(double re, double im) { return hypot(re, im); }
// 16 bytes of spectrum: two Float32 bins or one Float64 bin
template <typename T> struct alignas(16) BinVec { Cplx<T> b[16 / sizeof(Cplx<T>)]; };
template <typename T>
__device__ __forceinline__ bool card_keeps(T m, long long e, T tau, long long cut) { return m > tau || (m == tau && e <= cut); }
// nothing is dropped (k >= N or k >= the non-zero coefficients, k_card_decide): v stays as it is, bit for bit
template <typename T>
__device__ __forceinline__ bool card_identity(const ProjScalars<T>* ps) { return !ps->need && ps->tau == T(0); }

// R2C route, pass 1: the N magnitudes in natural order from the Nh stored bins.  A stored bin (k1, row) writes its own entry and,
// where its conjugate is not stored (1 <= k1 <= n1 - nh1), the conjugate's; in the planes k1 = 0 and k1 = n1/2 (n1 even) both
// members of a pair are stored and each takes the larger of the two magnitudes.  Every entry of mag is written exactly once.
template <typename T, typename IT>
__global__ __launch_bounds__(BLOCK) void k_card_dft_mag_half(long long Nh, DftIdx<IT> d, const Cplx<T>* __restrict__ z, T* __restrict__ mag) {
  constexpr int V = 16 / (int)sizeof(Cplx<T>);
  const IT ndup = d.n1 - d.nh1;
  const long long nvec = (Nh + V - 1) / V;
  for (long long p = (long long)blockIdx.x * BLOCK + threadIdx.x; p < nvec; p += (long long)gridDim.x * BLOCK) {
    const long long h0 = p * V;
    BinVec<T> bv;
    if (h0 + V <= Nh) bv = *reinterpret_cast<const BinVec<T>*>(z + h0);
    else bv.b[0] = z[h0];                                  // (odd Nh in Float32: the last bin alone)
#pragma unroll
    for (int q = 0; q < V; ++q) {
      if (h0 + q >= Nh) break;
      const IT h = (IT)(h0 + q);
      const IT row = h / d.nh1, k1 = h - row * d.nh1;
      const IT k3 = row / d.n2, k2 = row - k3 * d.n2;
      const IT crow = (k2 ? d.n2 - k2 : 0) + d.n2 * (k3 ? d.n3 - k3 : 0);
      T m = cplx_abs<T>(bv.b[q].re, bv.b[q].im);
      const long long e = (long long)k1 + (long long)d.n1 * (long long)row;
      if (k1 >= 1 && k1 <= ndup) {
        mag[(long long)(d.n1 - k1) + (long long)d.n1 * (long long)crow] = m;
      } else {
        const Cplx<T> c = z[(long long)k1 + (long long)d.nh1 * (long long)crow];
        const T mp = cplx_abs<T>(c.re, c.im);
        m = mp > m ? mp : m;
      }
      mag[e] = m;
    }
  }
}
// R2C route, pass 2: every stored bin times w = (keep[e] + keep[e*]) / 2 in {0, 1/2, 1}; the partner's decision from the partner's
// index (mag[e*] == mag[e] by construction).  Partners inside the stored planes get the same weight, self-conjugate bins keep[e].
template <typename T, typename IT>
__global__ __launch_bounds__(BLOCK) void k_card_dft_weight_half(long long Nh, DftIdx<IT> d, Cplx<T>* __restrict__ z, const T* __restrict__ mag,
                                                                const ProjScalars<T>* __restrict__ ps) {
  if (card_identity(ps)) return;
  constexpr int V = 16 / (int)sizeof(Cplx<T>);
  const T tau = ps->tau;
  const long long cut = ps->quota;
  const long long nvec = (Nh + V - 1) / V;
  for (long long p = (long long)blockIdx.x * BLOCK + threadIdx.x; p < nvec; p += (long long)gridDim.x * BLOCK) {
    const long long h0 = p * V;
    const bool full = h0 + V <= Nh;
    BinVec<T> bv;
    if (full) bv = *reinterpret_cast<const BinVec<T>*>(z + h0);
    else bv.b[0] = z[h0];
#pragma unroll
    for (int q = 0; q < V; ++q) {
      if (h0 + q >= Nh) break;
      const IT h = (IT)(h0 + q);
      const IT row = h / d.nh1, k1 = h - row * d.nh1;
      const IT k3 = row / d.n2, k2 = row - k3 * d.n2;
      const IT crow = (k2 ? d.n2 - k2 : 0) + d.n2 * (k3 ? d.n3 - k3 : 0);
      const long long e = (long long)k1 + (long long)d.n1 * (long long)row;
      const long long ep = (long long)(k1 ? d.n1 - k1 : 0) + (long long)d.n1 * (long long)crow;
      const T m = mag[e];
      const T w = T(0.5) * ((card_keeps(m, e, tau, cut) ? T(1) : T(0)) + (card_keeps(m, ep, tau, cut) ? T(1) : T(0)));
      bv.b[q].re = bv.b[q].re * w;
      bv.b[q].im = bv.b[q].im * w;
    }
    if (full) *reinterpret_cast<BinVec<T>*>(z + h0) = bv;
    else z[h0] = bv.b[0];
  }
}
// Complex route (SIPX_DFT_REAL=0, n1 < 4), pass 1: mag[e] = max(|Z[e]|, |Z[e*]|) -- both members of a pair compute the same value
template <typename T, typename IT>
__global__ __launch_bounds__(BLOCK) void k_card_dft_mag_full(long long N, DftIdx<IT> d, const Cplx<T>* __restrict__ z, T* __restrict__ mag) {
  for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < N; i += (long long)gridDim.x * BLOCK) {
    const IT e = (IT)i;
    const IT row = e / d.n1, k1 = e - row * d.n1;
    const IT k3 = row / d.n2, k2 = row - k3 * d.n2;
    const IT crow = (k2 ? d.n2 - k2 : 0) + d.n2 * (k3 ? d.n3 - k3 : 0);
    const long long ep = (long long)(k1 ? d.n1 - k1 : 0) + (long long)d.n1 * (long long)crow;
    const Cplx<T> a = z[i], b = z[ep];
    const T ma = cplx_abs<T>(a.re, a.im), mb = cplx_abs<T>(b.re, b.im);
    mag[i] = mb > ma ? mb : ma;
  }
}
// Complex route, pass 2: Z[e] <- 0 unless kept, the (tau, index cut) rule on the N bins themselves
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_card_dft_keep_full(long long N, Cplx<T>* __restrict__ z, const T* __restrict__ mag,
                                                              const ProjScalars<T>* __restrict__ ps) {
  if (card_identity(ps)) return;
  const T tau = ps->tau;
  const long long cut = ps->quota;
  for (long long e = (long long)blockIdx.x * BLOCK + threadIdx.x; e < N; e += (long long)gridDim.x * BLOCK) {
    if (card_keeps(mag[e], e, tau, cut)) continue;
    Cplx<T> c;
    c.re = T(0);
    c.im = T(0);
    z[e] = c;
  }
}
// v <- w * scale (w: N reals with stride `ws` -- the output of C2R, or the real parts of the complex inverse) unless nothing was dropped
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_card_dft_unpack(long long N, const T* __restrict__ w, int ws, T* __restrict__ v, T scale,
                                                           const ProjScalars<T>* __restrict__ ps) {
  if (card_identity(ps)) return;
  for (long long e = (long long)blockIdx.x * BLOCK + threadIdx.x; e < N; e += (long long)gridDim.x * BLOCK) v[e] = w[e * ws] * scale;
}
static rocblas_status gemm_sb(rocblas_handle h, rocblas_operation ta, rocblas_operation tb, int m, int n, int k, const float* A,
                              int lda, long long sa, const float* B, int ldb, long long sb, float* C, int ldc, long long sc, int batch) {
  const float one = 1.f, zero = 0.f;
  return rocblas_sgemm_strided_batched(h, ta, tb, m, n, k, &one, A, lda, sa, B, ldb, sb, &zero, C, ldc, sc, batch);
}
static rocblas_status gemm_sb(rocblas_handle h, rocblas_operation ta, rocblas_operation tb, int m, int n, int k, const double* A,
                              int lda, long long sa, const double* B, int ldb, long long sb, double* C, int ldc, long long sc, int batch) {
  const double one = 1.0, zero = 0.0;
  return rocblas_dgemm_strided_batched(h, ta, tb, m, n, k, &one, A, lda, sa, B, ldb, sb, &zero, C, ldc, sc, batch);
}
// dst <- src when the last search found v outside the set (ps->need), or always when ps == nullptr
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_copy_if_needed(long long N, const T* __restrict__ src, T* __restrict__ dst,
                                                          const ProjScalars<T>* __restrict__ ps) {
  if (ps && !ps->need) return;
  for (long long e = (long long)blockIdx.x * BLOCK + threadIdx.x; e < N; e += (long long)gridDim.x * BLOCK) dst[e] = src[e];
}

// ---- hipFFT by the model's type: the entry points, the transform types and the plan of a grid ----
static void fft_c2c(hipfftHandle p, Cplx<float>* z, int dir) {
  fft_check(hipfftExecC2C(p, (hipfftComplex*)z, (hipfftComplex*)z, dir), dir == HIPFFT_FORWARD ? "forward" : "inverse");
}
static void fft_c2c(hipfftHandle p, Cplx<double>* z, int dir) {
  fft_check(hipfftExecZ2Z(p, (hipfftDoubleComplex*)z, (hipfftDoubleComplex*)z, dir), dir == HIPFFT_FORWARD ? "forward" : "inverse");
}
static void fft_r2c(hipfftHandle p, float* v, Cplx<float>* z) { fft_check(hipfftExecR2C(p, v, (hipfftComplex*)z), "forward (real)"); }
static void fft_r2c(hipfftHandle p, double* v, Cplx<double>* z) { fft_check(hipfftExecD2Z(p, v, (hipfftDoubleComplex*)z), "forward (real)"); }
static void fft_c2r(hipfftHandle p, Cplx<float>* z, float* w) { fft_check(hipfftExecC2R(p, (hipfftComplex*)z, w), "inverse (real)"); }
static void fft_c2r(hipfftHandle p, Cplx<double>* z, double* w) { fft_check(hipfftExecZ2D(p, (hipfftDoubleComplex*)z, w), "inverse (real)"); }
template <typename T> struct FftKind;
template <> struct FftKind<float> { static constexpr hipfftType c2c = HIPFFT_C2C, r2c = HIPFFT_R2C, c2r = HIPFFT_C2R; };
template <> struct FftKind<double> { static constexpr hipfftType c2c = HIPFFT_Z2Z, r2c = HIPFFT_D2Z, c2r = HIPFFT_Z2D; };
struct FftPlan {
  hipfftHandle h = 0;
  bool have = false;
  // the 2-D / 3-D transform of the grid (slowest dimension first) on stream s; `which` ends the name an error gives the plan
  void create(int ndim, const Grid& G, hipfftType type, const char* which, hipStream_t s) {
    if (ndim == 2) fft_check(hipfftPlan2d(&h, (int)G.n[1], (int)G.n[0], type), (std::string("plan2d") + which).c_str());
    else fft_check(hipfftPlan3d(&h, (int)G.n[2], (int)G.n[1], (int)G.n[0], type), (std::string("plan3d") + which).c_str());
    have = true;
    set_stream(s);
  }
  void set_stream(hipStream_t s) { if (have) fft_check(hipfftSetStream(h, s), "set stream"); }
  operator hipfftHandle() const { return h; }
  ~FftPlan() { if (have) (void)hipfftDestroy(h); }
};

// ---- DFT mask, l1 ball and cardinality behind the DFT ---------------------------------------------------------------------------
template <typename T>
struct DftProj;
// Cardinality behind the DFT: transform, the N symmetric magnitudes in natural order, the engine's own cardinality search on them
// ((tau, index cut) in ps), the weights on the stored bins, inverse transform.  The scale of the transform does not matter to the
// order, so the raw spectrum is searched; 1/N on the way back.
template <typename T, typename IT>
static void card_dft_project(DftProj<T>& I, T* v, bool feas, double* partials, T* maxpart, T* compact) {
  const Grid& G = I.sp.G;
  const long long N = G.N;
  hipStream_t s = I.stream;
  ProjScalars<T>* ps = I.search.pick(feas);
  DftIdx<IT> d;
  d.n1 = (IT)G.n[0]; d.n2 = (IT)G.n[1]; d.n3 = (IT)G.n[2]; d.nh1 = (IT)(G.n[0] / 2 + 1);
  const T k = (T)I.sp.pmax, scale = (T)(1.0 / (double)N);
  if (I.real_fft) {
    fft_r2c(I.plan_r2c, v, I.z);
    hipLaunchKernelGGL((k_card_dft_mag_half<T, IT>), dim3(NB), dim3(BLOCK), 0, s, I.Nh, d, I.z, I.mag);
    K<T>::proj_scalars_arr(s, N, I.mag, PX_CARD, T(0), k, ps, partials, maxpart, compact, N);
    hipLaunchKernelGGL((k_card_dft_weight_half<T, IT>), dim3(NB), dim3(BLOCK), 0, s, I.Nh, d, I.z, I.mag, ps);
    // (as for the l1 ball: the inverse real transform writes into mag, free by now, and v stays untouched when nothing is dropped)
    fft_c2r(I.plan_c2r, I.z, I.mag);
    hipLaunchKernelGGL((k_card_dft_unpack<T>), dim3(NB), dim3(BLOCK), 0, s, N, I.mag, 1, v, scale, ps);
  } else {
    hipLaunchKernelGGL((k_pack<T>), dim3(NB), dim3(BLOCK), 0, s, N, v, I.z);
    fft_c2c(I.plan, I.z, HIPFFT_FORWARD);
    hipLaunchKernelGGL((k_card_dft_mag_full<T, IT>), dim3(NB), dim3(BLOCK), 0, s, N, d, I.z, I.mag);
    K<T>::proj_scalars_arr(s, N, I.mag, PX_CARD, T(0), k, ps, partials, maxpart, compact, N);
    hipLaunchKernelGGL((k_card_dft_keep_full<T>), dim3(NB), dim3(BLOCK), 0, s, N, I.z, I.mag, ps);
    fft_c2c(I.plan, I.z, HIPFFT_BACKWARD);
    hipLaunchKernelGGL((k_card_dft_unpack<T>), dim3(NB), dim3(BLOCK), 0, s, N, (const T*)I.z, 2, v, scale, ps);
  }
}
template <typename T>
struct DftProj : ExtImpl<T> {
  using ExtImpl<T>::sp;
  using ExtImpl<T>::stream;
  FftPlan plan;                        // the complex transform of the packed model
  FftPlan plan_r2c, plan_c2r;          // the real transform (half the spectrum)
  bool real_fft = false;
  int nh1 = 0, ndup = 0;
  long long Nh = 0;
  Cplx<T>* z = nullptr;
  T* mag = nullptr;                    // the magnitudes; the mask of EXT_DFT_MASK
  SearchState<T> search;
  T radius_raw = 0;
  void set_stream(hipStream_t s) override {
    if (stream == s) return;
    stream = s;
    plan.set_stream(s); plan_r2c.set_stream(s); plan_c2r.set_stream(s);
  }
  void reset() override { search.reinit(stream); }
  DftProj(const ExtSpec& spec, hipStream_t s) : ExtImpl<T>(spec, s) {
    const Grid& G = sp.G;
    const long long N = G.N;
    const int kind = sp.kind;
    if (kind == EXT_DFT_MASK) {
      if (!sp.ub) throw std::runtime_error("bounds in the DFT domain need the mask vector (constraint.max)");
      plan.create(sp.ndim, G, FftKind<T>::c2c, "", s);
      z = this->template alloc<Cplx<T>>(N);
      mag = this->template alloc<T>(N);
      SIPX_HIP(hipMemcpy(mag, sp.ub, sizeof(T) * N, hipMemcpyHostToDevice));
      return;
    }
    if (kind == EXT_L1_DFT && !(sp.pmax > 0)) throw std::runtime_error("Radius of L1 ball is negative");
    if (kind == EXT_CARD_DFT && (sp.pmax < 0 || sp.pmax != std::floor(sp.pmax)))
      throw std::runtime_error("cardinality behind the DFT: k must be a non-negative integer");
    real_fft = env_knobs().dft_real && G.n[0] >= 4;      // SIPX_DFT_REAL=0: the complex transform of the packed model (A/B switch, tests)
    if (real_fft) {
      plan_r2c.create(sp.ndim, G, FftKind<T>::r2c, " (real)", s);
      plan_c2r.create(sp.ndim, G, FftKind<T>::c2r, " (real, inverse)", s);
      nh1 = (int)(G.n[0] / 2 + 1);
      ndup = (int)G.n[0] - nh1;
      Nh = (long long)nh1 * (N / G.n[0]);
      z = this->template alloc<Cplx<T>>(Nh);
    } else {
      plan.create(sp.ndim, G, FftKind<T>::c2c, "", s);
      z = this->template alloc<Cplx<T>>(N);
    }
    mag = this->template alloc<T>(N);
    search.build(this->mem, s, kind == EXT_CARD_DFT ? N : 0);     // cidx: the tie cut of the cardinality search
    radius_raw = (T)(sp.pmax * sqrt((double)N));         // ||F_unitary v||_1 <= b  <=>  ||FFT v||_1 <= b sqrt(N)
  }

  // x -> Re(F' (UB .* F x)); the unitary factors of F and F' cancel into 1/N
  void mask_project(T* v) {
    const long long N = sp.G.N;
    hipStream_t s = stream;
    hipLaunchKernelGGL((k_pack<T>), dim3(NB), dim3(BLOCK), 0, s, N, v, z);
    fft_c2c(plan, z, HIPFFT_FORWARD);
    hipLaunchKernelGGL((k_cmask<T>), dim3(NB), dim3(BLOCK), 0, s, N, z, mag);
    fft_c2c(plan, z, HIPFFT_BACKWARD);
    hipLaunchKernelGGL((k_unpack_all<T>), dim3(NB), dim3(BLOCK), 0, s, N, z, v, (T)(1.0 / (double)N));
  }
  // the l1 ball through the real transform (k_cabs_half)
  void l1_real_project(T* v, bool feas, double* partials, T* maxpart, T* compact) {
    const long long N = sp.G.N;
    hipStream_t s = stream;
    ProjScalars<T>* ps = search.pick(feas);
    fft_r2c(plan_r2c, v, z);
    hipLaunchKernelGGL((k_cabs_half<T>), dim3(NB), dim3(BLOCK), 0, s, Nh, nh1, ndup, z, mag);
    K<T>::proj_scalars_arr(s, N, mag, PX_L1, T(0), radius_raw, ps, partials, maxpart, compact, N);
    hipLaunchKernelGGL((k_csoft<T>), dim3(NB), dim3(BLOCK), 0, s, Nh, z, mag, ps);
    // (the inverse real transform may overwrite its input; its output goes through mag, free by now, so that v stays untouched
    //  when it already lies inside the ball)
    fft_c2r(plan_c2r, z, mag);
    hipLaunchKernelGGL((k_unpack_real<T>), dim3(NB), dim3(BLOCK), 0, s, N, mag, v, (T)(1.0 / (double)N), ps);
  }
  // the l1 ball through the complex transform of the packed model (SIPX_DFT_REAL=0, n1 < 4)
  void l1_complex_project(T* v, bool feas, double* partials, T* maxpart, T* compact) {
    const long long N = sp.G.N;
    hipStream_t s = stream;
    ProjScalars<T>* ps = search.pick(feas);
    hipLaunchKernelGGL((k_pack<T>), dim3(NB), dim3(BLOCK), 0, s, N, v, z);
    fft_c2c(plan, z, HIPFFT_FORWARD);
    hipLaunchKernelGGL((k_cabs<T>), dim3(NB), dim3(BLOCK), 0, s, N, z, mag);
    K<T>::proj_scalars_arr(s, N, mag, PX_L1, T(0), radius_raw, ps, partials, maxpart, compact, N);
    hipLaunchKernelGGL((k_csoft<T>), dim3(NB), dim3(BLOCK), 0, s, N, z, mag, ps);
    fft_c2c(plan, z, HIPFFT_BACKWARD);
    hipLaunchKernelGGL((k_unpack<T>), dim3(NB), dim3(BLOCK), 0, s, N, z, v, (T)(1.0 / (double)N), ps);
  }
  void project(T* v, bool feas, double* partials, T* maxpart, T* compact) override {
    if (sp.kind == EXT_DFT_MASK) mask_project(v);
    else if (sp.kind == EXT_L1_DFT && real_fft) l1_real_project(v, feas, partials, maxpart, compact);
    else if (sp.kind == EXT_L1_DFT) l1_complex_project(v, feas, partials, maxpart, compact);
    else if (sp.G.N < (1ll << 31)) card_dft_project<T, unsigned>(*this, v, feas, partials, maxpart, compact);
    else card_dft_project<T, long long>(*this, v, feas, partials, maxpart, compact);
    SIPX_HIP(hipGetLastError());
  }
};

// ---- DCT and DWT: one of the engine's projectors on the coefficient array ------------------------------------------------------
static Grid grid_1d(long long N) {
  Grid g;
  g.n[0] = N; g.n[1] = 1; g.n[2] = 1; g.N = N; g.st[0] = 1; g.st[1] = N; g.st[2] = N;
  return g;
}
template <typename T>
struct CoefProj : ExtImpl<T> {
  using ExtImpl<T>::sp;
  using ExtImpl<T>::stream;
  BlasHandle blas;                                 // DCT
  T* Cm[3] = {nullptr, nullptr, nullptr};          // DCT: the orthonormal DCT-II matrix of every dimension
  T *W1 = nullptr, *W2 = nullptr;                  // two work arrays (DWT: the coefficients in W1, W2 the transform's scratch)
  T *dlb = nullptr, *dub = nullptr;                // DCT with per-element bounds
  SearchState<T> search;
  void project(T* v, bool feas, double* partials, T* maxpart, T* compact) override {
    if (sp.kind == EXT_DCT) dct_project(v, feas, partials, maxpart, compact);
    else dwt_project(v, feas, partials, maxpart, compact);
    SIPX_HIP(hipGetLastError());
  }
  void set_stream(hipStream_t s) override {
    if (stream == s) return;
    stream = s;
    blas.set_stream(s);
  }
  void reset() override { search.reinit(stream); }
  CoefProj(const ExtSpec& spec, hipStream_t s) : ExtImpl<T>(spec, s) {
    const Grid& G = sp.G;
    const long long N = G.N;
    if (sp.kind == EXT_DCT) {
      // Orthonormal DCT-II along every dimension as dense n_d x n_d matrices (built in float64, rounded to TF once):
      // C[k, i] = s_k cos(pi (2i+1) k / (2n)), s_0 = sqrt(1/n), s_k = sqrt(2/n).  joDCT's normalisation is not pinned by any
      // reference test; orthonormal is assumed (the operator declares AtA_diag, get_TD_operator.jl:49-51,84-86).
      const double PI = 3.14159265358979323846;
      for (int a = 0; a < sp.ndim; ++a) {
        const int n = (int)G.n[a];
        std::vector<T> C((size_t)n * n);
        for (int i = 0; i < n; ++i)
          for (int k = 0; k < n; ++k)
            C[(size_t)i * n + k] = (T)((k == 0 ? std::sqrt(1.0 / n) : std::sqrt(2.0 / n)) * std::cos(PI * (2.0 * i + 1.0) * k / (2.0 * n)));
        Cm[a] = this->template alloc<T>((size_t)n * n);      // column-major n x n: element (k, i) at k + n i
        SIPX_HIP(hipMemcpy(Cm[a], C.data(), sizeof(T) * C.size(), hipMemcpyHostToDevice));
      }
    } else {
      dwt_check_grid(sp.ndim, G.n);                          // db4 wavelet transform (kernels_dwt.hip)
    }
    W1 = this->template alloc<T>(N);
    W2 = this->template alloc<T>(N);
    if (sp.kind == EXT_DCT) blas.create(s);
    const int in = sp.inner;
    if (in == SIPX_PROJ_L1 || in == SIPX_PROJ_CARDINALITY) search.build(this->mem, s, in == SIPX_PROJ_CARDINALITY ? N : 0);
    if (sp.kind == EXT_DCT && in == SIPX_PROJ_BOUNDS_VEC) {
      if (!sp.lb || !sp.ub) throw std::runtime_error("per-element bounds need lb and ub");
      dlb = this->template alloc<T>(N); dub = this->template alloc<T>(N);
      SIPX_HIP(hipMemcpy(dlb, sp.lb, sizeof(T) * N, hipMemcpyHostToDevice));
      SIPX_HIP(hipMemcpy(dub, sp.ub, sizeof(T) * N, hipMemcpyHostToDevice));
    }
  }

  // The inner projector on the coefficient array `cur`.  vec_bounds: the DCT's per-element bounds (dlb / dub) are honoured.  Returns the
  // search state where the transform back may be skipped -- inside the l1 ball the round trip through an orthonormal transform
  // only adds rounding noise, and v is kept bit for bit there (as for the DFT) -- else nullptr.
  const ProjScalars<T>* project_coefficients(T* cur, bool feas, double* partials, T* maxpart, T* compact, bool vec_bounds) {
    const long long N = sp.G.N;
    const int in = sp.inner;
    const bool two = in == SIPX_PROJ_L1 || in == SIPX_PROJ_CARDINALITY;
    ProjScalars<T>* ps = two ? search.pick(feas) : nullptr;
    if (two) K<T>::proj_scalars_arr(stream, N, cur, in, (T)sp.pmin, (T)sp.pmax, ps, partials, maxpart, compact, N);
    proj_apply_grid<T>(stream, grid_1d(N), 0, nullptr, N, cur, in, vec_bounds && in == SIPX_PROJ_BOUNDS_VEC ? T(0) : (T)sp.pmin, (T)sp.pmax,
                       dlb, dub, ps);
    return in == SIPX_PROJ_L1 ? ps : nullptr;
  }
  void dct_project(T* v, bool feas, double* partials, T* maxpart, T* compact) {
    const Grid& G = sp.G;
    const int n1 = (int)G.n[0], n2 = (int)G.n[1], n3 = (int)G.n[2];
    const auto N_ = rocblas_operation_none, T_ = rocblas_operation_transpose;
    const long long s12 = (long long)n1 * n2;
    // forward: coefficients = C1 X C2' (per z plane) ... C3' ; ping-pong between v / W1 / W2
    blas_check(gemm_T(blas, N_, N_, n1, n2 * n3, n1, Cm[0], n1, v, n1, W1, n1), "dct dim 1");
    T *cur = W1, *oth = W2;
    if (n2 > 1) {
      blas_check(gemm_sb(blas, N_, T_, n1, n2, n2, cur, n1, s12, Cm[1], n2, 0, oth, n1, s12, n3), "dct dim 2");
      std::swap(cur, oth);
    }
    if (n3 > 1) {
      blas_check(gemm_T(blas, N_, T_, (int)s12, n3, n3, cur, (int)s12, Cm[2], n3, oth, (int)s12), "dct dim 3");
      std::swap(cur, oth);
    }
    const ProjScalars<T>* unchanged = project_coefficients(cur, feas, partials, maxpart, compact, true);
    // inverse (transposed matrices, reverse order)
    if (n3 > 1) {
      blas_check(gemm_T(blas, N_, N_, (int)s12, n3, n3, cur, (int)s12, Cm[2], n3, oth, (int)s12), "idct dim 3");
      std::swap(cur, oth);
    }
    if (n2 > 1) {
      blas_check(gemm_sb(blas, N_, N_, n1, n2, n2, cur, n1, s12, Cm[1], n2, 0, oth, n1, s12, n3), "idct dim 2");
      std::swap(cur, oth);
    }
    blas_check(gemm_T(blas, T_, N_, n1, n2 * n3, n1, Cm[0], n1, cur, n1, oth, n1), "idct dim 1");
    hipLaunchKernelGGL((k_copy_if_needed<T>), dim3(NB), dim3(BLOCK), 0, stream, G.N, oth, v, unchanged);
  }
  void dwt_project(T* v, bool feas, double* partials, T* maxpart, T* compact) {
    dwt_forward<T>(stream, sp.ndim, sp.G.n, v, W1, W2);
    const ProjScalars<T>* unchanged = project_coefficients(W1, feas, partials, maxpart, compact, false);
    // inside the l1 ball every launch of the inverse returns at once; otherwise its last launch writes v
    dwt_inverse<T>(stream, sp.ndim, sp.G.n, W1, v, W2, unchanged);
  }
};

template <typename T>
ExtImpl<T>* make_transform_family(const ExtSpec& spec, hipStream_t stream) {
  if (spec.kind == EXT_DCT || spec.kind == EXT_DWT) return new CoefProj<T>(spec, stream);
  return new DftProj<T>(spec, stream);
}
template ExtImpl<float>* make_transform_family<float>(const ExtSpec&, hipStream_t);
template ExtImpl<double>* make_transform_family<double>(const ExtSpec&, hipStream_t);

}  // namespace sipx
