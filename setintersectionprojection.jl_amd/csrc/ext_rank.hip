// Rank and nuclear-norm projectors on the slices of a materialised vector v (a matrix: one slice).
//
//   slice / matrix rank  x[:,:,i] <- U_r S_r V_r'      reference: projectors/project_rank!.jl:3-48
//   nuclear norm ball    the singular values of every slice on the l1 ball      reference: project_nuclear!.jl
//       rocSOLVER batched decompositions + rocBLAS batched GEMM: the one unit of the path that is not
//       bandwidth bound, so it is a library call, not a hand-written kernel.
//   Float32 models go through the Gram matrices of the slices, and the rank projector warm-starts a filtered block subspace
//   iteration on them from the previous call's vectors (RankFamily::project); Float64 models keep the one-sided Jacobi SVD.
#include "ext_family.h"

#include <rocsolver/rocsolver.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>

namespace sipx {

// U[:, j] *= S[j] for the first r columns of every slice
template <typename T>
__global__ __launch_bounds__(BLOCK) void k_scale_cols(int m, int r, int ldu, long long strideU, long long strideS,
                                                      int batch, T* __restrict__ U, const T* __restrict__ S) {
  const long long tot = (long long)batch * r * m;
  for (long long e = (long long)blockIdx.x * BLOCK + threadIdx.x; e < tot; e += (long long)gridDim.x * BLOCK) {
    const int i = (int)(e % m);
    const long long t = e / m;
    const int j = (int)(t % r);
    const long long b = t / r;
    U[b * strideU + (long long)j * ldu + i] *= S[b * strideS + j];
  }
}
// ------------------------------------------------------------------------------------------------
// Singular values of every slice projected onto the l1 ball of radius sigma (project_nuclear!.jl:19-20,40-41 with
// project_l1_Duchi!.jl:23,40-46 on the descending values).  flag[b] = 1 when slice b changed.
__global__ void k_nuc_shrink(int kmin, int batch, double sigma, double* __restrict__ S, int* __restrict__ flag) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  double* s = S + (long long)b * kmin;
  double sum = 0;
  for (int j = 0; j < kmin; ++j) sum += s[j];
  if (sum <= sigma) {                       // norm(v, 1) <= b && return v
    flag[b] = 0;
    return;
  }
  int rho = 0;
  double cum = 0;
  for (;;) {                                // while u[rho+1] > (sv[rho+1] - b)/(rho+1) && rho+1 < lv
    const double nxt = cum + s[rho];
    if (s[rho] > (nxt - sigma) / (double)(rho + 1) && rho + 1 < kmin) {
      cum = nxt;
      ++rho;
    } else {
      break;
    }
  }
  if (rho == 0) { rho = 1; cum = s[0]; }    // rho = max(1, rho)
  double theta = (cum - sigma) / (double)rho;
  theta = theta > 0 ? theta : 0;
  for (int j = 0; j < kmin; ++j) {
    const double t = s[j] - theta;
    s[j] = t > 0 ? t : 0;
  }
  flag[b] = 1;
}

// Gram route (Float32 models): W = ascending eigenvalues of X'X (or XX'), sigma_j = sqrt(W_j).  F_j = shrunk(sigma_j)/sigma_j
// for the nuclear-norm ball (same scan as k_nuc_shrink on the descending values), flag[b] = 0 when slice b is inside it.
__global__ void k_nuc_factors(int kmin, int batch, double sigma, const double* __restrict__ W, double* __restrict__ F,
                              int* __restrict__ flag) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  const double* w = W + (long long)b * kmin;
  double* f = F + (long long)b * kmin;
  auto sv = [&](int j) {                     // j-th largest singular value
    const double l = w[kmin - 1 - j];
    return l > 0 ? sqrt(l) : 0.0;
  };
  double sum = 0;
  for (int j = 0; j < kmin; ++j) sum += sv(j);
  if (sum <= sigma) {
    flag[b] = 0;
    for (int j = 0; j < kmin; ++j) f[j] = 1.0;
    return;
  }
  int rho = 0;
  double cum = 0;
  for (;;) {
    const double nxt = cum + sv(rho);
    if (sv(rho) > (nxt - sigma) / (double)(rho + 1) && rho + 1 < kmin) {
      cum = nxt;
      ++rho;
    } else {
      break;
    }
  }
  if (rho == 0) { rho = 1; cum = sv(0); }
  double theta = (cum - sigma) / (double)rho;
  theta = theta > 0 ? theta : 0;
  for (int j = 0; j < kmin; ++j) {           // f is indexed like W (ascending)
    const double l = w[j], sg = l > 0 ? sqrt(l) : 0.0, t = sg - theta;
    f[j] = (sg > 0 && t > 0) ? t / sg : 0.0;
  }
  flag[b] = 1;
}
// Gs[:, j] = G[:, j] * F[j] for every slice (k x k eigenvector matrices)
__global__ __launch_bounds__(BLOCK) void k_scale_eigvecs(int k, int batch, const double* __restrict__ G, const double* __restrict__ F,
                                                         double* __restrict__ Gs) {
  const long long tot = (long long)batch * k * k;
  for (long long e = (long long)blockIdx.x * BLOCK + threadIdx.x; e < tot; e += (long long)gridDim.x * BLOCK) {
    const long long b = e / ((long long)k * k);
    const int j = (int)((e / k) % k);
    Gs[e] = G[e] * F[b * k + j];
  }
}

// ---- block subspace iteration on the Gram matrices (rank projection, see ExtProj::project) ----
// Columns of Y (k x b per matrix) scaled to unit length; a column that vanished against the largest one (rank of the
// matrix below b) is replaced by fixed pseudo-random numbers so that the Cholesky factor of Y'Y exists.
__global__ __launch_bounds__(BLOCK) void k_sub_normalize(int k, int b, int batch, double* __restrict__ Y) {
  __shared__ double sm[BLOCK / 64];
  __shared__ double s_norm[64];      // b <= 64 is enforced by the caller
  const int l = blockIdx.x;
  double* Yl = Y + (long long)l * k * b;
  for (int j = 0; j < b; ++j) {
    double a = 0;
    for (int i = threadIdx.x; i < k; i += BLOCK) a += Yl[(long long)j * k + i] * Yl[(long long)j * k + i];
    a = wave_sum(a);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = 0;
      for (int w = 0; w < BLOCK / 64; ++w) t += sm[w];
      s_norm[j] = sqrt(t);
    }
  }
  __syncthreads();
  double mx = 0;
  for (int j = 0; j < b; ++j) mx = s_norm[j] > mx ? s_norm[j] : mx;
  for (int j = 0; j < b; ++j) {
    const double nj = s_norm[j];
    if (nj > 1e-13 * mx && nj > 0) {
      const double inv = 1.0 / nj;
      for (int i = threadIdx.x; i < k; i += BLOCK) Yl[(long long)j * k + i] *= inv;
    } else {
      for (int i = threadIdx.x; i < k; i += BLOCK) {
        unsigned h = (unsigned)(i * 2654435761u) ^ (unsigned)((j + 1) * 40503u) ^ (unsigned)(l * 69069u);
        h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
        Yl[(long long)j * k + i] = ((double)(h >> 8) / 16777216.0 - 0.5) / sqrt((double)k / 12.0);
      }
    }
  }
}
// ||G_l||_F^2 of every matrix of the batch: FRO_PARTS workgroups per matrix, each over one contiguous part with four sums in
// flight per thread, then the parts added in order by k_sub_fro_sum -- the same bits for a matrix whatever the batch it sits in.
// (One workgroup per matrix with one dependent sum per thread, rounds 3-5: 0.97 ms for 512 Gram matrices of 512^2 -- 1.1 TB/s --
//  and 0.40 ms for the 64 of a rank's share, once per call.)
#define FRO_PARTS 16
__global__ __launch_bounds__(BLOCK) void k_sub_fro_part(int k, const double* __restrict__ G, double* __restrict__ part) {
  __shared__ double sm[BLOCK / 64];
  const long long kk = (long long)k * k, seg = (kk + FRO_PARTS - 1) / FRO_PARTS;
  const long long l = blockIdx.x / FRO_PARTS, p = blockIdx.x % FRO_PARTS;
  const double* Gl = G + l * kk;
  const long long s0 = p * seg, s1 = s0 + seg < kk ? s0 + seg : kk;
  double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
  long long i = s0 + threadIdx.x;
  for (; i + 3 * BLOCK < s1; i += 4 * BLOCK) {
    const double v0 = Gl[i], v1 = Gl[i + BLOCK], v2 = Gl[i + 2 * BLOCK], v3 = Gl[i + 3 * BLOCK];
    a0 += v0 * v0; a1 += v1 * v1; a2 += v2 * v2; a3 += v3 * v3;
  }
  for (; i < s1; i += BLOCK) a0 += Gl[i] * Gl[i];
  double a = wave_sum((a0 + a1) + (a2 + a3));
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0;
    for (int w = 0; w < BLOCK / 64; ++w) t += sm[w];
    part[blockIdx.x] = t;
  }
}
__global__ void k_sub_fro_sum(int batch, const double* __restrict__ part, double* __restrict__ fro2, unsigned long long* res) {
  const int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= batch) return;
  double t = 0;
  for (int p = 0; p < FRO_PARTS; ++p) t += part[(long long)l * FRO_PARTS + p];
  fro2[l] = t;
  if (res) atomicMax(res + 7, (unsigned long long)__double_as_longlong(t));      // t >= 0: the bit patterns order like the values
}
static void sub_fro(hipStream_t s, int k, int batch, const double* G, double* part, double* fro2, unsigned long long* res = nullptr) {
  hipLaunchKernelGGL(k_sub_fro_part, dim3((unsigned)batch * FRO_PARTS), dim3(BLOCK), 0, s, k, G, part);
  hipLaunchKernelGGL(k_sub_fro_sum, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, s, batch, part, fro2, res);
}
// A start for a projector that has none (the first call of a solve; project_rank!.jl:26-45 has no state at all): fixed
// pseudo-random columns, the same hash as the re-seeded columns of k_sub_normalize.
__global__ __launch_bounds__(BLOCK) void k_sub_seed(int k, int b, int batch, double* __restrict__ X) {
  const long long per = (long long)k * b, total = per * batch;
  for (long long e = (long long)blockIdx.x * BLOCK + threadIdx.x; e < total; e += (long long)gridDim.x * BLOCK) {
    const long long l = e / per, o = e - l * per;
    const int j = (int)(o / k), i = (int)(o - (long long)j * k);
    unsigned h = (unsigned)(i * 2654435761u) ^ (unsigned)((j + 1) * 40503u) ^ (unsigned)((unsigned)l * 69069u);
    h ^= h >> 15; h *= 2246822519u; h ^= h >> 13; h *= 3266489917u; h ^= h >> 16;
    X[e] = ((double)(h >> 8) / 16777216.0 - 0.5) / sqrt((double)k / 12.0);
  }
}
// Largest residual of the top-r Ritz pairs, relative to the largest Ritz value: max_j ||(G Q) z_j - theta_j x_j|| / theta_max,
// with ZH = (G Q) Z and X = Q Z given (k x b per matrix, Ritz values ascending).  res[0] collects the maximum over the
// batch (bit pattern of a non-negative double), res[1] is raised when a factorisation failed or a value is not finite.
// eps_bw > 0 (Float32 models, round 5): the residual of pair j is measured against what a backward stable Float32 SVD of the slice
// X itself leaves -- project_rank!.jl:28-41 calls svd() in TF.  With theta = x'Gx the residual rho = G x - theta x is orthogonal to
// x, and (sigma, u = X x / sigma, x) is an EXACT singular triplet of X + E with E = -u rho' / sigma, ||E||_2 = ||rho|| / sigma_j: the
// pair is accepted when that is at most eps_bw ||X||_2, i.e. ||rho_j|| <= eps_bw sqrt(theta_max theta_j).  What is stored and compared
// with tol everywhere (the host's decisions, k_cheb_plan, k_sub_list) is the residual in units of its acceptance level times tol,
// never asking for more than the strict level tol theta_max; res[6] <- the largest residual / theta_max as before (what a start is
// judged by).
__global__ __launch_bounds__(BLOCK) void k_sub_residual(int k, int b, int r, int batch, const double* __restrict__ ZH,
                                                        const double* __restrict__ X, const double* __restrict__ W, int ldw,
                                                        const rocblas_int* __restrict__ info_chol,
                                                        const rocblas_int* __restrict__ info_eig,
                                                        const double* __restrict__ fro2, unsigned long long* res,
                                                        double* __restrict__ per_matrix = nullptr, double eps_bw = 0.0,
                                                        double tol = 1e-12) {
  __shared__ double sm[BLOCK / 64];
  const int l = blockIdx.x;
  const double tmax = W[(long long)l * ldw + b - 1];
  if (fro2[l] == 0.0) {               // a slice of zeros (the first iteration of a solve projects v = 0): nothing to find, nothing to certify
    if (threadIdx.x == 0 && per_matrix) per_matrix[l] = 0.0;
    return;
  }
  double worst = 0, worst_raw = 0;
  for (int j = b - r; j < b; ++j) {
    const double th = W[(long long)l * ldw + j];
    const double* z = ZH + ((long long)l * b + j) * k;
    const double* x = X + ((long long)l * b + j) * k;
    double a = 0;
    for (int i = threadIdx.x; i < k; i += BLOCK) {
      const double d = z[i] - th * x[i];
      a += d * d;
    }
    a = wave_sum(a);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = a;
    __syncthreads();
    double t = 0;
    for (int w = 0; w < BLOCK / 64; ++w) t += sm[w];
    const double raw = sqrt(t) / tmax;
    double rel = raw;
    if (eps_bw > 0.0) {
      const double lvl = eps_bw * sqrt(tmax * (th > 0.0 ? th : 0.0));
      if (lvl > tol * tmax) rel = sqrt(t) / lvl * tol;
    }
    worst = rel > worst ? rel : worst;
    worst_raw = raw > worst_raw ? raw : worst_raw;
  }
  if (threadIdx.x == 0 && per_matrix) per_matrix[l] = worst;
  if (threadIdx.x == 0) {
    // Certificate that no eigenvalue above the r-th Ritz value hides outside the converged pairs.  With P the projector
    // on the subspace, ||G||_F^2 = ||H||_F^2 + 2 ||(I-P) G P||_F^2 + ||(I-P) G (I-P)||_F^2 and ||H||_F^2 = sum of the
    // squared Ritz values, so rest = ||G||_F^2 - sum theta^2 bounds both the coupling (<= sqrt(rest/2)) and everything
    // in the complement (<= sqrt(rest)).  Once the top-r pairs are eigenpairs, the other eigenvalues of G are those of the
    // block [guard Ritz part, coupling; coupling', complement] <= max(theta_{r+1}, sqrt(rest)) + sqrt(rest/2).
    double ritz2 = 0;
    for (int j = 0; j < b; ++j) ritz2 += W[(long long)l * ldw + j] * W[(long long)l * ldw + j];
    const double rest = fmax(fro2[l] - ritz2, 0.0) + 1e-12 * fro2[l];
    const double others = fmax(W[(long long)l * ldw + b - r - 1], sqrt(rest)) + sqrt(0.5 * rest);
    const bool hidden = !(others < W[(long long)l * ldw + b - r]);
    const unsigned long long bad = (info_chol[l] != 0 ? 1ull : 0ull) | (info_eig[l] != 0 ? 2ull : 0ull) | (!(tmax > 0) ? 4ull : 0ull) |
                                   ((!(worst == worst) || isinf(worst)) ? 8ull : 0ull) | (hidden ? 16ull : 0ull);
    if (bad & 15ull) atomicOr(res + 1, bad);     // 1: Cholesky, 2: Ritz solver, 4: no positive Ritz value, 8: not finite
    else {
      if (hidden) atomicOr(res + 1, 16ull);      // 16: not certified (yet): fine while the residual is still above the tolerance
      atomicMax(res, (unsigned long long)__double_as_longlong(worst));
      atomicMax(res + 6, (unsigned long long)__double_as_longlong(worst_raw));
    }
  }
}
// ---- Chebyshev-filtered subspace iteration (rank projection on spectra without a gap behind the block) ----
// Column j of the block carries its own damped interval [0, a_j], a_j = max(a, theta_j / CHEB_KAPPA), a = the end of the part of
// the spectrum the block does not hold: everything outside the block (eigenvalues <= a) is damped in every column, the
// column's own direction grows like T_m(2 theta_j / a_j - 1).  Directions whose Ritz value exceeds CHEB_KAPPA max(theta_j, a)
// would outgrow column j by (theta_i / a_j)^m -- the constant part of a velocity slice is 1e5 times the rest -- so they are
// projected out of the product G y_j at every step (k_cheb_mask: the filter then runs in the compression of G onto their
// complement, whose spectrum has lost them up to the square of their error).  The Rayleigh-Ritz step behind the filter works
// on the whole block again.
#define CHEB_KAPPA 2.0
// a = the Ritz value of guard column g (a few columns above the lowest; the g columns below it are not filtered), not the
// lowest: the lowest Ritz values of a block that has not converged lie below eigenvalues the block does not hold, and what
// lies above a is amplified -- an interval 5 % short loses a factor T_m(1.1) (250 at degree 14) of the contraction, one 5 %
// long about 10.  And never below 0.9 of the (r+1)-th Ritz value: a guard column that had to be re-seeded (k_chol_inv) carries
// a Rayleigh quotient from the middle of the spectrum, far below the block's true lower end.
__device__ double g_cheb_floor_factor = 0.9;      // the interval never ends below this share of the (r+1)-th Ritz value
__device__ __forceinline__ double cheb_floor(const double* __restrict__ W, int b, int g, int r) {
  const double top = W[b - 1];
  double a = W[g];
  const double lo = g_cheb_floor_factor * W[b - r - 1];
  a = a > lo ? a : lo;
  return a > 1e-14 * top ? a : 1e-14 * top;      // a block deeper than the rank of the matrix: no interval of zero width
}
// C (nl x b per matrix, leading dimension b) = X_L' Z for the nl last (largest) Ritz vectors: keep entry (i, j) only where
// vector i is far above column j
__global__ void k_cheb_mask(int b, int g, int r, int nl, int batch, const double* __restrict__ W, double* __restrict__ C) {
  const long long per = (long long)nl * b, total = per * batch;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const long long l = e / per;
    const int o = (int)(e - l * per), j = o / nl, i = b - nl + (o - j * nl);
    const double* Wl = W + l * b;
    const double a = cheb_floor(Wl, b, g, r);
    const double tj = Wl[j] > a ? Wl[j] : a;
    if (!(Wl[i] > CHEB_KAPPA * tj)) C[l * (long long)b * b + (long long)j * b + (o - j * nl)] = 0.0;
  }
}
// One step of the three-term recurrence, per column scalars: first = 1: out = (2/a_j) Z - Y0;  else out = (4/a_j) Z - 2 Y1 - Y0
// (out may alias Z or Y0: every entry is read before it is written, by the same thread)
__global__ __launch_bounds__(BLOCK) void k_cheb_step(int k, int b, int g, int r, int batch, const double* __restrict__ W, const double* Z,
                                                     const double* Y1, const double* Y0, double* out, int first) {
  const long long per = (long long)k * b, total = per * batch;
  for (long long e = (long long)blockIdx.x * BLOCK + threadIdx.x; e < total; e += (long long)gridDim.x * BLOCK) {
    const long long l = e / per;
    const int j = (int)((e - l * per) / k);
    const double* Wl = W + l * b;
    const double a = cheb_floor(Wl, b, g, r);
    const double aj = Wl[j] / CHEB_KAPPA > a ? Wl[j] / CHEB_KAPPA : a;
    // no positive Ritz value -- a slice of zeros among others: there is no interval, (2 / 0) * 0 would fill the block with NaN that
    // k_sub_residual never looks at and the final product turns into the slice's output.  The block stays what it is.
    if (!(aj > 0.0)) { out[e] = first ? Y0[e] : Y1[e]; continue; }
    out[e] = first ? (2.0 / aj) * Z[e] - Y0[e] : (4.0 / aj) * Z[e] - 2.0 * Y1[e] - Y0[e];
  }
}
// The same step with the projection inside, for the common case that only the nl <= 2 largest Ritz vectors are far above
// anything (a velocity slice: its constant part): one wave per column, z_j - x_i (x_i' z_j) for the masked i, then the recurrence.
// Replaces two skinny GEMMs, the mask kernel and k_cheb_step by one launch.
__global__ __launch_bounds__(256) void k_cheb_step_proj(int k, int b, int g, int r, int nl, int batch, const double* __restrict__ W,
                                                        const double* __restrict__ X, const double* Z, const double* Y1, const double* Y0,
                                                        double* out, int first) {
  const long long col = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);       // (matrix, column) pairs, one per wave
  if (col >= (long long)b * batch) return;
  const int lane = threadIdx.x & 63;
  const long long l = col / b;
  const int j = (int)(col - l * b);
  const double* Wl = W + l * b;
  const double a = cheb_floor(Wl, b, g, r);
  const double tj = Wl[j] > a ? Wl[j] : a;
  const double aj = Wl[j] / CHEB_KAPPA > a ? Wl[j] / CHEB_KAPPA : a;
  const long long base = l * (long long)k * b + (long long)j * k;
  double c0 = 0, c1 = 0;
  const bool m0 = nl >= 1 && Wl[b - 1] > CHEB_KAPPA * tj, m1 = nl >= 2 && Wl[b - 2] > CHEB_KAPPA * tj;
  const double* x0 = X + l * (long long)k * b + (long long)(b - 1) * k;
  const double* x1 = X + l * (long long)k * b + (long long)(b - 2) * k;
  if (m0 || m1) {
    for (int i = lane; i < k; i += 64) {
      const double z = Z[base + i];
      if (m0) c0 += x0[i] * z;
      if (m1) c1 += x1[i] * z;
    }
    c0 = wave_sum(c0);
    c1 = wave_sum(c1);
  }
  for (int i = lane; i < k; i += 64) {
    double z = Z[base + i];
    if (m0) z -= x0[i] * c0;
    if (m1) z -= x1[i] * c1;
    if (!(aj > 0.0)) { out[base + i] = first ? Y0[base + i] : Y1[base + i]; continue; }      // (a slice of zeros: see k_cheb_step)
    out[base + i] = first ? (2.0 / aj) * z - Y0[base + i] : (4.0 / aj) * z - 2.0 * Y1[base + i] - Y0[base + i];
  }
}
// Cholesky QR without the triangular solve: M = Y'Y (b x b, b <= 64, column-major, both triangles) -> Rinv, the inverse of
// the factor R of M = R'R, so that Q = Y Rinv is one GEMM.  One workgroup per matrix, everything in LDS; the columns are
// scaled to unit length first (M' = D^-1 M D^-1), which is what keeps the factorisation of a filtered block -- columns of
// very different length -- accurate.  info[l] is WRITTEN only on failure (a pivot that is not a number), so that two passes
// can share it.
__global__ __launch_bounds__(256) void k_chol_inv(int b, int batch, const double* __restrict__ M, double* __restrict__ Rinv,
                                                  rocblas_int* __restrict__ info) {
  __shared__ double A[64 * 65];
  __shared__ double Bv[64 * 65];
  __shared__ double dsc[64];
  const int l = blockIdx.x, t = threadIdx.x;
  const double* Ml = M + (long long)l * b * b;
  double* Rl = Rinv + (long long)l * b * b;
  if (t < b) {
    const double dj = Ml[(long long)t * b + t];
    dsc[t] = dj > 0 ? 1.0 / sqrt(dj) : 0.0;
  }
  __syncthreads();
  for (int e = t; e < b * b; e += 256) {
    const int i = e % b, c = e / b;
    if (i <= c) A[i * 65 + c] = Ml[(long long)c * b + i] * dsc[i] * dsc[c];
    Bv[i * 65 + c] = 0.0;
  }
  bool lost = false;
  for (int j = 0; j < b; ++j) {
    __syncthreads();
    const double piv = A[j * 65 + j];
    if (!(piv == piv)) { lost = true; break; }             // the same value in every thread: a uniform exit
    // a column that depends on the ones before it to rounding (a guard vector the filter left nothing of): it is dropped --
    // unit pivot, no coupling -- and comes back as a vector of negligible length, a Ritz value near zero at the low end
    const bool dep = !(piv > 1e-13);
    const double inv = dep ? 0.0 : 1.0 / sqrt(piv);
    __syncthreads();
    if (t == 0) A[j * 65 + j] = dep ? 1.0 : sqrt(piv);
    for (int c = j + 1 + t; c < b; c += 256) A[j * 65 + c] *= inv;
    __syncthreads();
    const int nrem = b - j - 1;
    for (int e = t; e < nrem * nrem; e += 256) {
      const int ii = e / nrem, cc = e - ii * nrem;
      if (cc >= ii) A[(j + 1 + ii) * 65 + j + 1 + cc] -= A[j * 65 + j + 1 + ii] * A[j * 65 + j + 1 + cc];
    }
  }
  __syncthreads();
  if (lost) {
    if (t == 0) info[l] = 1;
    for (int e = t; e < b * b; e += 256) Rl[e] = (e % b == e / b) ? 1.0 : 0.0;
    return;
  }
  if (t < b) {                                               // column t of the inverse of the (scaled) factor, back substitution
    const int c = t;
    Bv[c * 65 + c] = 1.0 / A[c * 65 + c];
    for (int i = c - 1; i >= 0; --i) {
      double acc = 0;
      for (int q = i + 1; q <= c; ++q) acc += A[i * 65 + q] * Bv[q * 65 + c];
      Bv[i * 65 + c] = -acc / A[i * 65 + i];
    }
  }
  __syncthreads();
  for (int e = t; e < b * b; e += 256) {
    const int i = e % b, c = e / b;
    Rl[e] = i <= c ? Bv[i * 65 + c] * dsc[i] : 0.0;
  }
}
// The b x b Ritz problem (b <= 64): cyclic two-sided Jacobi with the round-robin ordering -- b/2 disjoint rotations per step,
// first from the right (columns of H and of the accumulated V), then from the left (rows of H) -- one workgroup per matrix,
// H and V in LDS.  Sweeps until the off-diagonal mass is below 1e-30 of ||H||_F^2 (15 at most).  Eigenvalues ascending in W,
// eigenvectors in the columns of S (column-major, leading dimension b; S may be H itself).  rocSOLVER's syevj takes 2.5 ms for
// 512 problems of 48 x 48, most of it launches; this kernel about a fifth.  (Round 4: the two passes of a step as one pass over
// 2 x 2 blocks, loads staged in front of the stores -- the same operations in the same order, the same bits: 1.5 -> 0.9 ms for 512
// problems of 56 x 56, 5-7 sweeps.)
__global__ __launch_bounds__(256) void k_ritz_jacobi(int b, int batch, const double* H_in, double* S, double* __restrict__ W,
                                                     rocblas_int* __restrict__ info, rocblas_int* __restrict__ nsweeps = nullptr) {
  __shared__ double H[64 * 65];
  __shared__ double V[64 * 65];
  __shared__ double rc[32], rs[32];
  __shared__ int rp[32], rq[32];
  __shared__ double red[4];
  __shared__ double s_off, s_fro;
  const int l = blockIdx.x, t = threadIdx.x;
  const double* Hl = H_in + (long long)l * b * b;
  const int n = b + (b & 1), half = n / 2;
  for (int e = t; e < n * n; e += 256) {
    const int i = e % n, c = e / n;
    // the upper triangle is what the GEMM before filled reliably symmetric to rounding: mirror it (an odd b is padded by a
    // row and a column of zeros: the rotations that involve the pad are the identity, its entries stay zero)
    H[i * 65 + c] = (i < b && c < b) ? (i <= c ? Hl[(long long)c * b + i] : Hl[(long long)i * b + c]) : 0.0;
    V[i * 65 + c] = i == c ? 1.0 : 0.0;
  }
  auto block_sum = [&](double v) -> double {
    v = wave_sum(v);
    __syncthreads();
    if ((t & 63) == 0) red[t >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
  };
  __syncthreads();
  {
    double f = 0;
    for (int e = t; e < b * b; e += 256) { const double h = H[(e % b) * 65 + e / b]; f += h * h; }
    f = block_sum(f);
    if (t == 0) s_fro = f;
  }
  int sweeps = 0;
  bool done = false;
  for (; sweeps < 15 && !done; ++sweeps) {
    for (int step = 0; step < n - 1; ++step) {
      __syncthreads();
      if (t < half) {
        int p, q;
        if (t == 0) { p = n - 1; q = step; }
        else {                                 // (step + t) and (step - t) modulo n - 1; t < n - 1
          p = step + t; if (p >= n - 1) p -= n - 1;
          q = step - t; if (q < 0) q += n - 1;
        }
        if (p > q) { const int x = p; p = q; q = x; }
        double c = 1.0, sn = 0.0;
        if (q < b) {
          const double hpq = H[p * 65 + q];
          if (hpq != 0.0) {
            const double tau = (H[q * 65 + q] - H[p * 65 + p]) / (2.0 * hpq);
            const double tt = tau >= 0 ? 1.0 / (tau + sqrt(1.0 + tau * tau)) : 1.0 / (tau - sqrt(1.0 + tau * tau));
            c = 1.0 / sqrt(1.0 + tt * tt);
            sn = tt * c;
          }
        }
        rp[t] = p; rq[t] = q; rc[t] = c; rs[t] = sn;
      }
      __syncthreads();
      // H <- J' (H J), one thread per 2 x 2 block (row pair i, column pair j): the column rotation of the block's two rows, then
      // the row rotation of its two columns -- the operations of a column pass followed by a row pass, in their order, without
      // the barrier between the passes and with half the LDS traffic.  Operands of all of a thread's blocks are loaded before
      // any is stored (the blocks are disjoint, which the compiler cannot know: it would wait for every store).
      {
        double h00[4], h01[4], h10[4], h11[4], c1[4], s1[4], c2[4], s2[4];
        int a00[4], a01[4], a10[4], a11[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int it = t + 256 * k;
          if (it < half * half) {
            const int i = it / half, j = it - i * half;
            const int p1 = rp[i], q1 = rq[i], p2 = rp[j], q2 = rq[j];
            c1[k] = rc[i]; s1[k] = rs[i]; c2[k] = rc[j]; s2[k] = rs[j];
            a00[k] = p1 * 65 + p2; a01[k] = p1 * 65 + q2; a10[k] = q1 * 65 + p2; a11[k] = q1 * 65 + q2;
            h00[k] = H[a00[k]]; h01[k] = H[a01[k]]; h10[k] = H[a10[k]]; h11[k] = H[a11[k]];
          }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int it = t + 256 * k;
          if (it < half * half) {
            const double r0 = c2[k] * h00[k] - s2[k] * h01[k], r1 = s2[k] * h00[k] + c2[k] * h01[k];       // row p1 after H J
            const double u0 = c2[k] * h10[k] - s2[k] * h11[k], u1 = s2[k] * h10[k] + c2[k] * h11[k];       // row q1 after H J
            H[a00[k]] = c1[k] * r0 - s1[k] * u0;
            H[a10[k]] = s1[k] * r0 + c1[k] * u0;
            H[a01[k]] = c1[k] * r1 - s1[k] * u1;
            H[a11[k]] = s1[k] * r1 + c1[k] * u1;
          }
        }
      }
      {                                                     // V <- V J, staged the same way
        double vp[8], vq[8], cc[8], ss[8];
        int ap[8], aq[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const int it = t + 256 * k;
          ap[k] = -1;
          if (it < half * b) {
            const int i = it / b, e = it - i * b;
            const int p = rp[i], q = rq[i];
            if (q < b) {
              cc[k] = rc[i]; ss[k] = rs[i];
              ap[k] = e * 65 + p; aq[k] = e * 65 + q;
              vp[k] = V[ap[k]]; vq[k] = V[aq[k]];
            }
          }
        }
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (ap[k] >= 0) {
            V[ap[k]] = cc[k] * vp[k] - ss[k] * vq[k];
            V[aq[k]] = ss[k] * vp[k] + cc[k] * vq[k];
          }
      }
    }
    __syncthreads();
    double off = 0;
    for (int e = t; e < b * b; e += 256) {
      const int i = e % b, c = e / b;
      if (i != c) { const double h = H[i * 65 + c]; off += h * h; }
    }
    off = block_sum(off);
    if (t == 0) s_off = off;
    __syncthreads();
    done = !(s_off > 1e-30 * s_fro);
  }
  __syncthreads();
  if (t == 0) info[l] = (done && s_fro == s_fro) ? 0 : 1;
  if (t == 0 && nsweeps) nsweeps[l] = sweeps;
  if (t < b) {                                               // ascending order: the rank of every eigenvalue
    const double mine = H[t * 65 + t];
    int pos = 0;
    for (int j = 0; j < b; ++j) {
      const double o = H[j * 65 + j];
      pos += (o < mine || (o == mine && j < t)) ? 1 : 0;
    }
    W[(long long)l * b + pos] = mine;
    // column t of V becomes column pos of S
    double* Sl = S + (long long)l * b * b + (long long)pos * b;
    for (int i = 0; i < b; ++i) Sl[i] = V[i * 65 + t];
  }
}
// (Round 5, measured and dropped: the same solver with ONE WAVE per matrix -- no workgroup barriers, three workgroups per CU, the 2 x 2
//  blocks of a step walked four per lane -- gives the same bits and takes TWICE as long: 512 problems of 56 x 56 in a C4 iteration
//  59.9 against 49.8 ms per iteration, a 64-slice share 25.4 against 12.3 ms.  The step's LDS round trips are latency, and 64 lanes
//  queue twelve of them behind each other where 256 threads queue four.)
// What the host needs to choose the next filter: res[2] <- min over the batch of t_r = 2 theta_r / a - 1 (bit pattern of a
// positive double, start from +inf), res[3] <- max over the batch of the number of Ritz vectors far above the lowest column
// -- both over the matrices whose residual (per_matrix, k_sub_residual) is still above tol: the others are not what the next
// filter is for (res[3]); res[5] <- the count of far-above vectors over ALL matrices (a filter that runs on the whole batch must
// project for the converged ones too: their vectors would lose what they have to a direction 1e5 times larger)
__global__ void k_cheb_plan(int b, int g, int r, int batch, const double* __restrict__ W, const double* __restrict__ per_matrix, double tol,
                            unsigned long long* res) {
  const int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= batch) return;
  const double* Wl = W + (long long)l * b;
  const double a = cheb_floor(Wl, b, g, r);
  int nl = 0;
  for (int i = 0; i < b; ++i) nl += Wl[i] > CHEB_KAPPA * a ? 1 : 0;
  atomicMax(res + 5, (unsigned long long)nl);
  if (!(per_matrix[l] > tol)) return;
  double t = 2.0 * Wl[b - r] / a - 1.0;
  if (!(t > 1.0)) t = 1.0;
  atomicMin(res + 2, (unsigned long long)__double_as_longlong(t));
  atomicMax(res + 3, (unsigned long long)nl);
}
// The matrices whose residual is still above tol, in ascending order -> idx, their number -> res[4] (one workgroup).
__global__ __launch_bounds__(256) void k_sub_list(int batch, const double* __restrict__ per_matrix, double tol, int* __restrict__ idx,
                                                  unsigned long long* res) {
  __shared__ int cnt[256];
  const int t = threadIdx.x;
  const int chunk = (batch + 255) / 256, lo = t * chunk, hi = lo + chunk < batch ? lo + chunk : batch;
  int c = 0;
  for (int l = lo; l < hi; ++l) c += per_matrix[l] > tol ? 1 : 0;
  cnt[t] = c;
  __syncthreads();
  int base = 0;
  for (int j = 0; j < t; ++j) base += cnt[j];
  for (int l = lo; l < hi; ++l)
    if (per_matrix[l] > tol) idx[base++] = l;
  if (t == 255) res[4] = (unsigned long long)base;
}
// dst[j] <- src[idx[j]] (gather) or dst[idx[j]] <- src[j] (scatter), `per` values per matrix
__global__ __launch_bounds__(BLOCK) void k_sub_move(long long per, int n, const int* __restrict__ idx, const double* __restrict__ src,
                                                    double* __restrict__ dst, int scatter) {
  const long long total = per * n;
  for (long long e = (long long)blockIdx.x * BLOCK + threadIdx.x; e < total; e += (long long)gridDim.x * BLOCK) {
    const long long j = e / per, o = e - j * per;
    if (scatter) dst[(long long)idx[j] * per + o] = src[e];
    else dst[e] = src[(long long)idx[j] * per + o];
  }
}
// Inertia certificate for a converged top-r block on a spectrum too flat for the energy bound of k_sub_residual:
// B = mu I - G + X_r Theta_r X_r' is positive definite (its Cholesky factorisation exists) exactly when G, with the r found
// pairs removed, has no eigenvalue above mu; mu = the middle of the gap between the r-th and the (r+1)-th Ritz value.
// First half: B <- mu I - G and XT <- X_r Theta_r (the rank-r term is added by a GEMM).
// (low = 1, SIPX_RANK_CERT_CHECK only: mu = half the (r+1)-th Ritz value, below an eigenvalue B must then have -- never definite)
__global__ __launch_bounds__(BLOCK) void k_cert_shift(int k, int b, int r, int batch, const double* __restrict__ G, const double* __restrict__ W,
                                                      double* __restrict__ B, int low = 0) {
  const long long per = (long long)k * k, total = per * batch;
  for (long long e = (long long)blockIdx.x * BLOCK + threadIdx.x; e < total; e += (long long)gridDim.x * BLOCK) {
    const long long l = e / per, o = e - l * per;
    const int row = (int)(o % k), col = (int)(o / k);
    const double mu = low ? 0.5 * W[l * b + b - r - 1] : 0.5 * (W[l * b + b - r] + W[l * b + b - r - 1]);
    B[e] = (row == col ? mu : 0.0) - G[e];
  }
}
__global__ __launch_bounds__(BLOCK) void k_cert_scale(int k, int b, int r, int batch, const double* __restrict__ X, const double* __restrict__ W,
                                                      double* __restrict__ XT) {
  const long long per = (long long)k * r, total = per * batch;
  for (long long e = (long long)blockIdx.x * BLOCK + threadIdx.x; e < total; e += (long long)gridDim.x * BLOCK) {
    const long long l = e / per, o = e - l * per;
    const int j = b - r + (int)(o / k);
    XT[l * (long long)k * b + (long long)(b - r) * k + o] = X[l * (long long)k * b + (long long)(b - r) * k + o] * W[l * b + j];
  }
}
// Blocked Cholesky for that certificate (only its success matters): the bs x bs diagonal block at (J, J) of every matrix --
// upper triangle, column-major, leading dimension k -- is factored in LDS, D = U'U, and the inverse of U goes to Winv (64 x 64 per
// matrix, leading dimension 64), so that the block row of the factor is one GEMM, U_J,rest = Winv' B_J,rest, and the trailing
// matrix takes one more, B_rest,rest -= U_J,rest' U_J,rest (rank_cert_factor below).  A pivot that is not positive raises info[l]
// and leaves the identity in Winv: the matrix is not positive definite, whatever the later steps make of it.
// (rocSOLVER's potrf_strided_batched: 7.3 ms for 512 matrices of 512 x 512, a fifth of the call.)
__global__ __launch_bounds__(256) void k_chol_diag(int k, int J, int bs, const double* __restrict__ B, long long sB, double* __restrict__ Winv,
                                                   rocblas_int* __restrict__ info) {
  __shared__ double A[64 * 65];
  __shared__ double Bv[64 * 65];
  const int l = blockIdx.x, t = threadIdx.x;
  const double* Bl = B + (long long)l * sB + (long long)J * k + J;
  double* Wl = Winv + (long long)l * 4096;
  for (int e = t; e < bs * bs; e += 256) {
    const int i = e % bs, c = e / bs;
    if (i <= c) A[i * 65 + c] = Bl[(long long)c * k + i];
    Bv[i * 65 + c] = 0.0;
  }
  bool bad = false;
  for (int j = 0; j < bs; ++j) {
    __syncthreads();
    const double piv = A[j * 65 + j];
    if (!(piv > 0.0)) { bad = true; break; }               // the same value in every thread: a uniform exit (NaN lands here too)
    const double inv = 1.0 / sqrt(piv);
    __syncthreads();
    if (t == 0) A[j * 65 + j] = sqrt(piv);
    for (int c = j + 1 + t; c < bs; c += 256) A[j * 65 + c] *= inv;
    __syncthreads();
    const int nrem = bs - j - 1;
    for (int e = t; e < nrem * nrem; e += 256) {
      const int ii = e / nrem, cc = e - ii * nrem;
      if (cc >= ii) A[(j + 1 + ii) * 65 + j + 1 + cc] -= A[j * 65 + j + 1 + ii] * A[j * 65 + j + 1 + cc];
    }
  }
  __syncthreads();
  if (bad) {
    if (t == 0) info[l] = 1;
    for (int e = t; e < 4096; e += 256) Wl[e] = (e % 64 == e / 64) ? 1.0 : 0.0;
    return;
  }
  if (t < bs) {                                              // column t of the inverse of U, back substitution
    const int c = t;
    Bv[c * 65 + c] = 1.0 / A[c * 65 + c];
    for (int i = c - 1; i >= 0; --i) {
      double acc = 0;
      for (int q = i + 1; q <= c; ++q) acc += A[i * 65 + q] * Bv[q * 65 + c];
      Bv[i * 65 + c] = -acc / A[i * 65 + i];
    }
  }
  __syncthreads();
  for (int e = t; e < 4096; e += 256) {
    const int i = e % 64, c = e / 64;
    Wl[e] = (i <= c && c < bs) ? Bv[i * 65 + c] : 0.0;
  }
}
__global__ void k_cert_or(int batch, const rocblas_int* __restrict__ info, unsigned long long* res) {
  const int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l < batch && info[l] != 0) atomicOr(res + 1, 32ull);
}
// After a full decomposition (eigenvalues ascending, k per matrix): the contraction factor subspace iteration on b vectors
// would see for the top-r space, theta_{b+1} / theta_r, maximum over the batch -> res[0] (bit pattern).
__global__ void k_sub_ratio(int k, int b, int r, int batch, const double* __restrict__ W, unsigned long long* res) {
  const int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= batch) return;
  const double tr = W[(long long)l * k + k - r], tb = W[(long long)l * k + k - b - 1];
  double q = (tr > 0 && tb >= 0) ? tb / tr : 1.0;
  if (!(q == q) || q > 1.0) q = 1.0;
  atomicMax(res, (unsigned long long)__double_as_longlong(q));
}
// The last b eigenvector columns of the full decomposition (k x k per matrix) become the next warm start -- unless the
// factorisation of that matrix did not converge (info != 0): its previous warm start stays.
__global__ __launch_bounds__(BLOCK) void k_sub_keep(int k, int b, int batch, const double* __restrict__ E, double* __restrict__ X,
                                                    const rocblas_int* __restrict__ info) {
  const long long per = (long long)k * b, total = per * batch;
  for (long long e = (long long)blockIdx.x * BLOCK + threadIdx.x; e < total; e += (long long)gridDim.x * BLOCK) {
    const long long l = e / per, o = e - l * per;
    if (info[l] != 0) continue;
    X[e] = E[l * (long long)k * k + (long long)(k - b) * k + o];
  }
}
// status words of a batched factorisation OR-ed into one flag (read by the host at the NEXT call of the projector: a
// projection built on a factorisation that did not converge must not go unnoticed)
// resid / smax given (one-sided Jacobi SVD): info = 1 there only says that the sweeps stopped short of the requested
// (machine-precision) tolerance; it counts as a failure when the off-diagonal mass it reports is not negligible against the
// largest singular value squared, or anything is not finite.
__global__ void k_info_or(int batch, const rocblas_int* __restrict__ info, int* __restrict__ fail, const double* __restrict__ resid,
                          const double* __restrict__ S, int k) {
  const int l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= batch || info[l] == 0) return;
  if (resid) {
    const double s0 = S[(long long)l * k], r = resid[l];
    if (r == r && s0 == s0 && r <= 1e-9 * s0 * s0) return;
  }
  atomicOr(fail, 1);
}

// switches of the rank routes, taken from env_knobs() once when the projector is built (tests and A/B runs set them before they
// build a context)
struct RankKnobs {
  int dbg = 0;                  // SIPX_EXT_DEBUG: 1 the route of every call on stderr, 2 milliseconds per phase, 3 open matrices and Jacobi sweeps per step
  bool pack = true;             // SIPX_RANK_PACK=0: every filter on the whole batch
  bool cert_check = false;      // SIPX_RANK_CERT_CHECK: both factorisations, compared matrix by matrix (tests)
  // Round 5.  eps_bw: the acceptance level of a Ritz pair as a backward error on the slice itself, ||E||_2 <= eps_bw ||X||_2
  // (k_sub_residual) -- the class of the reference's svd() in TF (project_rank!.jl:28-41).  2^-23 = eps(Float32): LAPACK's
  // sgesdd, the routine behind Julia's svd, leaves 1.4e-7 (median) to 5.9e-7 (largest) by the same measure on a 512 x 512 slice
  // of the C4 model (tests/test_svd_class.py::test_float32_svd_backward_error_class); with 2^-21 the projected slices were 2.5e-7
  // of their norm from the exact projection where sgesdd's are 2e-8 .. 1.5e-7 (tests/test_gpu_round5.py), hence the tighter level --
  // two filter degrees more per call.  0 = the strict level tol theta_max of rounds 3-4 (SIPX_RANK_STRICT=1; Float64 models never
  // come here: they keep the one-sided Jacobi SVD).
  double eps_bw = 1.1920928955078125e-07;
};

// what is kept of every slice: `inner` eigenvector columns from E (leading dimension k), `stride` doubles from one matrix to the next
struct KeptSpace {
  const double* E;
  long long stride;
};

template <typename T>
struct RankFamily;

// Is every matrix of I.Bd positive definite?  info[l] != 0 where not.  Right-looking blocked Cholesky, 64 columns a step:
// k_chol_diag, then the block row and the trailing update as two batched GEMMs (the whole trailing square: the lower half is
// wasted work the library does faster than a loop over block columns would save).
template <typename T>
static void rank_cert_factor(RankFamily<T>& I, int k) {
  hipStream_t s = I.stream;
  const double one = 1.0, zero = 0.0, mone = -1.0;
  const long long sG = (long long)k * k, sP = (long long)64 * k;
  const auto N_ = rocblas_operation_none, T_ = rocblas_operation_transpose;
  SIPX_HIP(hipMemsetAsync(I.info, 0, sizeof(rocblas_int) * I.batch, s));
  for (int J = 0; J < k; J += 64) {
    const int bs = std::min(64, k - J), rem = k - J - bs;
    hipLaunchKernelGGL(k_chol_diag, dim3(I.batch), dim3(256), 0, s, k, J, bs, I.Bd, sG, I.cert_w, I.info);
    if (rem <= 0) break;
    double* panel = I.Bd + (long long)(J + bs) * k + J;            // rows J .. J+bs, columns from J+bs on
    blas_check(rocblas_dgemm_strided_batched(I.blas, T_, N_, bs, rem, bs, &one, I.cert_w, 64, 4096, panel, k, sG, &zero, I.cert_p, 64, sP, I.batch),
               "certificate: block row");
    double* trail = I.Bd + (long long)(J + bs) * k + (J + bs);
    blas_check(rocblas_dgemm_strided_batched(I.blas, T_, N_, rem, rem, bs, &mone, I.cert_p, 64, sP, I.cert_p, 64, sP, &one, trail, k, sG, I.batch),
               "certificate: trailing update");
  }
  SIPX_HIP(hipGetLastError());
}

// ---- which rocBLAS kernel for a Float64 batched product (round 5) ----------------------------------------------------------------
// The library's own choice for the filter product G V (512 x 56 x 512 per slice) is a 64 x 32 macro tile: the 56 columns fall into
// two tiles and every Gram matrix crosses the fabric twice (profiles/r05_c4_512_pmc.json: 2.58 GB per launch against 1.3 GB);
// rocblas_gemm_strided_batched_ex lets the caller name a solution, and another one runs the same product in 0.26 instead of 0.36 ms
// (b x b x k: 0.035 instead of 0.061 ms; tools/gemm_solutions_bench.cpp).  The first call of a shape in a process therefore tries
// every solution the library lists for it, on the call's own operands (beta = 0: the output is simply written again):
//   * solutions are grouped by the BITS they produce (a hash of the output: kernels that add in the same order give the same bits --
//     all the fast ones of a shape do) -- the group is chosen by a rule that does not depend on timing noise (the library's own
//     group unless another is more than 8 % faster; among groups within 5 % of the fastest the one with the lowest solution number),
//     so that every process, every rank and every run of a library version ends with the same arithmetic;
//   * inside the group the fastest member by the clock (any member gives the same bits).
// The choice is kept per shape for the life of the process.  SIPX_GEMM_TUNE=0: the library's choice (A/B switch).
struct GemmShape {
  int ta, tb, m, n, k, lda, ldb, ldc;
  bool operator<(const GemmShape& o) const {
    return std::memcmp(this, &o, sizeof(GemmShape)) < 0;
  }
};
__global__ __launch_bounds__(256) void k_hash_bits(const unsigned long long* __restrict__ p, long long n, unsigned long long* out) {
  unsigned long long acc = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) acc += p[i] * (2ull * (unsigned long long)i + 1ull);
  atomicAdd(out, acc);       // (integer sums: the order of arrival does not matter)
}
static std::mutex& gemm_tune_mutex() { static std::mutex m; return m; }
static std::map<GemmShape, int>& gemm_tune_table() { static std::map<GemmShape, int> t; return t; }
static rocblas_status dgemm_ex(rocblas_handle h, rocblas_operation ta, rocblas_operation tb, int m, int n, int k, const double* alpha, const double* A, int lda,
                               long long sa, const double* B, int ldb, long long sb, const double* beta, double* C, int ldc, long long sc, int batch, int sol) {
  return rocblas_gemm_strided_batched_ex(h, ta, tb, m, n, k, alpha, A, rocblas_datatype_f64_r, lda, sa, B, rocblas_datatype_f64_r, ldb, sb, beta, C,
                                         rocblas_datatype_f64_r, ldc, sc, C, rocblas_datatype_f64_r, ldc, sc, batch, rocblas_datatype_f64_r,
                                         sol ? rocblas_gemm_algo_solution_index : rocblas_gemm_algo_standard, sol, 0);
}
static int gemm_tune(rocblas_handle h, const GemmShape& key, const double* A, long long sa, const double* B, long long sb, double* C, long long sc, int batch) {
  const rocblas_operation ta = (rocblas_operation)key.ta, tb = (rocblas_operation)key.tb;
  const double one = 1.0, zero = 0.0;
  hipStream_t s = nullptr;
  if (rocblas_get_stream(h, &s) != rocblas_status_success) return 0;
  rocblas_int ns = 0;
  if (rocblas_gemm_strided_batched_ex_get_solutions(h, ta, tb, key.m, key.n, key.k, &one, A, rocblas_datatype_f64_r, key.lda, sa, B, rocblas_datatype_f64_r, key.ldb,
                                                    sb, &zero, C, rocblas_datatype_f64_r, key.ldc, sc, C, rocblas_datatype_f64_r, key.ldc, sc, batch,
                                                    rocblas_datatype_f64_r, rocblas_gemm_algo_solution_index, 0, nullptr, &ns) != rocblas_status_success || ns < 1)
    return 0;
  std::vector<rocblas_int> sols(ns);
  if (rocblas_gemm_strided_batched_ex_get_solutions(h, ta, tb, key.m, key.n, key.k, &one, A, rocblas_datatype_f64_r, key.lda, sa, B, rocblas_datatype_f64_r, key.ldb,
                                                    sb, &zero, C, rocblas_datatype_f64_r, key.ldc, sc, C, rocblas_datatype_f64_r, key.ldc, sc, batch,
                                                    rocblas_datatype_f64_r, rocblas_gemm_algo_solution_index, 0, sols.data(), &ns) != rocblas_status_success)
    return 0;
  sols.resize(ns);
  unsigned long long* dh = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  DeviceMemory tmp;
  try { dh = tmp.alloc<unsigned long long>(1, Mem::NoFill); } catch (const std::exception&) { return 0; }
  (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  const long long span = sc * (long long)batch;
  struct Res { int sol; unsigned long long hash; float ms; };
  std::vector<Res> res;
  auto probe = [&](int sol, Res& r) -> bool {
    r.sol = sol;
    if (dgemm_ex(h, ta, tb, key.m, key.n, key.k, &one, A, key.lda, sa, B, key.ldb, sb, &zero, C, key.ldc, sc, batch, sol) != rocblas_status_success) return false;
    (void)hipMemsetAsync(dh, 0, sizeof(unsigned long long), s);
    hipLaunchKernelGGL(k_hash_bits, dim3(1024), dim3(256), 0, s, reinterpret_cast<const unsigned long long*>(C), span, dh);
    if (hipMemcpyAsync(&r.hash, dh, sizeof(unsigned long long), hipMemcpyDeviceToHost, s) != hipSuccess) return false;
    (void)hipEventRecord(e0, s);
    for (int rep = 0; rep < 2; ++rep)
      if (dgemm_ex(h, ta, tb, key.m, key.n, key.k, &one, A, key.lda, sa, B, key.ldb, sb, &zero, C, key.ldc, sc, batch, sol) != rocblas_status_success) return false;
    (void)hipEventRecord(e1, s);
    if (hipEventSynchronize(e1) != hipSuccess) return false;
    r.ms = 0;
    (void)hipEventElapsedTime(&r.ms, e0, e1);
    return r.ms > 0;
  };
  Res def{};
  const bool have_def = probe(0, def);
  for (int sol : sols) { Res r{}; if (probe(sol, r)) res.push_back(r); }
  int choice = 0;
  if (have_def && !res.empty()) {
    // groups by output bits: fastest member, lowest solution number
    std::map<unsigned long long, std::pair<float, int>> best;      // hash -> (fastest time, its solution)
    std::map<unsigned long long, int> lowest;
    for (const Res& r : res) {
      auto it = best.find(r.hash);
      if (it == best.end() || r.ms < it->second.first) best[r.hash] = {r.ms, r.sol};
      auto lt = lowest.find(r.hash);
      if (lt == lowest.end() || r.sol < lt->second) lowest[r.hash] = r.sol;
    }
    float t_best = 1e30f;
    for (auto& kv : best) t_best = std::min(t_best, kv.second.first);
    const float t_def_group = best.count(def.hash) ? std::min(def.ms, best[def.hash].first) : def.ms;
    if (t_def_group <= 1.08f * t_best) {
      choice = (best.count(def.hash) && best[def.hash].first < def.ms) ? best[def.hash].second : 0;      // the library's own arithmetic, its fastest kernel
    } else {
      unsigned long long pick = 0;
      int low = 0x7fffffff;
      for (auto& kv : best)
        if (kv.second.first <= 1.05f * t_best && lowest[kv.first] < low) { low = lowest[kv.first]; pick = kv.first; }
      choice = best[pick].second;
    }
    if (env_knobs().gemm_tune_debug)
      fprintf(stderr, "[sipx gemm] %c%c %d x %d x %d, batch %d: %d solutions in %zu groups by bits; library %.3f ms, fastest %.3f ms; solution %d\n",
              key.ta == rocblas_operation_none ? 'N' : 'T', key.tb == rocblas_operation_none ? 'N' : 'T', key.m, key.n, key.k, batch, ns, best.size(),
              def.ms / 2, t_best / 2, choice);
  }
  // the call's own result, by the kernel that was chosen (the probes left another candidate's output in C)
  (void)dgemm_ex(h, ta, tb, key.m, key.n, key.k, &one, A, key.lda, sa, B, key.ldb, sb, &zero, C, key.ldc, sc, batch, choice);
  (void)hipStreamSynchronize(s);
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  return choice;
}
static rocblas_status gemm_sbx(rocblas_handle h, rocblas_operation ta, rocblas_operation tb, int m, int n, int k, double alpha, const double* A,
                               int lda, long long sa, const double* B, int ldb, long long sb, double beta, double* C, int ldc, long long sc, int batch,
                               int tune = 0) {
  // (the tuned path: plain products C = A B with whole outputs.  tune 1: a FIXED shape -- what the filter loop is made of; tune 2: a
  //  shape whose first dimension follows the data -- the projection on the vectors far above the rest, X_L' Z with 6 ... 31 rows,
  //  for which the library's choice takes 0.2-0.56 ms where another kernel takes 0.03: tried once, at the first such call, and the
  //  solution kept for every row count (a call it does not take falls back to the library's); 0: the library's choice)
  //  3: no trial, but the kernel a trial of the same shape has chosen, if there was one -- products that accumulate, beta = 1)
  const bool may_try = (tune == 1 || tune == 2) && alpha == 1.0 && beta == 0.0 && (const double*)C != A && (const double*)C != B;
  if (tune && env_knobs().gemm_tune && batch > 0 && (long long)m * n * k >= (1ll << 16)) {
    const GemmShape key{(int)ta, (int)tb, tune == 2 ? -1 : m, n, k, lda, ldb, ldc};
    int sol = 0;
    bool known = false;
    {
      std::lock_guard<std::mutex> lk(gemm_tune_mutex());
      auto it = gemm_tune_table().find(key);
      if (it != gemm_tune_table().end()) { sol = it->second; known = true; }
    }
    if (!known && may_try) {
      GemmShape probe = key;
      probe.m = m;
      sol = gemm_tune(h, probe, A, sa, B, sb, C, sc, batch);      // (leaves the product in C)
      std::lock_guard<std::mutex> lk(gemm_tune_mutex());
      gemm_tune_table()[key] = sol;
      return rocblas_status_success;
    }
    if (sol != 0) {
      const rocblas_status st = dgemm_ex(h, ta, tb, m, n, k, &alpha, A, lda, sa, B, ldb, sb, &beta, C, ldc, sc, batch, sol);
      if (st == rocblas_status_success) return st;
      if (tune != 2) {
        std::lock_guard<std::mutex> lk(gemm_tune_mutex());      // (a solution that does not take this batch count: the library's choice from here on)
        gemm_tune_table()[key] = 0;
      }
    }
  }
  return rocblas_dgemm_strided_batched(h, ta, tb, m, n, k, &alpha, A, lda, sa, B, ldb, sb, &beta, C, ldc, sc, batch);
}

// the buffers of the filtered iteration
struct RouteBufs {
  double *G, *Gp;          // the matrices; room for the packed ones
  double* X;               // Ritz vectors: the start, then every Rayleigh-Ritz step's result
  double *A, *F1, *F2;     // three blocks in rotation
  double* Xc;              // Ritz vectors of the packed matrices
  double* Cs;              // b x b per matrix: inverse Cholesky factor / masked projection coefficients
  double* Zs;              // b x b per matrix: eigenvectors of the Ritz problem
};
// the state of one call of the filtered route
struct ChebCtl {
  int w = 0, k = 0;
  bool cold = false;
  int mults = 0;
  bool fresh_start = true, tried_other = false;
  int ramp = -1, max_outer = 9;
  double ph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  std::chrono::steady_clock::time_point t_start, t_mark;
  bool hidden = true;           // at convergence: the energy bound of k_sub_residual does NOT rule out a larger eigenvalue outside the block
};
enum { CHEB_GIVE_UP = 0, CHEB_CONVERGED = 1 };

// The loop of the filtered route: Rayleigh-Ritz step, residual, decisions, filter.
// CHEB_CONVERGED: every wanted pair is below its level (B.X and I.Ws hold the pairs of the whole batch, unpacked);
// CHEB_GIVE_UP: the caller decomposes fully.
template <typename T>
static int cheb_loop(RankFamily<T>& I, RouteBufs B, ChebCtl& C) {
  hipStream_t s = I.stream;
  const int k = C.k, w = C.w;
  const int b = I.sub_b, r = I.r, batch = I.batch;
  const long long sG = (long long)k * k, sX = (long long)k * b, sH = (long long)b * b;
  const auto N_ = rocblas_operation_none, T_ = rocblas_operation_transpose;
  const auto& KN = I.knobs;
  constexpr int budget = 160;      // multiplications with G a call may spend
  constexpr int m_cap = 16;        // degree of one filter at most
  constexpr double tol = 1e-12;    // convergence level of a Ritz pair relative to theta_max
  const int dbg = KN.dbg;
  // index of the Ritz value that ends the damped interval (C4 with 24 guards: 2 / 3 / 4 / 6 -> 16.8 / 16.5 / 16.6 / 16.0 it/s)
  const int g = std::max(2, (b - r) / 12);
  auto mark = [&](int which) {
    if (dbg < 2) return;
    SIPX_HIP(hipStreamSynchronize(s));
    const auto now = std::chrono::steady_clock::now();
    C.ph[which] += std::chrono::duration<double, std::milli>(now - C.t_mark).count();
    C.t_mark = now;
  };
  double* X = B.X;
  // three blocks in rotation: A the block to orthonormalise (then the orthonormal basis), F1 and F2 free
  double *A = B.A, *F1 = B.F1, *F2 = B.F2;
  // what the loop works on: the whole batch -- or, once three quarters of it have converged, the matrices that have not, packed
  // (G into the certificate's matrix, which is free until the end; X into a block of its own: the converged matrices' vectors
  // stay where they are; the scratch blocks are used from their front).  The second and later filters of a call were observed
  // to run for 1 to 27 of 512 slices.
  int nb = batch;
  double* Gd = B.G;
  double *Ws = I.Ws, *Fro = I.Fro;
  bool packed = false;
  const bool may_pack = I.sub_cap > 0 && KN.pack;
  int m_prev = 0;
  double prev = -1;
  bool retried = false;
  int m_lim = m_cap;
  // A start that says nothing about this input -- none at all (the block is pseudo-random: `cold`), or the previous call's vectors
  // on the second iteration of a solve (first residual above 1e-3 theta_max) -- is RAMPED instead of given up (rounds 3-4 decomposed
  // fully: 105-185 ms for 512 slices of 512 x 512).  What went wrong with long filters from such a block (DESIGN_HISTORY, round 3):
  // a direction 1e5 times the rest that the block holds only roughly cannot be projected out of the products, is amplified in every
  // column and leaves a block of dependent columns; and the Ritz values of a cold block say nothing about where the unwanted part
  // of the spectrum ends.  So: three steps of degree one (a shifted power step each, no product beyond the Rayleigh-Ritz step's own:
  // whatever is far above the rest converges by its ratio per step), then degrees 2, 4, 8 -- every Rayleigh-Ritz step moves the
  // interval ends towards the spectrum's -- then the usual filters.  The stall rule waits until the ramp is over.
  static const int ramp_deg[6] = {1, 1, 1, 2, 4, 8};
  const int budget_all = budget * 2;
  for (int outer = 0; outer < C.max_outer; ++outer) {
    // Rayleigh-Ritz on span(A): Cholesky QR (twice behind a filter: its columns lean on each other), H = Q'GQ, X = Q S
    SIPX_HIP(hipMemsetAsync(I.info, 0, sizeof(rocblas_int) * 2 * batch, s));
    for (int pass = 0; pass < (m_prev > 0 ? 2 : 1); ++pass) {
      blas_check(gemm_sbx(I.blas, T_, N_, b, b, k, 1.0, A, k, sX, A, k, sX, 0.0, I.Hs, b, sH, nb, 1), "Y'Y");
      hipLaunchKernelGGL(k_chol_inv, dim3(nb), dim3(256), 0, s, b, nb, I.Hs, B.Cs, I.info);
      blas_check(gemm_sbx(I.blas, N_, N_, k, b, b, 1.0, A, k, sX, B.Cs, b, sH, 0.0, F1, k, sX, nb, 1), "Y Rinv");
      std::swap(A, F1);
    }
    mark(0);
    blas_check(gemm_sbx(I.blas, N_, N_, k, b, k, 1.0, Gd, k, sG, A, k, sX, 0.0, F1, k, sX, nb, 1), "G Q");
    ++C.mults;
    mark(1);
    blas_check(gemm_sbx(I.blas, T_, N_, b, b, k, 1.0, A, k, sX, F1, k, sX, 0.0, I.Hs, b, sH, nb, 1), "Q'GQ");
    mark(2);
    hipLaunchKernelGGL(k_ritz_jacobi, dim3(nb), dim3(256), 0, s, b, nb, I.Hs, B.Zs, Ws, I.info + batch, I.info + 2 * batch);
    mark(3);
    blas_check(gemm_sbx(I.blas, N_, N_, k, b, b, 1.0, A, k, sX, B.Zs, b, sH, 0.0, X, k, sX, nb, 1), "Q Z");
    blas_check(gemm_sbx(I.blas, N_, N_, k, b, b, 1.0, F1, k, sX, B.Zs, b, sH, 0.0, F2, k, sX, nb, 1), "(GQ) Z");
    mark(2);
    SIPX_HIP(hipMemsetAsync(I.sub_res, 0, 8 * sizeof(unsigned long long), s));
    SIPX_HIP(hipMemsetAsync(I.sub_res + 2, 0x7f, sizeof(unsigned long long), s));       // a large positive double: the minimum starts there
    hipLaunchKernelGGL(k_sub_residual, dim3(nb), dim3(BLOCK), 0, s, k, b, r, nb, F2, X, Ws, b, I.info, I.info + batch, Fro, I.sub_res, I.Es,
                       KN.eps_bw, tol);
    hipLaunchKernelGGL(k_cheb_plan, dim3((nb + 63) / 64), dim3(64), 0, s, b, g, r, nb, Ws, I.Es, tol, I.sub_res);
    if (may_pack && !packed) hipLaunchKernelGGL(k_sub_list, dim3(1), dim3(256), 0, s, nb, I.Es, tol, I.sub_idx, I.sub_res);
    SIPX_HIP(hipMemcpyAsync(I.sub_res_host, I.sub_res, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    SIPX_HIP(hipStreamSynchronize(s));
    mark(4);
    double res, tmin, res_raw;
    std::memcpy(&res, &I.sub_res_host[0], sizeof(double));
    std::memcpy(&tmin, &I.sub_res_host[2], sizeof(double));
    std::memcpy(&res_raw, &I.sub_res_host[6], sizeof(double));
    const bool failed = (I.sub_res_host[1] & 15ull) != 0;
    const int n_open = (int)I.sub_res_host[4];
    const bool pack_now = may_pack && !packed && res > tol && n_open >= 1 && n_open <= I.sub_cap;
    const int nl = (int)I.sub_res_host[(packed || pack_now) ? 3 : 5];
    if (dbg) fprintf(stderr, "[sipx rank] filtered subspace step %d: %d products, residual %.3e (%.3e of theta_max), fail-bits %llu, t_r %.4g, "
                             "%d vectors far above, %d of %d matrices%s%s, %.2f ms\n",
                     outer, C.mults, res, res_raw, I.sub_res_host[1], tmin, nl, nb, batch, packed ? " (packed)" : "", C.ramp >= 0 ? " (ramp)" : "",
                     std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - C.t_start).count());
    if (dbg >= 3) {
      std::vector<rocblas_int> sw(nb);
      SIPX_HIP(hipMemcpy(sw.data(), I.info + 2 * batch, sizeof(rocblas_int) * nb, hipMemcpyDeviceToHost));
      long long tot = 0; int mx = 0;
      for (int l = 0; l < nb; ++l) { tot += sw[l]; mx = std::max(mx, (int)sw[l]); }
      fprintf(stderr, "[sipx rank]   Jacobi sweeps: mean %.1f, max %d\n", (double)tot / nb, mx);
    }
    if (dbg >= 3) {                                        // how many matrices of the batch still need a filter
      std::vector<double> pm(nb);
      SIPX_HIP(hipMemcpy(pm.data(), I.Es, sizeof(double) * nb, hipMemcpyDeviceToHost));
      int a12 = 0, a10 = 0, a8 = 0, worst_l = 0;
      for (int l = 0; l < nb; ++l) { a12 += pm[l] > 1e-12; a10 += pm[l] > 1e-10; a8 += pm[l] > 1e-8; if (pm[l] > pm[worst_l]) worst_l = l; }
      fprintf(stderr, "[sipx rank]   matrices above 1e-12: %d, above 1e-10: %d, above 1e-8: %d (of %d)\n", a12, a10, a8, nb);
      if (dbg >= 4) {                                      // the worst matrix: its Ritz values and the residual of every column, in units of theta_j
        std::vector<double> ww(b);
        std::vector<double> zz((size_t)k * b), xx((size_t)k * b);
        SIPX_HIP(hipMemcpy(ww.data(), Ws + (size_t)worst_l * b, sizeof(double) * b, hipMemcpyDeviceToHost));
        SIPX_HIP(hipMemcpy(zz.data(), F2 + (size_t)worst_l * sX, sizeof(double) * sX, hipMemcpyDeviceToHost));
        SIPX_HIP(hipMemcpy(xx.data(), X + (size_t)worst_l * sX, sizeof(double) * sX, hipMemcpyDeviceToHost));
        fprintf(stderr, "[sipx rank]   worst matrix %d (%.3e): column: Ritz value / theta_max, residual / theta_j\n", worst_l, pm[worst_l]);
        for (int j = b - 1; j >= 0; --j) {
          double t = 0;
          for (int i = 0; i < k; ++i) { const double d = zz[(size_t)j * k + i] - ww[j] * xx[(size_t)j * k + i]; t += d * d; }
          fprintf(stderr, " %d:%.3e/%.2e", b - j, ww[j] / ww[b - 1], std::sqrt(t) / (ww[j] > 0 ? ww[j] : 1.0));
        }
        fprintf(stderr, "\n");
      }
    }
    if (failed) break;
    // The previous call's vectors say little about this input (the first iterations of a solve): filters started from there
    // were observed to swamp the guard columns and then stall at a residual of 1e-8 theta_max.
    if (C.fresh_start && C.ramp < 0 && res_raw > 1e-3) {
      // the feasibility estimate is asked for every tenth iteration only, its own vectors are ten iterations old: those of the
      // y update of this iteration (another input, but the same x behind it) may be the better start
      if (w == 1 && I.sub_have[0] && !C.tried_other) {
        C.tried_other = true;
        SIPX_HIP(hipMemcpyAsync(A, I.Xs[0], sizeof(double) * (size_t)sX * batch, hipMemcpyDeviceToDevice, s));
        if (dbg) fprintf(stderr, "[sipx rank] poor start: once more from the vectors of the y update\n");
        continue;
      }
      C.ramp = 0;                     // go on from what the step left, by the ramp
      C.max_outer = 24;
      C.cold = true;                  // (its budget)
      if (dbg) fprintf(stderr, "[sipx rank] poor start (%.3e of theta_max): ramped filters\n", res_raw);
    }
    C.fresh_start = false;
    if (res <= tol) {
      if (packed) {                   // the vectors and Ritz values of the packed matrices go back to their places
        hipLaunchKernelGGL(k_sub_move, dim3(NB), dim3(BLOCK), 0, s, sX, nb, I.sub_idx, X, B.X, 1);
        hipLaunchKernelGGL(k_sub_move, dim3(64), dim3(BLOCK), 0, s, (long long)b, nb, I.sub_idx, Ws, I.Ws, 1);
      }
      // (packed: the bit of the converged matrices is no longer seen)
      C.hidden = packed || (I.sub_res_host[1] & 16ull) != 0;
      return CHEB_CONVERGED;
    }
    if (C.ramp >= 0) prev = -1;                           // (no verdict on a filter while the intervals are still being found)
    if (prev > 0 && !(res < 0.5 * prev) && !retried) {
      // The filter did not do what its degree promised -- in a long C4 solve (80 iterations) the residual ROSE behind a filter in
      // one call of nine (4.9e-5 -> 1.4e-4 for all 512 slices, 3.6e-8 -> 3.0e-6 for seven): the intervals of a call's first filter
      // come from Ritz values the previous call's vectors give on THIS call's matrices, and where a spectrum has moved a
      // column is amplified where it should be damped, swamps its neighbours and is re-seeded.  The Rayleigh-Ritz step behind
      // the filter has corrected the Ritz values; what it left is no worse than a usual start (1e-4 ... 1e-5), so the call goes
      // on from there with filters of half the degree -- once: 16-45 products against a full decomposition and the calls that
      // used to sit out behind it.
      retried = true;
      m_lim = std::max(4, m_lim / 2);
      prev = -1;
      if (dbg) fprintf(stderr, "[sipx rank] residual %.3e behind a filter (not half of the one before): once more, degree <= %d\n", res, m_lim);
    }
    if (prev > 0 && !(res < 0.5 * prev)) {               // the filter did not do what its degree promised
      if (dbg) {                                           // which matrix, and what its Ritz values look like
        std::vector<double> pm(nb), ww((size_t)b * nb);
        SIPX_HIP(hipMemcpy(pm.data(), I.Es, sizeof(double) * nb, hipMemcpyDeviceToHost));
        SIPX_HIP(hipMemcpy(ww.data(), Ws, sizeof(double) * b * nb, hipMemcpyDeviceToHost));
        int worst_l = 0, above = 0;
        for (int l = 0; l < nb; ++l) { if (pm[l] > pm[worst_l]) worst_l = l; above += pm[l] > tol ? 1 : 0; }
        fprintf(stderr, "[sipx rank] stalled: %d matrices above the tolerance, worst %d (%.3e); its Ritz values:", above, worst_l, pm[worst_l]);
        for (int j = 0; j < b; ++j) fprintf(stderr, " %.4e", ww[(size_t)worst_l * b + j]);
        fprintf(stderr, "\n");
      }
      break;
    }
    prev = res;
    if (pack_now) {
      // X, G X, the Ritz values, ||G||_F^2 and G itself of the open matrices, packed; G X lands in F1 (free: the product G Q
      // has gone into F2 = (G Q) Z), which then takes the place of F2
      hipLaunchKernelGGL(k_sub_move, dim3(NB), dim3(BLOCK), 0, s, sG, n_open, I.sub_idx, B.G, B.Gp, 0);
      hipLaunchKernelGGL(k_sub_move, dim3(NB), dim3(BLOCK), 0, s, sX, n_open, I.sub_idx, X, B.Xc, 0);
      hipLaunchKernelGGL(k_sub_move, dim3(NB), dim3(BLOCK), 0, s, sX, n_open, I.sub_idx, F2, F1, 0);
      hipLaunchKernelGGL(k_sub_move, dim3(64), dim3(BLOCK), 0, s, (long long)b, n_open, I.sub_idx, I.Ws, I.Wc, 0);
      hipLaunchKernelGGL(k_sub_move, dim3(1), dim3(BLOCK), 0, s, 1LL, n_open, I.sub_idx, I.Fro, I.Froc, 0);
      std::swap(F1, F2);
      Gd = B.Gp; X = B.Xc; Ws = I.Wc; Fro = I.Froc;
      nb = n_open;
      packed = true;
      ++I.n_packed;
      mark(7);
    }
    // the next filter: T_m(t_r) = cosh(m acosh t_r) >= 10 res / tol, within the cap and the budget
    const double need = std::acosh(std::max(10.0 * res / tol, 2.0));
    const double per = std::acosh(std::max(tmin, 1.0 + 1e-9));
    int m = (int)std::ceil(need / per);
    if (m < 2) m = 2;
    const int m_max = m_lim;
    if (C.ramp >= 0) {
      const int md = ramp_deg[C.ramp];
      m = C.ramp < 3 ? md : std::min(std::max(m, 2), md);   // (a block that is nearly there does not need the whole ramp's degrees)
      if (++C.ramp >= 6) C.ramp = -1;
      if (C.mults + m + 1 > budget_all) break;
    } else if (m > m_max) {                               // several filters: can the budget still hold them?
      const double outers = std::ceil(need / (per * m_max));
      if (C.mults + outers * (m_max + 1) > (C.cold ? budget_all : budget)) {
        if (dbg) fprintf(stderr, "[sipx rank] filtered subspace: %g more products needed, over the budget\n", outers * (m_max + 1));
        break;
      }
      m = m_max;
    } else if (C.mults + m + 1 > (C.cold ? budget_all : budget)) break;
    // Y_0 = X, Y_1 = (2/a) P G X - X with G X = F2 already there; Y_{i+1} = (4/a) P G Y_i - 2 Y_i - Y_{i-1}.  X stays (the
    // projections need it); products go to F1, the iterates alternate between F2 and A, each new one over the one two steps back
    double *Y0 = X, *Y1 = X;
    for (int i = 1; i <= m; ++i) {
      double* Z = F2;
      if (i > 1) {
        blas_check(gemm_sbx(I.blas, N_, N_, k, b, k, 1.0, Gd, k, sG, Y1, k, sX, 0.0, F1, k, sX, nb, 1), "G Y");
        ++C.mults;
        Z = F1;
        mark(1);
      }
      double* out = i == 1 ? F2 : (i == 2 ? A : Y0);
      if (nl <= 2) {
        mark(5);
        hipLaunchKernelGGL(k_cheb_step_proj, dim3((unsigned)(((long long)b * nb + 3) / 4)), dim3(256), 0, s, k, b, g, r, nl, nb, Ws, X, Z, Y1, Y0,
                           out, i == 1 ? 1 : 0);
        mark(6);
        Y0 = Y1;
        Y1 = out;
        continue;
      }
      if (nl > 0) {
        const double* XL = X + (long long)(b - nl) * k;
        blas_check(gemm_sbx(I.blas, T_, N_, nl, b, k, 1.0, XL, k, sX, Z, k, sX, 0.0, B.Cs, b, sH, nb, 2), "X_L' Z");
        hipLaunchKernelGGL(k_cheb_mask, dim3((unsigned)std::min<long long>(NB, ((long long)nl * b * nb + 255) / 256)), dim3(256), 0, s, b, g, r, nl, nb,
                           Ws, B.Cs);
        blas_check(gemm_sbx(I.blas, N_, N_, k, b, nl, -1.0, XL, k, sX, B.Cs, b, sH, 1.0, Z, k, sX, nb), "Z - X_L C");
      }
      mark(5);
      hipLaunchKernelGGL(k_cheb_step, dim3(NB), dim3(BLOCK), 0, s, k, b, g, r, nb, Ws, Z, Y1, Y0, out, i == 1 ? 1 : 0);
      mark(6);
      Y0 = Y1;
      Y1 = out;
    }
    m_prev = m;
    if (Y1 != A) std::swap(A, F2);                       // the filtered block is the one to orthonormalise next
    // the g lowest columns sit inside the damped interval: T_m there is anything in [-1, 1], also (nearly) zero, and such a
    // column would be nothing but what leaked in from above -- dependent on the other columns.  They stay what they were.
    if (g > 0)
      SIPX_HIP(hipMemcpy2DAsync(A, sizeof(double) * (size_t)sX, X, sizeof(double) * (size_t)sX, sizeof(double) * (size_t)k * g, nb,
                                hipMemcpyDeviceToDevice, s));
  }
  return CHEB_GIVE_UP;
}

// Rank projection, Gram route: the top-r invariant subspace of every G_l from the Ritz vectors of the previous call (I.Xs[w]),
// by Rayleigh-Ritz steps with a Chebyshev filter between them (kernels above).  One multiplication with G per filter degree
// and one per Rayleigh-Ritz step; the degree of every filter is chosen from the residual still to be removed and the
// flattest spectrum of the batch, T_m(t_r) >= 10 residual / tolerance.  Accepted when every top-r pair has a residual below
// its level (k_sub_residual) AND nothing above theta_r can hide outside the block: the energy bound of k_sub_residual where the
// spectrum decays, the inertia of G with the found pairs removed (one batched Cholesky factorisation) where it is flat.
// Returns false -- the caller then decomposes fully -- when the budget of multiplications cannot suffice, a factorisation
// fails or the certificate does not hold.
template <typename T>
static bool rank_cheb_route(RankFamily<T>& I, int w, int k, bool cold = false) {
  hipStream_t s = I.stream;
  const int b = I.sub_b, r = I.r, batch = I.batch;
  const double one = 1.0;
  const long long sG = (long long)k * k, sX = (long long)k * b;
  const auto N_ = rocblas_operation_none, T_ = rocblas_operation_transpose;
  const auto& KN = I.knobs;
  const int dbg = KN.dbg;
  ChebCtl C;
  C.w = w; C.k = k; C.cold = cold;
  C.ramp = cold ? 0 : -1;
  C.max_outer = cold ? 24 : 9;
  C.t_start = C.t_mark = std::chrono::steady_clock::now();
  auto mark = [&](int which) {
    if (dbg < 2) return;
    SIPX_HIP(hipStreamSynchronize(s));
    const auto now = std::chrono::steady_clock::now();
    C.ph[which] += std::chrono::duration<double, std::milli>(now - C.t_mark).count();
    C.t_mark = now;
  };
  RouteBufs B{I.Gd, I.Bd, I.Xs[w], I.Qs, I.Ys, I.Zs, I.Xc, I.Cs, I.Hs};
  double* X = I.Xs[w];
  sub_fro(s, k, batch, I.Gd, I.FroPart, I.Fro);
  SIPX_HIP(hipMemcpyAsync(B.A, X, sizeof(double) * (size_t)sX * batch, hipMemcpyDeviceToDevice, s));
  mark(7);
  const int rc = cheb_loop<T>(I, B, C);
  bool ok = false;
  if (rc == CHEB_CONVERGED && !C.hidden) {
    ok = true;                        // a spectrum that decays behind the block: the energy bound has certified the pairs
  } else if (rc == CHEB_CONVERGED) {
    double* F1 = I.Ys;
    // flat spectrum: the inertia certificate (X_r Theta_r goes through F1)
    hipLaunchKernelGGL(k_cert_shift, dim3(NB), dim3(BLOCK), 0, s, k, b, r, batch, I.Gd, I.Ws, I.Bd);
    hipLaunchKernelGGL(k_cert_scale, dim3(NB), dim3(BLOCK), 0, s, k, b, r, batch, X, I.Ws, F1);
    blas_check(gemm_sbx(I.blas, N_, T_, k, k, r, 1.0, F1 + (long long)(b - r) * k, k, sX, X + (long long)(b - r) * k, k, sX, 1.0, I.Bd, k, sG, batch, 3),
               "certificate: rank-r term");
    rank_cert_factor<T>(I, k);
    SIPX_HIP(hipMemsetAsync(I.sub_res, 0, 2 * sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_cert_or, dim3((batch + 63) / 64), dim3(64), 0, s, batch, I.info, I.sub_res);
    SIPX_HIP(hipMemcpyAsync(I.sub_res_host, I.sub_res, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    SIPX_HIP(hipStreamSynchronize(s));
    ok = (I.sub_res_host[1] & 32ull) == 0;
    mark(7);
    if (KN.cert_check) {
      // the blocked factorisation against the library's, matrix by matrix, on the certificate's own matrices and on matrices
      // that cannot be definite (tests)
      for (int low = 0; low < 2; ++low) {
        std::vector<rocblas_int> v[2];
        for (int lib = 0; lib < 2; ++lib) {
          hipLaunchKernelGGL(k_cert_shift, dim3(NB), dim3(BLOCK), 0, s, k, b, r, batch, I.Gd, I.Ws, I.Bd, low);
          blas_check(rocblas_dgemm_strided_batched(I.blas, N_, T_, k, k, r, &one, F1 + (long long)(b - r) * k, k, sX, X + (long long)(b - r) * k, k, sX,
                                                   &one, I.Bd, k, sG, batch), "certificate: rank-r term");
          if (lib) blas_check(rocsolver_dpotrf_strided_batched(I.blas, rocblas_fill_upper, k, I.Bd, k, sG, I.info, batch), "certificate: potrf");
          else rank_cert_factor<T>(I, k);
          v[lib].resize(batch);
          SIPX_HIP(hipStreamSynchronize(s));
          SIPX_HIP(hipMemcpy(v[lib].data(), I.info, sizeof(rocblas_int) * batch, hipMemcpyDeviceToHost));
        }
        int differ = 0, indef = 0;
        for (int l = 0; l < batch; ++l) { differ += (v[0][l] != 0) != (v[1][l] != 0); indef += v[1][l] != 0; }
        fprintf(stderr, "[sipx rank] certificate check (%s shift): %d of %d matrices not positive definite, the two factorisations differ on %d\n",
                low ? "low" : "the certificate's", indef, batch, differ);
        if (differ) throw std::runtime_error("internal: the blocked Cholesky of the inertia certificate and the library's disagree");
      }
    }
    if (dbg) fprintf(stderr, "[sipx rank] inertia certificate %s, %.2f ms\n", ok ? "holds" : "fails",
                     std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - C.t_start).count());
  }
  if (dbg >= 2)
    fprintf(stderr, "[sipx rank] phases (ms): orthonormalise %.2f, products with G %.2f (%d), small products %.2f, Ritz solver %.2f, residual %.2f, "
                    "projections %.2f, recurrence %.2f, copy + certificate %.2f\n", C.ph[0], C.ph[1], C.mults, C.ph[2], C.ph[3], C.ph[4], C.ph[5], C.ph[6], C.ph[7]);
  I.n_products += C.mults;
  SIPX_HIP(hipGetLastError());
  return ok;
}

template <typename T>
struct RankFamily : ExtImpl<T> {
  using ExtImpl<T>::sp;
  using ExtImpl<T>::stream;
  SegMap map{};
  BlasHandle blas;
  int r = 0, m = 0, n = 0, k = 0, batch = 1;       // slices of m x n, k = min(m, n)
  double *Ad = nullptr, *Ud = nullptr, *Sd = nullptr, *Vd = nullptr, *Ed = nullptr;
  double *Gd = nullptr, *Gs = nullptr, *Wd = nullptr;     // Gram route: eigenvectors, scaled copy, eigenvalues
  bool gram = false;
  // rank, Gram route: warm-started block subspace iteration (top-r invariant subspace of the Gram matrices)
  int sub_b = 0;                                   // block size r + 16 or r + 24 (0 = route not used)
  double *Xs[2] = {nullptr, nullptr};              // Ritz vectors of the previous call (y update / feasibility estimate)
  bool sub_have[2] = {false, false}, sub_try[2] = {false, false};
  double *Qs = nullptr, *Zs = nullptr, *Hs = nullptr, *Ws = nullptr, *Es = nullptr, *Fro = nullptr, *FroPart = nullptr;
  // Chebyshev-filtered variant of the same route (spectra without a gap behind the block): one more block, the matrix of the
  // inertia certificate, calls to sit out after a failed attempt
  bool cheb = false;
  double *Ys = nullptr, *Bd = nullptr, *Cs = nullptr;
  RankKnobs knobs;
  // the matrices that still need a filter when most of the batch has converged, packed (rank_cheb_route)
  double *Xc = nullptr, *Wc = nullptr, *Froc = nullptr;
  double *cert_w = nullptr, *cert_p = nullptr;     // the certificate's blocked Cholesky: inverse diagonal factors, one block row
  int* sub_idx = nullptr;
  int sub_cap = 0;
  long long n_packed = 0;
  int cheb_skip[2] = {0, 0}, cheb_fails[2] = {0, 0};
  long long n_calls = 0, n_subspace = 0, n_full = 0, n_products = 0;       // route_counts()
  unsigned long long* sub_res = nullptr;           // device: bit pattern of the largest relative residual, failure flag
  unsigned long long* sub_res_host = nullptr;      // pinned
  rocblas_int* info = nullptr;
  int* flag = nullptr;
  // status of the batched factorisations: OR of info != 0, copied to pinned memory behind the call, looked at by the next one
  int* fail = nullptr;
  int* fail_host = nullptr;
  hipEvent_t fail_ev = nullptr;
  bool fail_pending = false;

  RankFamily(const ExtSpec& spec, hipStream_t s) : ExtImpl<T>(spec, s) {
    try { build(); } catch (...) { release(); throw; }       // (the pinned buffer: everything else releases itself)
  }
  ~RankFamily() override { release(); }
  void release() {
    if (sub_res_host) (void)hipHostFree(sub_res_host);
    if (fail_host) (void)hipHostFree(fail_host);
    if (fail_ev) (void)hipEventDestroy(fail_ev);
  }
  void note_status(hipStream_t s, const double* resid = nullptr, const double* S = nullptr, int k = 0) {
    if (!fail) {
      fail = this->template alloc<int>(1);
      SIPX_HIP(hipHostMalloc((void**)&fail_host, sizeof(int), hipHostMallocDefault));
      SIPX_HIP(hipEventCreateWithFlags(&fail_ev, hipEventDisableTiming));
    }
    SIPX_HIP(hipMemsetAsync(fail, 0, sizeof(int), s));
    hipLaunchKernelGGL(k_info_or, dim3((batch + 63) / 64), dim3(64), 0, s, batch, info, fail, resid, S, k);
    SIPX_HIP(hipMemcpyAsync(fail_host, fail, sizeof(int), hipMemcpyDeviceToHost, s));
    SIPX_HIP(hipEventRecord(fail_ev, s));
    fail_pending = true;
  }
  void check_status() {
    if (!fail_pending) return;
    fail_pending = false;
    SIPX_HIP(hipEventSynchronize(fail_ev));
    if (*fail_host != 0)
      throw std::runtime_error("rank / nuclear projector: the batched eigen / singular value decomposition did not converge on some slice "
                               "(rocSOLVER info != 0) in the previous call");
  }
  bool right() const { return n <= m; }            // eigenvectors of X'X (right singular vectors) or of XX' (left ones)
  void set_stream(hipStream_t s) override {
    if (stream == s) return;
    stream = s;
    blas.set_stream(s);
  }
  // Back to the state of a freshly built projector (sipx_reset): no warm start of any kind, no pending status, counters at zero.
  void reset() override {
    if (fail_pending) { fail_pending = false; (void)hipEventSynchronize(fail_ev); }
    for (int w = 0; w < 2; ++w) { sub_have[w] = sub_try[w] = false; cheb_skip[w] = cheb_fails[w] = 0; }
    n_calls = n_subspace = n_full = n_products = 0;
    n_packed = 0;
  }
  void route_counts(long long out[4]) const override { out[0] = n_calls; out[1] = n_subspace; out[2] = n_full; out[3] = n_products; }

  void build() {
    const int kind = sp.kind;
    ExtSpec seg = sp;
    if (seg.mode == SIPX_MODE_WHOLE) {                     // a matrix: one "slice" orthogonal to the unit third dimension
      if (seg.dims[2] != 1)
        throw std::runtime_error("requested rank or nuclear norm constraints on a tensor, use mode=(slice,x) e.t.c. to "
                                 "define constraints per slice");                       // setup_constraints.jl:60-62
      seg.mode = SIPX_MODE_SLICE;
      seg.dir = 2;
    } else if (seg.mode != SIPX_MODE_SLICE) {
      throw std::runtime_error("mode[1] for rank / nuclear norm projections can only be: slice");
    }
    map = make_segmap(seg);
    m = (int)map.LA; n = (int)map.LB; batch = (int)map.nseg;
    k = m < n ? m : n;
    if (kind == EXT_RANK) {
      r = (int)sp.pmax;
      if (r < 1) throw std::runtime_error("rank constraint needs r >= 1");
      if (r > k) r = k;                                    // U[:,1:r] with r = min(n1,n2): the projection is the identity
    } else if (!(sp.pmax > 0)) {
      throw std::runtime_error("Radius of L1 ball is negative");                        // project_l1_Duchi!.jl:22 on F.S
    }
    blas.create(stream);
    // Float32 models take the Gram route (eigenvectors of the smaller of X'X and XX', 12-24x faster than the Jacobi SVD
    // on 256..512-sized slices); its error eps64 * cond^2 stays far below Float32 resolution.  Float64 models keep the
    // one-sided Jacobi SVD, which works on the columns of X itself.
    gram = sizeof(T) == 4;
    Ad = this->template alloc<double>((size_t)m * n * batch);
    Ud = this->template alloc<double>((size_t)m * k * batch);
    Vd = this->template alloc<double>((size_t)k * n * batch);
    Sd = this->template alloc<double>((size_t)k * batch);
    Ed = this->template alloc<double>((size_t)(gram ? k : 1) * batch);
    if (gram) {
      Gd = this->template alloc<double>((size_t)k * k * batch);
      Wd = this->template alloc<double>((size_t)k * batch);
      if (kind == EXT_NUCLEAR) Gs = this->template alloc<double>((size_t)k * k * batch);
      const EnvKnobs& E = env_knobs();
      knobs.dbg = E.ext_debug;
      knobs.pack = E.rank_pack;
      knobs.cert_check = E.rank_cert_check;
      if (E.rank_strict) knobs.eps_bw = 0.0;
      // columns the block holds beyond the r wanted ones: 24 where the matrices are large enough for the route with them, else 16.
      // (C4, 512 slices of 512 x 512, r = 32, round 4: 12 / 16 / 20 / 24 / 28 / 32 guards -> 15.7 / 15.4 / 16.3 / 16.5 / 16.4 / 16.1 it/s:
      //  more guards move the end of the damped interval away from theta_r, and the library's GEMM tiles are 32 columns wide --
      //  48 columns cost what 64 do.)
      const int extra = (r + 24) * 4 <= k && r + 24 <= 64 ? 24 : 16;
      // SIPX_RANK_SUBSPACE=0 keeps the full decomposition every call; the route is worth it only for r << k
      if (kind == EXT_RANK && E.rank_subspace && (r + extra) * 4 <= k && r + extra <= 64) {
        sub_b = r + extra;
        build_subspace_route();
      }
    }
    info = this->template alloc<rocblas_int>((size_t)3 * batch);   // info, n_sweeps / second info, sweeps of the Ritz solver
    flag = this->template alloc<int>((size_t)batch);
  }
  void build_subspace_route() {
    const size_t nb = (size_t)k * sub_b * batch;
    for (int w = 0; w < 2; ++w) Xs[w] = this->template alloc<double>(nb);
    Qs = this->template alloc<double>(nb);
    Zs = this->template alloc<double>(nb);
    Hs = this->template alloc<double>((size_t)sub_b * sub_b * batch);
    Ws = this->template alloc<double>((size_t)sub_b * batch);
    Es = this->template alloc<double>((size_t)sub_b * batch);
    Fro = this->template alloc<double>((size_t)batch);
    FroPart = this->template alloc<double>((size_t)batch * FRO_PARTS);
    sub_res = this->template alloc<unsigned long long>(8);
    SIPX_HIP(hipHostMalloc((void**)&sub_res_host, 8 * sizeof(unsigned long long), hipHostMallocDefault));
    cheb = env_knobs().rank_cheb;           // SIPX_RANK_CHEB=0: plain subspace iteration only (spectra with a gap)
    if (!cheb) return;
    Ys = this->template alloc<double>(nb);
    Cs = this->template alloc<double>((size_t)sub_b * sub_b * batch);
    Bd = this->template alloc<double>((size_t)k * k * batch);       // the matrix of the inertia certificate
    cert_w = this->template alloc<double>((size_t)4096 * batch);
    cert_p = this->template alloc<double>((size_t)64 * k * batch);
    sub_cap = batch / 4;
    if (sub_cap > 0) {
      Xc = this->template alloc<double>((size_t)k * sub_b * sub_cap);
      Wc = this->template alloc<double>((size_t)sub_b * sub_cap);
      Froc = this->template alloc<double>((size_t)sub_cap);
      sub_idx = this->template alloc<int>((size_t)batch);
    }
  }
  void form_gram() {
    const long long sA = (long long)m * n, sG = (long long)k * k;
    const auto N_ = rocblas_operation_none, T_ = rocblas_operation_transpose;
    if (right())
      blas_check(gemm_sbx(blas, T_, N_, k, k, m, 1.0, Ad, m, sA, Ad, m, sA, 0.0, Gd, k, sG, batch, 1), "gram");
    else
      blas_check(gemm_sbx(blas, N_, T_, k, k, n, 1.0, Ad, m, sA, Ad, m, sA, 0.0, Gd, k, sG, batch, 1), "gram");
  }
  // No start (round 5): is there anything to project?  The first iteration of a solve from zero hands over v = 0
  // (rhs = 0, x = 0: PARSDMM.jl:101-107 with y = l = 0) -- rounds 3-4 decomposed 512 zero matrices for 119 ms and kept
  // their arbitrary eigenvectors as the next start.  P(0) = 0: v stays as it is, the state stays cold.
  bool nothing_to_project() {
    hipStream_t s = stream;
    SIPX_HIP(hipMemsetAsync(sub_res, 0, 8 * sizeof(unsigned long long), s));
    sub_fro(s, k, batch, Gd, FroPart, Fro, sub_res);
    SIPX_HIP(hipMemcpyAsync(sub_res_host, sub_res, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    SIPX_HIP(hipStreamSynchronize(s));
    return sub_res_host[7] == 0ull;
  }
  // The filtered iteration (rank_cheb_route) from the previous call's vectors, or from pseudo-random ones where there are none
  // (cold).  It does not need a gap behind the block; an attempt that failed costs its products on top of the full decomposition,
  // so the next attempts wait (1, 2, 4, ... calls).
  bool try_filtered_route(int w, bool cold) {
    if (cold) hipLaunchKernelGGL(k_sub_seed, dim3(NB), dim3(BLOCK), 0, stream, k, sub_b, batch, Xs[w]);
    if (cheb_skip[w] > 0 && !cold) {
      --cheb_skip[w];
      return false;
    }
    const bool ok = rank_cheb_route<T>(*this, w, k, cold);
    if (ok) sub_have[w] = true;
    if (ok) cheb_fails[w] = 0;
    // (the decomposition that follows a failure leaves exact vectors behind, the best start there is: the next call tries
    //  again; only a second failure in a row makes calls sit out -- 1, 2, 4 ...)
    else { cheb_skip[w] = cheb_fails[w] >= 1 ? 1 << std::min(cheb_fails[w] - 1, 5) : 0; ++cheb_fails[w]; }
    if (knobs.dbg) fprintf(stderr, "[sipx rank] %s\n", ok ? "subspace accepted" : "full decomposition");
    return ok;
  }
  // SIPX_RANK_CHEB=0: block subspace iteration without a filter, Rayleigh-Ritz on the same block (r + 16 or r + 24 vectors) from the
  // previous call's Ritz vectors, eight steps at most.  It contracts by theta_{b+1} / theta_r per step, so it is tried only where
  // the last full decomposition measured that ratio below 1/4 (sub_try), and given up when the contraction seen so far cannot
  // reach the level within the steps left.  Accepted when every top-r pair has a residual below the strict level 1e-12 theta_max
  // and the energy bound of k_sub_residual rules out a larger eigenvalue outside the block.
  bool try_plain_subspace(int w) {
    hipStream_t s = stream;
    const int b = sub_b, dbg = knobs.dbg, max_it = 8;
    const long long sG = (long long)k * k, sX = (long long)k * b, sH = (long long)b * b;
    const auto N_ = rocblas_operation_none, T_ = rocblas_operation_transpose;
    const double one = 1.0, tol = 1e-12;
    bool sub_ok = false;
    double prev = -1;
    double* X = Xs[w];
    sub_fro(s, k, batch, Gd, FroPart, Fro);
    for (int it = 0; it < max_it; ++it) {
      blas_check(gemm_sbx(blas, N_, N_, k, b, k, 1.0, Gd, k, sG, X, k, sX, 0.0, Qs, k, sX, batch, 1), "G X");
      hipLaunchKernelGGL(k_sub_normalize, dim3(batch), dim3(BLOCK), 0, s, k, b, batch, Qs);
      blas_check(gemm_sbx(blas, T_, N_, b, b, k, 1.0, Qs, k, sX, Qs, k, sX, 0.0, Hs, b, sH, batch, 1), "Y'Y");
      blas_check(rocsolver_dpotrf_strided_batched(blas, rocblas_fill_upper, b, Hs, b, sH, info, batch), "potrf");
      blas_check(rocblas_dtrsm_strided_batched(blas, rocblas_side_right, rocblas_fill_upper, N_, rocblas_diagonal_non_unit, k, b, &one,
                                               Hs, b, sH, Qs, k, sX, batch), "trsm");          // Qs: orthonormal basis
      blas_check(gemm_sbx(blas, N_, N_, k, b, k, 1.0, Gd, k, sG, Qs, k, sX, 0.0, Zs, k, sX, batch, 1), "G Q");
      blas_check(gemm_sbx(blas, T_, N_, b, b, k, 1.0, Qs, k, sX, Zs, k, sX, 0.0, Hs, b, sH, batch, 1), "Q'GQ");
      // b x b Ritz problem: one-kernel Jacobi (the divide-and-conquer driver applies its b-1 reflectors one launch at a
      // time, 50 ms for 256 matrices of 48 x 48)
      blas_check(rocsolver_dsyevj_strided_batched(blas, rocblas_esort_ascending, rocblas_evect_original, rocblas_fill_upper, b, Hs,
                                                  b, sH, 0.0, Es, 100, info + 2 * batch, Ws, b, info + batch, batch),
                 "syevj (Ritz)");
      blas_check(gemm_sbx(blas, N_, N_, k, b, b, 1.0, Qs, k, sX, Hs, b, sH, 0.0, X, k, sX, batch, 1), "Q Z");
      blas_check(gemm_sbx(blas, N_, N_, k, b, b, 1.0, Zs, k, sX, Hs, b, sH, 0.0, Qs, k, sX, batch, 1), "(GQ) Z");
      SIPX_HIP(hipMemsetAsync(sub_res, 0, 2 * sizeof(unsigned long long), s));
      hipLaunchKernelGGL(k_sub_residual, dim3(batch), dim3(BLOCK), 0, s, k, b, r, batch, Qs, X, Ws, b, info,
                         info + batch, Fro, sub_res);
      SIPX_HIP(hipMemcpyAsync(sub_res_host, sub_res, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
      SIPX_HIP(hipStreamSynchronize(s));
      double res;
      std::memcpy(&res, &sub_res_host[0], sizeof(double));
      const bool failed = (sub_res_host[1] & 15ull) != 0;
      const bool certified = (sub_res_host[1] & 16ull) == 0;
      if (dbg) fprintf(stderr, "[sipx rank] subspace it %d: residual %.3e fail-bits %llu\n", it + 1, res, sub_res_host[1]);
      if (failed) break;
      if (res <= tol) { sub_ok = certified; break; }     // converged pairs that might not be the largest: decompose fully
      if (prev > 0) {                       // contraction observed so far: give up when the budget cannot suffice
        const double c = res / prev;
        if (!(c < 1.0)) break;
        const double need = std::log(tol / res) / std::log(c);
        if (need > (double)(max_it - 1 - it)) break;
      }
      prev = res;
    }
    if (dbg) fprintf(stderr, "[sipx rank] %s\n", sub_ok ? "subspace accepted" : "full decomposition");
    return sub_ok;
  }
  // All eigenpairs of every Gram matrix (syevd); the last r eigenvector columns span the top-r space (eigenvalues ascend).
  KeptSpace full_decomposition(int w) {
    hipStream_t s = stream;
    const int b = sub_b;
    const long long sG = (long long)k * k;
    blas_check(rocsolver_dsyevd_strided_batched(blas, rocblas_evect_original, rocblas_fill_upper, k, Gd, k, sG, Wd, k, Ed, k, info, batch),
               "syevd");
    note_status(s);
    if (b > 0) {
      // keep the top-b eigenvectors as the next warm start, and decide from the spectrum whether the plain iteration should use
      // them: it contracts by theta_{b+1} / theta_r per step, so a truncation inside a flat part of the spectrum
      // (ratio near 1) would never get there and the attempt is not made
      hipLaunchKernelGGL(k_sub_keep, dim3(NB), dim3(BLOCK), 0, s, k, b, batch, Gd, Xs[w], info);
      SIPX_HIP(hipMemsetAsync(sub_res, 0, 2 * sizeof(unsigned long long), s));
      hipLaunchKernelGGL(k_sub_ratio, dim3((batch + 63) / 64), dim3(64), 0, s, k, b, r, batch, Wd, sub_res);
      SIPX_HIP(hipMemcpyAsync(sub_res_host, sub_res, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
      SIPX_HIP(hipStreamSynchronize(s));
      double q;
      std::memcpy(&q, &sub_res_host[0], sizeof(double));
      sub_have[w] = true;
      sub_try[w] = q < 0.25;
      if (knobs.dbg) fprintf(stderr, "[sipx rank] theta_{b+1}/theta_r = %.3e -> %s\n", q, sub_try[w] ? "subspace next" : "full next");
    }
    return KeptSpace{Gd + (long long)(k - r) * k, sG};
  }
  // The slices times the projector on the kept space (rank), or with the eigenvectors scaled to the shrunk singular values
  // (nuclear norm: all k of them, slices inside the ball keep their values bit for bit, flag = 0), rounded back to TF once.
  void apply_truncation(T* v, KeptSpace kept) {
    hipStream_t s = stream;
    const long long sU = (long long)m * k, sV = (long long)k * n, sA = (long long)m * n;
    const auto N_ = rocblas_operation_none, T_ = rocblas_operation_transpose;
    const int* keep_flag = nullptr;
    int inner = r;
    const double *Esel = kept.E, *Escl = kept.E;
    long long stride = kept.stride;
    if (sp.kind == EXT_NUCLEAR) {
      hipLaunchKernelGGL(k_nuc_factors, dim3((batch + 63) / 64), dim3(64), 0, s, k, batch, sp.pmax, Wd, Sd, flag);
      hipLaunchKernelGGL(k_scale_eigvecs, dim3(NB), dim3(BLOCK), 0, s, k, batch, Gd, Sd, Gs);
      keep_flag = flag;
      inner = k;
      Esel = Gd;
      Escl = Gs;
      stride = (long long)k * k;
    }
    if (right()) {     // X <- (X * Escl) * Esel'
      blas_check(gemm_sbx(blas, N_, N_, m, inner, k, 1.0, Ad, m, sA, Escl, k, stride, 0.0, Ud, m, sU, batch, 1), "gemm X V");
      blas_check(gemm_sbx(blas, N_, T_, m, n, inner, 1.0, Ud, m, sU, Esel, k, stride, 0.0, Ad, m, sA, batch, 1), "gemm (XV) V'");
    } else {           // X <- Escl * (Esel' * X)
      blas_check(gemm_sbx(blas, T_, N_, inner, n, k, 1.0, Esel, k, stride, Ad, m, sA, 0.0, Vd, k, sV, batch, 1), "gemm U' X");
      blas_check(gemm_sbx(blas, N_, N_, m, n, inner, 1.0, Escl, k, stride, Vd, k, sV, 0.0, Ad, m, sA, batch, 1), "gemm U (U'X)");
    }
    hipLaunchKernelGGL((k_seg_scatter<T, double>), dim3(NB), dim3(BLOCK), 0, s, map, Ad, v, keep_flag);
    SIPX_HIP(hipGetLastError());
  }
  // Float64 models: batched one-sided Jacobi SVD of the slices themselves, U_r S_r V_r' as one product.
  void jacobi_svd_route(T* v) {
    hipStream_t s = stream;
    const long long sU = (long long)m * k, sV = (long long)k * n, sA = (long long)m * n;
    blas_check(rocsolver_dgesvdj_strided_batched(blas, rocblas_svect_singular, rocblas_svect_singular, m, n, Ad, m, sA, 0.0, Ed, 100,
                                                 info + batch, Sd, k, Ud, m, sU, Vd, k, sV, info, batch),
               "gesvdj");
    note_status(s, Ed, Sd, k);
    int inner = r;
    const int* keep_flag = nullptr;
    if (sp.kind == EXT_NUCLEAR) {     // slices already inside the ball keep their values bit for bit (flag = 0)
      hipLaunchKernelGGL(k_nuc_shrink, dim3((batch + 63) / 64), dim3(64), 0, s, k, batch, sp.pmax, Sd, flag);
      inner = k;
      keep_flag = flag;
    }
    hipLaunchKernelGGL((k_scale_cols<double>), dim3(NB), dim3(BLOCK), 0, s, m, inner, m, sU, (long long)k, batch, Ud, Sd);
    const double one = 1.0, zero = 0.0;
    blas_check(rocblas_dgemm_strided_batched(blas, rocblas_operation_none, rocblas_operation_none, m, n, inner, &one, Ud, m, sU, Vd, k, sV,
                                             &zero, Ad, m, sA, batch),
               "gemm");
    hipLaunchKernelGGL((k_seg_scatter<T, double>), dim3(NB), dim3(BLOCK), 0, s, map, Ad, v, keep_flag);
    SIPX_HIP(hipGetLastError());
  }

  // v <- P(v): the slices widened to float64 whatever TF is (rocSOLVER's gesvdj works on A'A, condition number squared; the
  // truncated product is rounded back once), then the decision between the routes.  Only the span of the top-r eigenvectors of a
  // slice's Gram matrix is needed, and it moves little from one PARSDMM iteration to the next: the rank projector first tries
  // to follow it from the previous call's vectors -- the filtered iteration by default, the plain one with SIPX_RANK_CHEB=0 --
  // and decomposes fully where that is not possible or not accepted (no start for the plain route, slow contraction, a failed
  // factorisation or certificate); the full decomposition provides the next warm start.
  void project(T* v, bool feas, double*, T*, T*) override {
    check_status();
    if (sp.kind == EXT_RANK && r >= k) return;              // nothing to truncate
    hipLaunchKernelGGL((k_seg_gather<T, double>), dim3(NB), dim3(BLOCK), 0, stream, map, v, Ad);
    if (!gram) return jacobi_svd_route(v);
    form_gram();
    const int w = feas ? 1 : 0;
    bool sub_ok = false;
    if (sub_b > 0 && cheb) {
      const bool cold = !sub_have[w];
      if (cold && nothing_to_project()) {
        if (knobs.dbg) fprintf(stderr, "[sipx rank] every slice is zero: nothing to project\n");
        ++n_calls; ++n_subspace;
        return;
      }
      sub_ok = try_filtered_route(w, cold);
    } else if (sub_b > 0 && sub_have[w] && sub_try[w]) {
      sub_ok = try_plain_subspace(w);
    }
    ++n_calls;
    if (sub_ok) ++n_subspace; else ++n_full;
    // (Ritz values ascend: the last r columns of the block span the top-r space)
    apply_truncation(v, sub_ok ? KeptSpace{Xs[w] + (long long)(sub_b - r) * k, (long long)k * sub_b} : full_decomposition(w));
  }
};

template <typename T>
ExtImpl<T>* make_rank_family(const ExtSpec& spec, hipStream_t stream) { return new RankFamily<T>(spec, stream); }
template ExtImpl<float>* make_rank_family<float>(const ExtSpec&, hipStream_t);
template ExtImpl<double>* make_rank_family<double>(const ExtSpec&, hipStream_t);

}  // namespace sipx
