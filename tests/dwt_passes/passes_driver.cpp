// The work items of the db4 axis passes (kernels_dwt.hip: pass_item<T, INV, R>, fwd_run, inv_run) on the CPU against the direct
// formula of dwt.h.  Built with hipcc (the file pulls in the HIP headers) but makes no HIP call: the item functions are
// __host__ __device__ and run here as plain host code.
//
// stdin: one line of the 8 low-pass and one of the 8 high-pass coefficients (hex floats, from tests/dwt_ref.py), then one line
// "ndim n0 n1 n2 b0 b1 b2" per box: a level's box b of the grid n.  Every box runs in float and double, forward and inverse,
// with R = 1, RC and RS outputs per item, along every axis, from the grid's strides into a compact box and back (level 1: both
// are the grid's).  Source and destination carry GUARD elements on each side.  The source is NaN outside the box, guards and the
// gaps between the box's lines alike, so a read outside the box shows as a NaN in the result; the destination is checked for
// being untouched outside the box.
// stdout: one line per box "box ... passes P err_f E err_d E", then "ok" or "FAILED"; a line "FAIL ..." per failing pass.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "kernels_dwt.hip"

namespace {

constexpr long long GUARD = 64;
double LO[8], HI[8];

struct Lcg {                         // values in [-1, 1): the same on every platform
  unsigned long long s;
  double next() {
    s = s * 6364136223846793005ULL + 1442695040888963407ULL;
    return (double)(long long)(s >> 11) / 4503599627370496.0 - 1.0;
  }
};

// one level along a line of length m, in double: y <- W x (a to [0, m/2), d to [m/2, m)) or y <- W' x
void line_ref(const std::vector<double>& x, std::vector<double>& y, int m, bool inv) {
  const int h = m / 2;
  for (int i = 0; i < m; ++i) y[i] = 0.0;
  for (int k = 0; k < h; ++k)
    for (int j = 0; j < 8; ++j) {
      const int i = (int)((((2LL * k + 4 - j) % m) + m) % m);
      if (inv) {
        y[i] += LO[j] * x[k] + HI[j] * x[h + k];
      } else {
        y[k] += LO[j] * x[i];
        y[h + k] += HI[j] * x[i];
      }
    }
}

template <typename T>
bool same_bits(T a, T b) { return std::memcmp(&a, &b, sizeof(T)) == 0; }

int failures = 0;

// one pass of the box b (strides 1, s1, s2 in src; 1, d1, d2 in dst) along axis: returns the largest error
template <typename T, bool INV, int R>
double run_pass(const long long* b, int axis, long long s1, long long s2, long long d1, long long d2, Lcg& rng, double tol,
                const char* what) {
  const long long sext = (b[0] - 1) + (b[1] - 1) * s1 + (b[2] - 1) * s2 + 1;
  const long long dext = (b[0] - 1) + (b[1] - 1) * d1 + (b[2] - 1) * d2 + 1;
  const T fence = (T)-7777.25;
  std::vector<T> src((size_t)(sext + 2 * GUARD), std::numeric_limits<T>::quiet_NaN());
  std::vector<T> dst((size_t)(dext + 2 * GUARD), fence);
  std::vector<char> inbox((size_t)(dext + 2 * GUARD), 0);
  for (long long i2 = 0; i2 < b[2]; ++i2)
    for (long long i1 = 0; i1 < b[1]; ++i1)
      for (long long i0 = 0; i0 < b[0]; ++i0) {
        src[(size_t)(GUARD + i0 + i1 * s1 + i2 * s2)] = (T)rng.next();
        inbox[(size_t)(GUARD + i0 + i1 * d1 + i2 * d2)] = 1;
      }
  sipx::PassArgs a;
  a.s1 = s1; a.s2 = s2; a.d1 = d1; a.d2 = d2;
  a.b0 = (int)b[0]; a.b1 = (int)b[1]; a.b2 = (int)b[2]; a.axis = axis;
  const unsigned items = sipx::pass_items<R>(a);
  for (unsigned t = 0; t < items; ++t) sipx::pass_item<T, INV, R>(src.data() + GUARD, dst.data() + GUARD, a, t);

  bool ok = true;
  for (size_t e = 0; e < dst.size(); ++e)
    if (!inbox[e] && !same_bits(dst[e], fence)) ok = false;            // a write outside the box
  const int m = (int)b[axis];
  const long long sst = axis == 0 ? 1 : (axis == 1 ? s1 : s2), dstd = axis == 0 ? 1 : (axis == 1 ? d1 : d2);
  std::vector<double> x((size_t)m), y((size_t)m);
  double err = 0.0;
  long long c[3];
  for (c[2] = 0; c[2] < (axis == 2 ? 1 : b[2]); ++c[2])
    for (c[1] = 0; c[1] < (axis == 1 ? 1 : b[1]); ++c[1])
      for (c[0] = 0; c[0] < (axis == 0 ? 1 : b[0]); ++c[0]) {
        const long long so = GUARD + c[0] + c[1] * s1 + c[2] * s2, dof = GUARD + c[0] + c[1] * d1 + c[2] * d2;
        for (int i = 0; i < m; ++i) x[(size_t)i] = (double)src[(size_t)(so + i * sst)];
        line_ref(x, y, m, INV);
        for (int i = 0; i < m; ++i) {
          const double d = std::fabs((double)dst[(size_t)(dof + i * dstd)] - y[(size_t)i]);
          if (!(d <= err)) err = d;                                    // a NaN sticks
        }
      }
  if (!(err <= tol)) ok = false;
  if (!ok) {
    ++failures;
    std::printf("FAIL %s %s R=%d axis=%d box %lld %lld %lld strides %lld %lld -> %lld %lld: err %.3e (bound %.1e)%s\n", what,
                INV ? "inverse" : "forward", R, axis, b[0], b[1], b[2], s1, s2, d1, d2, err, tol,
                err <= tol ? ", wrote outside the box" : "");
  }
  return err;
}

template <typename T>
double run_box(int ndim, const long long* n, const long long* b, Lcg& rng, double tol, const char* what, int& passes) {
  const long long f1 = n[0], f2 = n[0] * n[1], c1 = b[0], c2 = b[0] * b[1];
  double err = 0.0;
  auto up = [&](double e) { if (!(e <= err)) err = e; ++passes; };
  for (int lay = 0; lay < 2; ++lay) {
    const long long s1 = lay ? c1 : f1, s2 = lay ? c2 : f2, d1 = lay ? f1 : c1, d2 = lay ? f2 : c2;
    for (int axis = 0; axis < ndim; ++axis) {
      up(run_pass<T, false, 1>(b, axis, s1, s2, d1, d2, rng, tol, what));
      up(run_pass<T, true, 1>(b, axis, s1, s2, d1, d2, rng, tol, what));
      up(run_pass<T, false, sipx::RC>(b, axis, s1, s2, d1, d2, rng, tol, what));
      up(run_pass<T, true, sipx::RC>(b, axis, s1, s2, d1, d2, rng, tol, what));
      up(run_pass<T, false, sipx::RS>(b, axis, s1, s2, d1, d2, rng, tol, what));
      up(run_pass<T, true, sipx::RS>(b, axis, s1, s2, d1, d2, rng, tol, what));
    }
  }
  return err;
}

}  // namespace

int main() {
  for (int j = 0; j < 8; ++j)
    if (std::scanf("%lf", &LO[j]) != 1) return 2;
  for (int j = 0; j < 8; ++j)
    if (std::scanf("%lf", &HI[j]) != 1) return 2;
  Lcg rng{20240611ULL};
  int ndim;
  long long n[3], b[3];
  while (std::scanf("%d %lld %lld %lld %lld %lld %lld", &ndim, &n[0], &n[1], &n[2], &b[0], &b[1], &b[2]) == 7) {
    if ((ndim != 2 && ndim != 3) || b[0] < 2 || b[1] < 2 || b[2] < 1 || b[0] > n[0] || b[1] > n[1] || b[2] > n[2] ||
        b[0] % 2 || b[1] % 2 || (ndim == 3 && b[2] % 2) || (ndim == 2 && b[2] != 1))
      return 2;
    int passes = 0;
    const double ef = run_box<float>(ndim, n, b, rng, 2e-6, "float", passes);
    const double ed = run_box<double>(ndim, n, b, rng, 1e-13, "double", passes);
    std::printf("box %lld %lld %lld of %lld %lld %lld passes %d err_f %.3e err_d %.3e\n", b[0], b[1], b[2], n[0], n[1], n[2], passes,
                ef, ed);
  }
  std::puts(failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}
