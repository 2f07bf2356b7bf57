// Host-side driver of csrc/seg_norm.h (tests/test_seg_norms_cpu.py): the plan of a launch and the threshold rule of a segment are
// __host__ __device__ functions, so they run here without a GPU.  No HIP call is made.
//
// stdin, one request per line:
//   shape <ndim> <n0> <n1> <n2> <mode 1|2> <dir>
//       -> "plan ..." for float and double, after walking every (tile, lane segment, element) of the plan on the identity's extents
//          and on those of each difference operator: the addresses must be those of seg_addr, inside the grid, each valid entry once
//   l1 <f|d> <b> <L> <v_0> ... <v_{L-1}>         (hex floats)
//       -> "theta <need> <theta as a hex double> <Michelot steps>": the serial iteration with the kernel's own step functions
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "seg_norm.h"

using namespace sipx;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { ++fails; std::printf("FAIL " __VA_ARGS__); std::printf("\n"); } } while (0)

static long long walk(const ExtSpec& sp, int elem_bytes, SegNormPlan& p, SegMap& m) {
  m = make_segmap(sp);
  p = seg_norm_plan(m, elem_bytes);
  const long long N = sp.G.N;
  std::vector<int> seen((size_t)N, 0);
  long long visited = 0;
  CHECK(p.F >= 1 && p.F <= 64 && (p.F & (p.F - 1)) == 0 && (1 << p.logF) == p.F && BLOCK % p.F == 0, "F = %d", p.F);
  CHECK(p.grid >= 1 && (long long)p.grid <= p.ntiles && (long long)p.grid <= SEGN_MAX_GRID, "grid");
  CHECK((long long)p.lds_bytes <= SEGN_LDS_BYTES && (!p.lds || (long long)p.lds_bytes == p.F * m.L * elem_bytes), "LDS bytes");
  CHECK(p.lds == (p.F * m.L * elem_bytes <= SEGN_LDS_BYTES ? 1 : 0), "LDS rule");
  CHECK(m.L < (1ll << 31), "L");
  for (long long tile = 0; tile < p.ntiles; ++tile)
    for (int f = 0; f < p.F; ++f) {
      long long base;
      if (!seg_tile_base(m, p, tile, f, base)) continue;
      const long long s = (tile % p.ntA) * p.F + f + m.SA * (tile / p.ntA);
      CHECK(s < m.nseg, "segment index");
      for (long long t = 0; t < m.L; ++t) {
        const long long a = base + seg_toff(m, t);
        if (a != seg_addr(m, s, t) || a < 0 || a >= N) { CHECK(false, "address of s = %lld t = %lld: %lld", s, t, a); return -1; }
        ++seen[(size_t)a];
        ++visited;
      }
    }
  // every entry of the valid block once, nothing else
  for (long long k = 0; k < sp.G.n[2]; ++k)
    for (long long j = 0; j < sp.G.n[1]; ++j)
      for (long long i = 0; i < sp.G.n[0]; ++i) {
        const bool valid = i < sp.dims[0] && j < sp.dims[1] && k < sp.dims[2];
        const int c = seen[(size_t)(i * sp.G.st[0] + j * sp.G.st[1] + k * sp.G.st[2])];
        if (c != (valid ? 1 : 0)) { CHECK(false, "entry (%lld, %lld, %lld) visited %d times", i, j, k, c); return -1; }
      }
  CHECK(visited == m.nseg * m.L, "visited");
  return visited;
}

static void do_shape(std::istringstream& in) {
  ExtSpec sp;
  int ndim, mode, dir;
  long long n[3];
  in >> ndim >> n[0] >> n[1] >> n[2] >> mode >> dir;
  sp.ndim = ndim; sp.mode = mode; sp.dir = dir;
  sp.G.n[0] = n[0]; sp.G.n[1] = n[1]; sp.G.n[2] = n[2];
  sp.G.N = n[0] * n[1] * n[2];
  sp.G.st[0] = 1; sp.G.st[1] = n[0]; sp.G.st[2] = n[0] * n[1];
  for (int eb = 4; eb <= 8; eb += 4) {
    SegNormPlan p, q;
    SegMap m, mq;
    for (int a = 0; a < 3; ++a) sp.dims[a] = n[a];
    walk(sp, eb, p, m);
    for (int d = 0; d < ndim; ++d) {          // TD_n of D_x, D_y / D_z: one entry less along d, the pads are never touched
      if (n[d] < 2) continue;
      for (int a = 0; a < 3; ++a) sp.dims[a] = n[a] - (a == d ? 1 : 0);
      walk(sp, eb, q, mq);
    }
    std::printf("plan bytes %d path %d F %d lds %d ntiles %lld grid %u L %lld nseg %lld ragged %lld\n", eb, p.path(), p.F, p.lds, p.ntiles,
                p.grid, m.L, m.nseg, m.SA % p.F);
  }
}

template <typename T>
static void do_l1(std::istringstream& in) {
  std::string tok;
  long long L;
  in >> tok;
  const T b = (T)std::strtod(tok.c_str(), nullptr);
  in >> L;
  std::vector<T> v((size_t)L);
  for (auto& x : v) { in >> tok; x = (T)std::strtod(tok.c_str(), nullptr); }
  double asum = 0, vmin = INFINITY;
  for (T x : v) { const double a = std::fabs((double)x); asum += a; vmin = a < vmin ? a : vmin; }
  const bool need = !((T)asum <= b);
  double theta = 0;
  long long steps = 0;
  if (need) {
    L1SegState st = l1_seg_start(asum, (double)b, L);
    for (long long it = 0; it <= L + 1 && !st.done; ++it, ++steps) {
      double S = 0, C = 0;
      for (T x : v) { const double a = std::fabs((double)x); if (a > st.theta) { S += a; C += 1.0; } }
      l1_seg_step(st, S, C, (double)b);
    }
    CHECK(st.done, "Michelot's iteration did not end within L + 2 steps");
    theta = l1_seg_finish(st, asum, vmin, (double)b, L);
  }
  std::printf("theta %d %a %lld\n", need ? 1 : 0, theta, steps);
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    if (cmd == "shape") do_shape(in);
    else if (cmd == "l1") {
      std::string tf;
      in >> tf;
      if (tf == "f") do_l1<float>(in); else do_l1<double>(in);
    } else CHECK(false, "unknown request %s", cmd.c_str());
  }
  if (fails) std::printf("failed %d\n", fails);
  else std::printf("ok\n");
  return fails ? 1 : 0;
}
