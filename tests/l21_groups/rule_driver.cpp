// csrc/l21_groups.h on the CPU (tests/test_l21_groups_cpu.py): the plan of the norms launch and the rule on the segment norms are host
// functions, so they run here without a GPU.  hipcc compiles it (the headers need the HIP headers); the program makes no HIP call.
//
// stdin, one request per line (hexadecimal floating point):
//   plan <ndim> <n0> <n1> <n2> <op dir, -1: identity> <mode 1|2> <dir>
//       -> "plan bytes <4|8> slices . path . F . tiles_ragged . L . nseg . chunk . nchunk . last . vw . grid ." for float and double, after
//          walking every (workgroup, thread, element) of a slice plan: each valid entry of the block exactly once, nothing else, every
//          address inside the grid, every partial slot written once
//   r <f|d> <tau> <n> <weights 0|1> <g_0> <w_0> ... <g_{n-1}> <w_{n-1}>
//       -> "r <need> <theta> <(T)asum> <passes> <f_0> ... <f_{n-1}>" of l21g_rule_serial (weights 0: w is not passed)
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "l21_groups.h"

using namespace sipx;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { ++fails; std::printf("FAIL " __VA_ARGS__); std::printf("\n"); } } while (0)

static double num(std::istringstream& in) {
  std::string w;
  in >> w;
  return std::strtod(w.c_str(), nullptr);
}

// the walk of k_l21g_part: workgroup b = (tile, chunk), thread tid = (f, r), elements t0 + r vw + k, stride G vw
static void walk_slices(const ExtSpec& sp, const SegMap& m, const L21GroupsPlan& p) {
  const long long N = sp.G.N;
  std::vector<int> seen((size_t)N, 0), slot((size_t)(p.ntA * p.F * p.nchunk), 0);
  CHECK(p.F >= 1 && (p.F & (p.F - 1)) == 0 && (1 << p.logF) == p.F && BLOCK % p.F == 0, "F = %d", p.F);
  CHECK(p.chunk >= p.vw && p.chunk % p.vw == 0, "chunk %lld vw %d", p.chunk, p.vw);
  CHECK(p.grid == p.ntA * p.nchunk && p.grid < (1ll << 31), "grid");
  CHECK((p.nchunk - 1) * p.chunk < m.L && p.nchunk * p.chunk >= m.L, "chunks cover L");
  const int G = BLOCK >> p.logF;
  for (long long b = 0; b < p.grid; ++b) {
    const long long c = b % p.nchunk, tile = b / p.nchunk;
    for (int tid = 0; tid < BLOCK; ++tid) {
      const int f = tid & (p.F - 1), r = tid >> p.logF;
      const long long sa = tile * p.F + f;
      if (sa >= m.nseg) continue;
      for (long long t = p.t0(c) + (long long)r * p.vw; t < p.t1(c, m.L); t += (long long)G * p.vw)
        for (int k = 0; k < p.vw; ++k) {
          if (t + k >= p.t1(c, m.L)) continue;
          const long long a = sa * m.sSa + seg_toff(m, t + k);
          if (a != seg_addr(m, sa, t + k) || a < 0 || a >= N) { CHECK(false, "address of s = %lld t = %lld: %lld", sa, t + k, a); return; }
          ++seen[(size_t)a];
        }
      if (tid < p.F) ++slot[(size_t)(sa * p.nchunk + c)];
    }
  }
  for (long long k = 0; k < sp.G.n[2]; ++k)
    for (long long j = 0; j < sp.G.n[1]; ++j)
      for (long long i = 0; i < sp.G.n[0]; ++i) {
        const bool valid = i < sp.dims[0] && j < sp.dims[1] && k < sp.dims[2];
        const int c = seen[(size_t)(i * sp.G.st[0] + j * sp.G.st[1] + k * sp.G.st[2])];
        if (c != (valid ? 1 : 0)) { CHECK(false, "entry (%lld, %lld, %lld) visited %d times", i, j, k, c); return; }
      }
  for (long long s = 0; s < m.nseg * p.nchunk; ++s)
    if (slot[(size_t)s] != 1) { CHECK(false, "partial %lld written %d times", s, slot[(size_t)s]); return; }
}

static void do_plan(std::istringstream& in) {
  ExtSpec sp;
  int ndim, opdir, mode, dir;
  long long n[3];
  in >> ndim >> n[0] >> n[1] >> n[2] >> opdir >> mode >> dir;
  sp.ndim = ndim; sp.mode = mode; sp.dir = dir;
  sp.G.N = n[0] * n[1] * n[2];
  sp.G.st[0] = 1; sp.G.st[1] = n[0]; sp.G.st[2] = n[0] * n[1];
  for (int a = 0; a < 3; ++a) { sp.G.n[a] = n[a]; sp.dims[a] = n[a] - (a == opdir ? 1 : 0); }
  const SegMap m = make_segmap(sp);
  for (int eb = 4; eb <= 8; eb += 4) {
    const L21GroupsPlan p = l21_groups_plan(m, mode, eb);
    const SegNormPlan t = seg_norm_plan(m, eb);
    if (p.slices) walk_slices(sp, m, p);
    else CHECK(p.fiber.lds == 0 && p.fiber.lds_bytes == 0 && p.fiber.F == t.F && p.grid == (long long)t.grid, "the fiber plan is seg_norm_plan's");
    std::printf("plan bytes %d slices %d path %d F %d tiles_ragged %d L %lld nseg %lld chunk %lld nchunk %lld last %lld vw %d grid %lld\n", eb,
                p.slices, t.path(), p.slices ? p.F : t.F, (int)(m.SA % t.F != 0), m.L, m.nseg, p.chunk, p.nchunk,
                m.L - (p.nchunk - 1) * p.chunk, p.vw, p.grid);
  }
}

template <typename T>
static void rule(std::istringstream& in) {
  const T tau = (T)num(in);
  long long n = 0;
  int hasw = 0;
  in >> n >> hasw;
  std::vector<T> g((size_t)n), w((size_t)n), f((size_t)n);
  for (long long k = 0; k < n; ++k) {
    g[(size_t)k] = (T)num(in);
    w[(size_t)k] = (T)num(in);
  }
  T theta = T(0);
  double asum = 0.0;
  int passes = 0;
  const int need = l21g_rule_serial<T>(g.data(), hasw ? w.data() : nullptr, n, tau, theta, asum, passes, f.data());
  std::printf("r %d %a %a %d", need, (double)theta, (double)(T)asum, passes);
  for (long long k = 0; k < n; ++k) std::printf(" %a", (double)f[(size_t)k]);
  std::printf("\n");
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    std::string what;
    in >> what;
    if (what == "plan") {
      do_plan(in);
    } else if (what == "r") {
      std::string tf;
      in >> tf;
      if (tf == "f") rule<float>(in);
      else if (tf == "d") rule<double>(in);
      else { std::printf("FAIL cannot read: %s\n", line.c_str()); return 1; }
    } else {
      std::printf("FAIL cannot read: %s\n", line.c_str());
      return 1;
    }
  }
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
