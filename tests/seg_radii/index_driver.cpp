// Host-side driver of the per-segment radius index of csrc/seg_norm.h (tests/test_seg_radii_cpu.py).  seg_tile_index is a
// __host__ __device__ function, so the walk the kernel makes over (tile, f) runs here without a GPU.  No HIP call is made.
//
// stdin, one request per line:
//   shape <ndim> <n0> <n1> <n2> <mode 1|2> <dir>
//       -> "index bytes <4|8> nseg <nseg> tiles <ntiles> F <F> dead <lanes of ragged tiles without a segment>", for float and double, on
//          the identity's extents and on those of each difference operator, after checking that
//            every s in 0 .. nseg-1 is hit by exactly one (tile, f),
//            the base address of that (tile, f) is seg_addr(m, s, 0),
//            a lane for which seg_tile_base reports no segment yields the index -1, and no other lane does.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "seg_norm.h"

using namespace sipx;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { ++fails; std::printf("FAIL " __VA_ARGS__); std::printf("\n"); } } while (0)

static void walk(const ExtSpec& sp, int elem_bytes, bool print) {
  const SegMap m = make_segmap(sp);
  const SegNormPlan p = seg_norm_plan(m, elem_bytes);
  std::vector<int> hits((size_t)m.nseg, 0);
  long long dead = 0;
  for (long long tile = 0; tile < p.ntiles; ++tile)
    for (int f = 0; f < p.F; ++f) {
      long long base;
      const bool live = seg_tile_base(m, p, tile, f, base);
      const long long s = seg_tile_index(m, p, tile, f);
      if (!live) {
        ++dead;
        CHECK(s == -1, "dead lane (tile %lld, f %d) yields index %lld", tile, f, s);
        continue;
      }
      if (s < 0 || s >= m.nseg) { CHECK(false, "index %lld of (tile %lld, f %d) outside 0 .. %lld", s, tile, f, m.nseg - 1); continue; }
      ++hits[(size_t)s];
      CHECK(base == seg_addr(m, s, 0), "base of (tile %lld, f %d) is %lld, segment %lld starts at %lld", tile, f, base, s, seg_addr(m, s, 0));
    }
  for (long long s = 0; s < m.nseg; ++s)
    if (hits[(size_t)s] != 1) { CHECK(false, "segment %lld hit %d times", s, hits[(size_t)s]); break; }
  CHECK(dead == p.ntiles * p.F - m.nseg, "dead lanes %lld, expected %lld", dead, p.ntiles * p.F - m.nseg);
  if (print) std::printf("index bytes %d nseg %lld tiles %lld F %d dead %lld\n", elem_bytes, m.nseg, p.ntiles, p.F, dead);
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
    for (int a = 0; a < 3; ++a) sp.dims[a] = n[a];
    walk(sp, eb, true);
    for (int d = 0; d < ndim; ++d) {          // TD_n of D_x, D_y / D_z: one entry less along d
      if (n[d] < 2) continue;
      for (int a = 0; a < 3; ++a) sp.dims[a] = n[a] - (a == d ? 1 : 0);
      walk(sp, eb, false);
    }
  }
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    if (!(in >> cmd)) continue;
    if (cmd == "shape") do_shape(in);
    else CHECK(false, "unknown request %s", cmd.c_str());
  }
  if (fails) std::printf("failed %d\n", fails);
  else std::printf("ok\n");
  return fails ? 1 : 0;
}
