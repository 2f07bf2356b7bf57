// csrc/l20.h on the CPU (tests/test_l20_cpu.py): the serial selection, the per-frame radix select, the key of one group and the check of
// k are __host__ __device__ functions of a header that needs no HIP header, so a plain host compiler builds this program -- also with
// -fsanitize=address,undefined.  It makes no HIP call.
//
// stdin, one request per line (hexadecimal floating point):
//   s <f|d> <k> <n> <g_0> ... <g_{n-1}>
//       -> "s <need> <tau> <cut> <keep_0 ... keep_{n-1} as one word of 0 / 1>": l20_select_serial, then l20_kept
//   r <f|d> <k> <n> <g_0> ... <g_{n-1}>
//       -> "r <need> <tau> <cut> <keep word>": l20_frame_select (the radix select of k_l20_frames), then l20_kept
//   g <f|d> <nblk> <member_0> <v_0> ... -> "g <key>": l20_key
//   m <cd> <nd> -> "m <0|1>": l20_member
//   k <f|d> <k as a double> <ngroups> -> "k ok" or "k <the refusal>" of l20_check_k
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "l20.h"

using namespace sipx;

static int fails = 0;

static double num(std::istringstream& in) {
  std::string w;
  in >> w;
  return std::strtod(w.c_str(), nullptr);
}

template <typename T>
static void select(std::istringstream& in, bool radix) {
  long long k = 0, n = 0;
  in >> k >> n;
  std::vector<T> g((size_t)(n > 0 ? n : 1));
  for (long long s = 0; s < n; ++s) g[(size_t)s] = (T)num(in);
  const CardGSel<T> a = radix ? l20_frame_select<T>(g.data(), n, k) : l20_select_serial<T>(g.data(), n, k);
  std::vector<unsigned char> keep((size_t)(n > 0 ? n : 1));
  l20_kept<T>(g.data(), n, a, keep.data());
  std::string word((size_t)n, '0');
  for (long long s = 0; s < n; ++s) word[(size_t)s] = keep[(size_t)s] ? '1' : '0';
  std::printf("%c %d %a %lld %s\n", radix ? 'r' : 's', a.need, (double)a.tau, a.cut, n ? word.c_str() : "-");
}

template <typename T>
static void key(std::istringstream& in) {
  int nblk = 0;
  in >> nblk;
  if (nblk < 0 || nblk > 3) { ++fails; std::printf("FAIL nblk\n"); return; }
  T v[3] = {T(0), T(0), T(0)};
  bool mem[3] = {false, false, false};
  for (int q = 0; q < nblk; ++q) {
    int m = 0;
    in >> m;
    mem[q] = m != 0;
    v[q] = (T)num(in);
  }
  std::printf("g %a\n", (double)l20_key<T>(v, mem, nblk));
}

template <typename T>
static void check_k(std::istringstream& in) {
  const double k = num(in);
  long long n = 0;
  in >> n;
  try {
    l20_check_k<T>(k, n);
    std::printf("k ok\n");
  } catch (const std::exception& e) {
    std::printf("k %s\n", e.what());
  }
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what, prec;
    in >> what;
    if (what == "m") {
      int cd = 0, nd = 0;
      in >> cd >> nd;
      std::printf("m %d\n", l20_member(cd, nd) ? 1 : 0);
      continue;
    }
    in >> prec;
    const bool f = prec == "f";
    if (what == "s" || what == "r") { if (f) select<float>(in, what == "r"); else select<double>(in, what == "r"); }
    else if (what == "g") { if (f) key<float>(in); else key<double>(in); }
    else if (what == "k") { if (f) check_k<float>(in); else check_k<double>(in); }
    else if (!what.empty()) { ++fails; std::printf("FAIL unknown request %s\n", what.c_str()); }
  }
  std::printf(fails ? "failed\n" : "ok\n");
  return fails ? 1 : 0;
}
