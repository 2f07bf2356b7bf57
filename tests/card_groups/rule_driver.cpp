// csrc/card_groups.h on the CPU (tests/test_card_groups_cpu.py): the serial rule and the rank-by-counting rule of the small route are
// __host__ __device__ functions of a header that needs no HIP header, so a plain host compiler builds this program -- also with
// -fsanitize=address,undefined.  It makes no HIP call.
//
// stdin, one request per line (hexadecimal floating point):
//   s <f|d> <k> <n> <g_0> ... <g_{n-1}>
//       -> "s <need> <tau> <cut> <need> <tau> <cut> <keep_0 ... keep_{n-1} as one word of 0 / 1>": cardg_select_serial, then
//          cardg_select_by_rank, then cardg_kept of the first; the two selections are also compared here
//   k <f|d> <k as a double> <nseg>
//       -> "k ok" or "k <the refusal>" of cardg_check_k
//   c -> "c <CARDG_SMALL_MAX>"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "card_groups.h"

using namespace sipx;

static int fails = 0;

static double num(std::istringstream& in) {
  std::string w;
  in >> w;
  return std::strtod(w.c_str(), nullptr);
}

template <typename T>
static void select(std::istringstream& in) {
  long long k = 0, n = 0;
  in >> k >> n;
  std::vector<T> g((size_t)n);
  for (auto& x : g) x = (T)num(in);
  const CardGSel<T> a = cardg_select_serial<T>(g.data(), n, k), b = cardg_select_by_rank<T>(g.data(), n, k);
  if (a.need != b.need || !(a.tau == b.tau) || a.cut != b.cut) {
    ++fails;
    std::printf("FAIL the two rules differ: (%d, %a, %lld) against (%d, %a, %lld)\n", a.need, (double)a.tau, a.cut, b.need, (double)b.tau, b.cut);
  }
  std::vector<unsigned char> keep((size_t)(n > 0 ? n : 1));
  cardg_kept<T>(g.data(), n, a, keep.data());
  std::string word((size_t)n, '0');
  for (long long s = 0; s < n; ++s) word[(size_t)s] = keep[(size_t)s] ? '1' : '0';
  std::printf("s %d %a %lld %d %a %lld %s\n", a.need, (double)a.tau, a.cut, b.need, (double)b.tau, b.cut, n ? word.c_str() : "-");
}

template <typename T>
static void check_k(std::istringstream& in) {
  const double k = num(in);
  long long n = 0;
  in >> n;
  try {
    cardg_check_k<T>(k, n);
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
    if (what == "c") { std::printf("c %d\n", CARDG_SMALL_MAX); continue; }
    in >> prec;
    if (what == "s") { if (prec == "f") select<float>(in); else select<double>(in); }
    else if (what == "k") { if (prec == "f") check_k<float>(in); else check_k<double>(in); }
    else if (!what.empty()) { ++fails; std::printf("FAIL unknown request %s\n", what.c_str()); }
  }
  std::printf(fails ? "failed\n" : "ok\n");
  return fails ? 1 : 0;
}
