// csrc/l2inf.h on the CPU (tests/test_l2inf_cpu.py): the rule of one group of the l2,inf ball, one group per input line
//     <f|d> <n> <c> <m_0> ... <m_{n-1}> <v_0> ... <v_{n-1}>          (n <= 16 entries; m_q: 1 a member, 0 a row the block does not have;
//                                                                    c and v in hexadecimal floating point, or inf / nan)
// -> "g <norm> clipped <0|1> y <n entries>" in the precision asked for: l2inf_group on a copy of v; and
//     units <f|d> <m>    -> "units <l2inf_excess_units(m)>"
//     shape <M> <B>      -> "shape <G>" or "error <message>"
//     vector <f|d> <per> <stacked 0|1> <c_0> ... -> "vector ok" or "error <message>": l2inf_check_vector with the member rule of set_config.h
// hipcc compiles it (the header needs the HIP headers); the program makes no HIP call.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "l2inf.h"

template <typename T>
static int one(std::istringstream& in) {
  int n = 0;
  std::string w;
  if (!(in >> n >> w) || n < 0 || n > 16) return 1;
  const T c = (T)std::strtod(w.c_str(), nullptr);
  bool member[16];
  T v[16];
  for (int q = 0; q < n; ++q) {
    int m = 0;
    if (!(in >> m)) return 1;
    member[q] = m != 0;
  }
  for (int q = 0; q < n; ++q) {
    if (!(in >> w)) return 1;
    v[q] = (T)std::strtod(w.c_str(), nullptr);
  }
  const T g = sipx::l2inf_group<T>(v, member, n, c);
  std::printf("g %a clipped %d y", (double)g, (int)sipx::l2inf_clipped<T>(g, c));
  for (int q = 0; q < n; ++q) std::printf(" %a", (double)v[q]);
  std::printf("\n");
  return 0;
}

template <typename T>
static void vector_check(std::istringstream& in) {
  long long per = 0;
  int stacked = 0;
  in >> per >> stacked;
  std::vector<T> c;
  std::string w;
  while (in >> w) c.push_back((T)std::strtod(w.c_str(), nullptr));
  sipx::l2inf_check_vector<T>(c.data(), (long long)c.size(), [&](long long p) { return stacked || p % per != per - 1; });
  std::printf("vector ok\n");
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    std::string tf;
    in >> tf;
    try {
      if (tf == "units") {
        std::string t;
        long long m = 0;
        in >> t >> m;
        std::printf("units %a\n", t == "f" ? sipx::l2inf_excess_units<float>(m) : sipx::l2inf_excess_units<double>(m));
        continue;
      }
      if (tf == "shape") {
        long long M = 0, B = 0;
        in >> M >> B;
        std::printf("shape %lld\n", sipx::l2infs_check_shape(M, B));
        continue;
      }
      if (tf == "vector") {
        std::string t;
        in >> t;
        if (t == "f") vector_check<float>(in); else vector_check<double>(in);
        continue;
      }
    } catch (const std::exception& e) {
      std::printf("error %s\n", e.what());
      continue;
    }
    const int bad = tf == "f" ? one<float>(in) : (tf == "d" ? one<double>(in) : 1);
    if (bad) {
      std::printf("FAIL cannot read: %s\n", line.substr(0, 200).c_str());
      return 1;
    }
  }
  std::printf("ok\n");
  return 0;
}
