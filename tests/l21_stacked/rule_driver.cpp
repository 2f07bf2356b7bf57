// csrc/l21_stacked.h on the CPU (tests/test_l21_stacked_cpu.py): the group norm and the weight of the l2,1 ball across the blocks of a
// stacked operator, one array per input line
//     <f|d> <B> <G> <theta> <v_0> ... <v_{B G - 1}>                                    (hexadecimal floating point)
// -> "g <G norms>", "f <G weights>", "y <B G scaled entries>" in the precision asked for: g_p = l21s_group_norm, f_p = l21_weight(g_p, theta),
// y[q G + p] = l21s_scaled(v[q G + p], f_p); and the Float64 threshold of an active set, added serially in two halves that are merged
//     theta <tau> <theta of the search> <n> <g_0> ... <g_{n-1}>
// -> "theta <l21_theta_refined of the g above the search's theta>"; and the shape check
//     shape <M> <B>   -> "shape <G>" or "error <message>".
// hipcc compiles it (the header needs the HIP headers); the program makes no HIP call.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "l21_stacked.h"

template <typename T>
static int one(std::istringstream& in) {
  int B = 0;
  unsigned G = 0;
  std::string w;
  if (!(in >> B >> G >> w)) return 1;
  const T theta = (T)std::strtod(w.c_str(), nullptr);
  std::vector<T> v((size_t)B * G);
  for (T& x : v) {
    if (!(in >> w)) return 1;
    x = (T)std::strtod(w.c_str(), nullptr);
  }
  std::vector<T> g(G), f(G);
  for (unsigned p = 0; p < G; ++p) {
    g[p] = sipx::l21s_group_norm<T>(v.data(), B, G, p);
    f[p] = sipx::l21_weight<T>(g[p], theta);
  }
  std::printf("g");
  for (unsigned p = 0; p < G; ++p) std::printf(" %a", (double)g[p]);
  std::printf("\nf");
  for (unsigned p = 0; p < G; ++p) std::printf(" %a", (double)f[p]);
  std::printf("\ny");
  for (int q = 0; q < B; ++q)
    for (unsigned p = 0; p < G; ++p) std::printf(" %a", (double)sipx::l21s_scaled<T>(v[sipx::l21s_index((unsigned)q, G, p)], f[p]));
  std::printf("\n");
  return 0;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    std::string tf;
    in >> tf;
    if (tf == "theta") {
      std::string w;
      long long n = 0;
      in >> w;
      const double tau = std::strtod(w.c_str(), nullptr);
      in >> w;
      const double ths = std::strtod(w.c_str(), nullptr);
      in >> n;
      sipx::L21Sum acc{0.0, 0.0}, half{0.0, 0.0};
      double cnt = 0.0;
      for (long long k = 0; k < n && (in >> w); ++k) {
        const double a = std::strtod(w.c_str(), nullptr);
        if (!(a > ths)) continue;
        if (k % 2) sipx::l21_sum_add(half, a);           // two partial sums merged: the kernels' tree in small
        else sipx::l21_sum_add(acc, a);
        cnt += 1.0;
      }
      sipx::l21_sum_merge(acc, half);
      std::printf("theta %a\n", sipx::l21_theta_refined(acc, cnt, tau, (double)n, ths));
      continue;
    }
    if (tf == "shape") {
      long long M = 0, B = 0;
      in >> M >> B;
      try {
        std::printf("shape %lld\n", sipx::l21s_check_shape(M, B));
      } catch (const std::exception& e) {
        std::printf("error %s\n", e.what());
      }
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
