// csrc/l21.h on the CPU: the group norm and the weight of the l2,1 ball, one group per input line
//     <f|d> <member mask, bit q: block q has a row> <v0> <v1> <v2> <theta>      (hexadecimal floating point)
// -> "g <norm> <weight> <y0> <y1> <y2>" in the precision asked for, y_q = v_q * weight for the members, v_q itself otherwise
// (a row a block does not have is not written), and the Float64 threshold of an active set, added serially in the given order
//     theta <tau> <theta of the search> <n> <g_0> ... <g_{n-1}>
// -> "theta <l21_theta_refined of the g above the search's theta>".  hipcc compiles it (the header needs the HIP headers); the program makes no HIP call.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "l21.h"

template <typename T>
static int one(std::istringstream& in) {
  int mask = 0;
  std::string w[4];
  if (!(in >> mask >> w[0] >> w[1] >> w[2] >> w[3])) return 1;
  T v[3];
  bool member[3];
  for (int q = 0; q < 3; ++q) {
    v[q] = (T)std::strtod(w[q].c_str(), nullptr);
    member[q] = (mask >> q) & 1;
  }
  const T theta = (T)std::strtod(w[3].c_str(), nullptr);
  const T g = sipx::l21_group_norm<T>(v, member, 3);
  const T f = sipx::l21_weight<T>(g, theta);
  std::printf("g %a %a", (double)g, (double)f);
  for (int q = 0; q < 3; ++q) std::printf(" %a", (double)(member[q] ? v[q] * f : v[q]));
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
    const int bad = tf == "f" ? one<float>(in) : (tf == "d" ? one<double>(in) : 1);
    if (bad) {
      std::printf("FAIL cannot read: %s\n", line.c_str());
      return 1;
    }
  }
  // the membership rule: a point on the far face along a direction has no row in that block
  if (sipx::l21_member(3, 5) != true || sipx::l21_member(4, 5) != false || sipx::l21_member(0, 1) != false) {
    std::printf("FAIL l21_member\n");
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
