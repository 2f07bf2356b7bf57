// csrc/l1_weighted.h on the CPU: the whole projection serially (hexadecimal floating point)
//     p <f|d> <tau> <n> <v_0> <w_0> ... <v_{n-1}> <w_{n-1}>
// -> "p <need> <theta> <(T)asum> <passes> <y_0> ... <y_{n-1}>" of l1w_project_serial
//     a <f|d> <v> <w> <theta>
// -> "a <y>", y = l1w_shrink(v, w, theta) for an entry whose cleaned weight is > 0, v itself otherwise
// hipcc compiles it (the header needs the HIP headers); the program makes no HIP call.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "l1_weighted.h"

static double num(std::istringstream& in) {
  std::string w;
  in >> w;
  return std::strtod(w.c_str(), nullptr);      // ("nan", "inf" and hexadecimal forms alike)
}

template <typename T>
static void project(std::istringstream& in) {
  const T tau = (T)num(in);
  long long n = 0;
  in >> n;
  std::vector<T> v((size_t)n), w((size_t)n);
  for (long long k = 0; k < n; ++k) {
    v[(size_t)k] = (T)num(in);
    w[(size_t)k] = (T)num(in);
  }
  T theta = T(0);
  double asum = 0.0;
  int passes = 0;
  const int need = sipx::l1w_project_serial<T>(v.data(), w.data(), n, tau, theta, asum, passes);
  std::printf("p %d %a %a %d", need, (double)theta, (double)(T)asum, passes);
  for (long long k = 0; k < n; ++k) std::printf(" %a", (double)v[(size_t)k]);
  std::printf("\n");
}

template <typename T>
static void apply(std::istringstream& in) {
  const T v = (T)num(in), w = sipx::l21w_clean<T>((T)num(in)), theta = (T)num(in);
  std::printf("a %a\n", (double)(w > T(0) ? sipx::l1w_shrink<T>(v, w, theta) : v));
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    std::string what, tf;
    in >> what >> tf;
    const bool f32 = tf == "f";
    if ((what != "p" && what != "a") || (!f32 && tf != "d")) {
      std::printf("FAIL cannot read: %s\n", line.c_str());
      return 1;
    }
    if (what == "p") { if (f32) project<float>(in); else project<double>(in); }
    else { if (f32) apply<float>(in); else apply<double>(in); }
  }
  std::printf("ok\n");
  return 0;
}
