// csrc/l21_weighted.h on the CPU: the weighted Michelot search serially, and the factor of one group (hexadecimal floating point)
//     s <f|d> <tau> <n> <g_0> <w_0> ... <g_{n-1}> <w_{n-1}>
// -> "s <need> <theta> <(T)asum> <passes>" of l21w_search_serial
//     a <f|d> <g> <w> <theta> <v>
// -> "a <factor> <y>", y = v * factor for a group whose cleaned weight is > 0, v itself otherwise
// hipcc compiles it (the header needs the HIP headers); the program makes no HIP call.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "l21_weighted.h"

static double num(std::istringstream& in) {
  std::string w;
  in >> w;
  return std::strtod(w.c_str(), nullptr);      // ("nan", "inf" and hexadecimal forms alike)
}

template <typename T>
static void search(std::istringstream& in) {
  const T tau = (T)num(in);
  long long n = 0;
  in >> n;
  std::vector<T> g((size_t)n), w((size_t)n);
  for (long long k = 0; k < n; ++k) {
    g[(size_t)k] = (T)num(in);
    w[(size_t)k] = (T)num(in);
  }
  T theta = T(0);
  double asum = 0.0;
  int passes = 0;
  const int need = sipx::l21w_search_serial<T>(g.data(), w.data(), n, tau, theta, asum, passes);
  std::printf("s %d %a %a %d\n", need, (double)theta, (double)(T)asum, passes);
}

template <typename T>
static void apply(std::istringstream& in) {
  const T g = (T)num(in), w = sipx::l21w_clean<T>((T)num(in)), theta = (T)num(in), v = (T)num(in);
  const T f = sipx::l21w_factor<T>(g, w, theta);
  std::printf("a %a %a\n", (double)f, (double)(w > T(0) ? v * f : v));
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    std::string what, tf;
    in >> what >> tf;
    const bool f32 = tf == "f";
    if ((what != "s" && what != "a") || (!f32 && tf != "d")) {
      std::printf("FAIL cannot read: %s\n", line.c_str());
      return 1;
    }
    if (what == "s") { if (f32) search<float>(in); else search<double>(in); }
    else { if (f32) apply<float>(in); else apply<double>(in); }
  }
  // a weight that is not >= 0 and finite counts as 0
  if (sipx::l21w_clean<float>(-1.f) != 0.f || sipx::l21w_clean<float>(NAN) != 0.f || sipx::l21w_clean<double>(INFINITY) != 0.0 ||
      sipx::l21w_clean<double>(0.25) != 0.25 || sipx::l21w_clean<float>(-0.f) != 0.f) {
    std::printf("FAIL l21w_clean\n");
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
