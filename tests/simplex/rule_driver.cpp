// csrc/seg_simplex.h on the CPU (hexadecimal floating point)
//     p <f|d> <smin> <smax> <L> <stride> <a_0> ... <a_{(L-1) stride}>
// -> "p <case> <theta> <(T)spos> <steps> <a_0> ... " of simplex_project_serial on the entries a_0, a_stride, ...; the others are not its
//    business and come back as they went in
//     k <L> <LB> <sSa>
// -> "k <bucket>" of simplex_lane_bucket for a mapping with those three fields
// hipcc compiles it (the header needs the HIP headers); the program makes no HIP call.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "seg_simplex.h"

static double num(std::istringstream& in) {
  std::string w;
  in >> w;
  return std::strtod(w.c_str(), nullptr);      // ("nan", "inf" and hexadecimal forms alike)
}

template <typename T>
static void project(std::istringstream& in) {
  const T smin = (T)num(in), smax = (T)num(in);
  long long L = 0, stride = 1;
  in >> L >> stride;
  std::vector<T> v((size_t)((L - 1) * stride + 1));
  for (T& a : v) a = (T)num(in);
  T theta = T(0), spos = T(0);
  int steps = 0;
  const int act = sipx::simplex_project_serial<T>(v.data(), L, stride, smin, smax, theta, spos, steps);
  std::printf("p %d %a %a %d", act, (double)theta, (double)spos, steps);
  for (const T a : v) std::printf(" %a", (double)a);
  std::printf("\n");
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    std::string what;
    in >> what;
    if (what == "k") {
      sipx::SegMap m{};
      in >> m.L >> m.LB >> m.sSa;
      std::printf("k %d\n", sipx::simplex_lane_bucket(m));
      continue;
    }
    std::string tf;
    in >> tf;
    if (what != "p" || (tf != "f" && tf != "d")) {
      std::printf("FAIL cannot read: %s\n", line.c_str());
      return 1;
    }
    if (tf == "f") project<float>(in);
    else project<double>(in);
  }
  std::printf("ok\n");
  return 0;
}
