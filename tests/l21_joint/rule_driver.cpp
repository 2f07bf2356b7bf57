// csrc/l21_joint.h on the CPU: the launch plan of the z-march and the rule of the joint l2,1 ball, one request per input line
//     plan <L> <n3> <bytes per entry>                           -> "plan <nchunk> <zc>"
//     <f|d> <n1> <n2> <n3> <theta> <vy_0> ... <vy_{N-1}> <vx_0> ... <vx_{N-1}>
//                                                               -> "g <g_0> ... <g_{L-1}>" and "v <vy ...> <vx ...>" after the scaling
// the two padded blocks of D_y and D_x, N = n1 n2 n3 entries each; numbers in hexadecimal floating point in the precision asked for.
// hipcc compiles it (the headers need the HIP headers); the program makes no HIP call.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "l21_joint.h"

template <typename T>
static int rule(std::istringstream& in) {
  long long n1 = 0, n2 = 0, n3 = 0;
  std::string w;
  if (!(in >> n1 >> n2 >> n3 >> w) || n1 < 1 || n2 < 1 || n3 < 1) return 1;
  const T theta = (T)std::strtod(w.c_str(), nullptr);
  const long long L = n1 * n2, N = L * n3;
  std::vector<T> v((size_t)(2 * N)), g((size_t)L);
  for (long long t = 0; t < 2 * N; ++t) {
    if (!(in >> w)) return 1;
    v[(size_t)t] = (T)std::strtod(w.c_str(), nullptr);
  }
  const sipx::L21JointPlan plan = sipx::l21_joint_plan(L, n3, (int)sizeof(T));
  sipx::l21_joint_norms_serial<T>(plan, n1, n2, n3, v.data(), v.data() + N, g.data());
  sipx::l21_joint_scale_serial<T>(n1, n2, n3, v.data(), v.data() + N, g.data(), theta);
  std::printf("g");
  for (long long p = 0; p < L; ++p) std::printf(" %a", (double)g[(size_t)p]);
  std::printf("\nv");
  for (long long t = 0; t < 2 * N; ++t) std::printf(" %a", (double)v[(size_t)t]);
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
    if (tf == "plan") {
      long long L = 0, n3 = 0;
      int eb = 0;
      in >> L >> n3 >> eb;
      const sipx::L21JointPlan p = sipx::l21_joint_plan(L, n3, eb);
      std::printf("plan %d %d\n", p.nchunk, p.zc);
      continue;
    }
    const int bad = tf == "f" ? rule<float>(in) : (tf == "d" ? rule<double>(in) : 1);
    if (bad) {
      std::printf("FAIL cannot read: %s\n", line.substr(0, 200).c_str());
      return 1;
    }
  }
  std::printf("constants %d %d\n", (int)L21J_FILL_THREADS, (int)L21J_MIN_CHUNK);
  std::printf("ok\n");
  return 0;
}
