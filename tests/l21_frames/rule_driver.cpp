// csrc/l21_seg.h on the CPU: the launch plan of the per-frame threshold kernel and the rule of one frame, one request per input line
//     plan <L> <frames> <bytes per entry>                  -> "plan <lds> <grid> <lds_bytes> <path>"
//     <f|d> <tau> <vec 0|1> <L> <g_0> ... <g_{L-1}>        -> "frame <decision> <(T)asum> <theta> <Michelot passes>"
// numbers in hexadecimal floating point, g and tau in the precision asked for; the sums run serially in index order
// (l21_seg_frame).  hipcc compiles it (the headers need the HIP headers); the program makes no HIP call.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "l21_seg.h"

template <typename T>
static int frame(std::istringstream& in) {
  std::string w;
  int vec = 0;
  long long L = 0;
  if (!(in >> w >> vec >> L) || L < 1) return 1;
  const T tau = (T)std::strtod(w.c_str(), nullptr);
  std::vector<T> g((size_t)L);
  for (long long t = 0; t < L; ++t) {
    if (!(in >> w)) return 1;
    g[(size_t)t] = (T)std::strtod(w.c_str(), nullptr);
  }
  T asum, theta;
  int passes;
  const int act = sipx::l21_seg_frame<T>(g.data(), L, tau, vec != 0, asum, theta, passes);
  std::printf("frame %d %a %a %d\n", act, (double)asum, (double)theta, passes);
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
      long long L = 0, nf = 0;
      int eb = 0;
      in >> L >> nf >> eb;
      const sipx::L21SegPlan p = sipx::l21_seg_plan(L, nf, eb);
      std::printf("plan %d %u %u %d\n", p.lds, p.grid, p.lds_bytes, p.path());
      continue;
    }
    const int bad = tf == "f" ? frame<float>(in) : (tf == "d" ? frame<double>(in) : 1);
    if (bad) {
      std::printf("FAIL cannot read: %s\n", line.substr(0, 200).c_str());
      return 1;
    }
  }
  std::printf("budget %d %lld\n", sipx::SEGN_LDS_BYTES, (long long)sipx::SEGN_MAX_GRID);
  std::printf("ok\n");
  return 0;
}
