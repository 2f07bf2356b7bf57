// csrc/tnv.h on the CPU: the rule of total nuclear variation, one request per input line
//     <f|d> <n1> <n2> <n3> <in file> <out file> <theta_0> [<theta_1> ...]
// in file: the two padded blocks of D_y and D_x, N = n1 n2 n3 entries each, raw numbers of the precision asked for.  out file, raw too:
// s = [sigma1; sigma2] (2 L), rot = [cs; sn] (2 L), then for every theta the 2 N entries of the blocks after the scaling (each from the
// input, not from one another).  theta in hexadecimal floating point.  The answer line is "done <L> <thetas>".
// The chunks are those of l21_joint_plan (tests/l21_joint/rule_driver.cpp answers for the plan itself).
// hipcc compiles it (the headers need the HIP headers); the program makes no HIP call.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "tnv.h"

template <typename T>
static int rule(std::istringstream& in) {
  long long n1 = 0, n2 = 0, n3 = 0;
  std::string fin, fout, w;
  if (!(in >> n1 >> n2 >> n3 >> fin >> fout) || n1 < 1 || n2 < 1 || n3 < 1) return 1;
  const long long L = n1 * n2, N = L * n3;
  std::vector<T> v((size_t)(2 * N)), s((size_t)(2 * L)), rot((size_t)(2 * L));
  FILE* f = std::fopen(fin.c_str(), "rb");
  if (!f) return 1;
  const size_t got = std::fread(v.data(), sizeof(T), v.size(), f);
  std::fclose(f);
  if (got != v.size()) return 1;
  const sipx::L21JointPlan plan = sipx::l21_joint_plan(L, n3, (int)sizeof(T));
  sipx::tnv_decompose_serial<T>(plan, n1, n2, n3, v.data(), v.data() + N, s.data(), rot.data());
  f = std::fopen(fout.c_str(), "wb");
  if (!f) return 1;
  bool ok = std::fwrite(s.data(), sizeof(T), s.size(), f) == s.size() && std::fwrite(rot.data(), sizeof(T), rot.size(), f) == rot.size();
  int thetas = 0;
  while (ok && (in >> w)) {
    const T theta = (T)std::strtod(w.c_str(), nullptr);
    std::vector<T> y(v);
    sipx::tnv_apply_serial<T>(n1, n2, n3, y.data(), y.data() + N, s.data(), rot.data(), theta);
    ok = std::fwrite(y.data(), sizeof(T), y.size(), f) == y.size();
    ++thetas;
  }
  std::fclose(f);
  if (!ok) return 1;
  std::printf("done %lld %d\n", L, thetas);
  return 0;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    std::string tf;
    in >> tf;
    const int bad = tf == "f" ? rule<float>(in) : (tf == "d" ? rule<double>(in) : 1);
    if (bad) {
      std::printf("FAIL cannot serve: %s\n", line.substr(0, 200).c_str());
      return 1;
    }
  }
  std::printf("words %d %d\n", sipx::tnv_words<float>(), sipx::tnv_words<double>());
  std::printf("ok\n");
  return 0;
}
