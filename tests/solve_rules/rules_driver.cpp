// Runs the host rules of csrc/solve_rules.h on cases read from stdin, one answer line per case
// (tests/test_solve_rules_cpu.py compares the lines with oracle/parsdmm_oracle.py bit for bit).
// A case is a line of tokens: <command> <f|d> <arguments>; numbers travel as C99 hex floats ("nan", "inf" as words).
//   bb      6 sums, rho, gamma, adjust_rho, adjust_gamma                      -> rho gamma
//   argmax  n, row                                                            -> index
//   clamp   rho                                                               -> rho
//   sum     n, row                                                            -> sum
//   flags   switches, it                                                      -> flags
//   may     switches, it, pp, p, rho                                          -> 0 | 1
//   next    switches, it, pp, p, feasibility row, rho                         -> rho
//   stop    switches, maxit, pp, 3 tolerances (evol, feas, obj), nrows, set_feasibility, obj, evol_x, r_pri_total
//           -> per iteration up to the stop: stop adjust_rho adjust_gamma adjust_feas_rho ind_ref
//   switches = adjust_rho adjust_gamma adjust_feas_rho freq ind_ref
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "solve_rules.h"

namespace {

double num() {
  std::string t;
  std::cin >> t;
  return std::strtod(t.c_str(), nullptr);
}
int integer() {
  int v = 0;
  std::cin >> v;
  return v;
}
std::vector<double> row(int n) {
  std::vector<double> v((size_t)n);
  for (double& x : v) x = num();
  return v;
}
sipx::RuleSwitches switches() {
  sipx::RuleSwitches s;
  s.adjust_rho = integer() != 0;
  s.adjust_gamma = integer() != 0;
  s.adjust_feas_rho = integer() != 0;
  s.freq = integer();
  s.ind_ref = integer();
  return s;
}
void put(double v) {
  if (v != v) std::printf(" nan");
  else std::printf(" %a", v);
}

template <typename T>
void run(const std::string& cmd) {
  if (cmd == "bb") {
    const std::vector<double> a = row(8);
    const bool adjust_rho = integer() != 0, adjust_gamma = integer() != 0;
    T rho = (T)a[6], gamma = (T)a[7];
    sipx::bb_rule<T>((T)a[0], (T)a[1], (T)a[2], (T)a[3], (T)a[4], (T)a[5], adjust_rho, adjust_gamma, rho, gamma);
    put((double)rho);
    put((double)gamma);
  } else if (cmd == "argmax") {
    const int n = integer();
    const std::vector<double> v = row(n);
    std::printf(" %d", sipx::julia_argmax(v.data(), n));
  } else if (cmd == "clamp") {
    put((double)sipx::clamp_rho((T)num()));
  } else if (cmd == "sum") {
    const int n = integer();
    const std::vector<double> v = row(n);
    put(sipx::seq_sum<T>(v.data(), n));
  } else if (cmd == "flags") {
    const sipx::RuleSwitches s = switches();
    std::printf(" %d", sipx::yl_flags(s, integer()));
  } else if (cmd == "may") {
    const sipx::RuleSwitches s = switches();
    const int it = integer(), pp = integer(), p = integer();
    const std::vector<double> rho = row(p);
    std::printf(" %d", sipx::rho_may_change<T>(s, it, pp, rho.data(), p) ? 1 : 0);
  } else if (cmd == "next") {
    const sipx::RuleSwitches s = switches();
    const int it = integer(), pp = integer(), p = integer();
    const std::vector<double> feas = row(pp);
    std::vector<double> rho = row(p);
    sipx::next_rho<T>(s, it, pp, feas.data(), rho.data(), p);
    for (double v : rho) put(v);
  } else if (cmd == "stop") {
    sipx::RuleSwitches s = switches();
    const int maxit = integer(), pp = integer();
    sipx::Tolerances<T> tol;
    tol.evol_rel = (T)num();
    tol.feas = (T)num();
    tol.obj = (T)num();
    const int nrows = integer();
    const std::vector<double> feas = row(nrows * pp), obj = row(maxit), evol = row(maxit), rpri = row(maxit);
    const sipx::LogView log{feas.data(), obj.data(), evol.data(), rpri.data()};
    int counter = 2;
    for (int i = 1; i <= maxit; ++i) {
      if (sipx::feas_due(i)) counter += 1;                 // the y/l update of iteration i has filled a row
      const bool stop = sipx::stop_rule<T>(log, i, counter, pp, tol, s);
      std::printf(" %d %d %d %d %d", stop ? 1 : 0, (int)s.adjust_rho, (int)s.adjust_gamma, (int)s.adjust_feas_rho, s.ind_ref);
      if (stop) break;
    }
  } else {
    std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
    std::exit(2);
  }
  std::printf("\n");
}

}  // namespace

int main() {
  std::string cmd, type;
  while (std::cin >> cmd >> type) {
    if (type == "f") run<float>(cmd);
    else run<double>(cmd);
  }
  return 0;
}
