// The host rules of a PARSDMM solve, each written once: what the reference decides on the CPU between the kernels of an
// iteration -- the stop rule (src/stop_PARSDMM.jl), the Barzilai-Borwein scalars (src/adapt_rho_gamma.jl), the schedule and
// the rho rules of the main loop (src/PARSDMM.jl:163-227).  Templated on the working type T where the reference computes
// in TF; logs and rho travel as double and hold T values.  engine.cpp calls these and contains none of the arithmetic.
// (tests/test_solve_rules_cpu.py compares every function with a numpy restatement of the reference, bit for bit, on the CPU.)
// No HIP header: this file compiles with a plain host compiler.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>

namespace sipx {

// Julia maximum(): NaN-propagating
template <typename It>
double julia_maximum(It b, It e) {
  double m = -INFINITY;
  for (; b != e; ++b) {
    if (std::isnan(*b)) return NAN;
    m = std::max(m, (double)*b);
  }
  return m;
}

// Julia findmax(): the first NaN wins, otherwise the first maximum
inline int julia_argmax(const double* row, int n) {
  int arg = 0;
  for (int k = 0; k < n; ++k) {
    if (std::isnan(row[k])) return k;
    if (row[k] > row[arg]) arg = k;
  }
  return arg;
}

// sum() of a short log row holding T values: sequential T additions (r_pri_total, r_dual_total; PARSDMM.jl:134,138)
template <typename T>
double seq_sum(const double* row, int n) {
  if (n < 1) return 0.0;
  T acc = (T)row[0];
  for (int k = 1; k < n; ++k) acc = acc + (T)row[k];
  return (double)acc;
}

// PARSDMM.jl:226
template <typename T>
T clamp_rho(T rho) {
  return std::max(std::min(rho, T(1e4)), T(1e-2));
}

// Barzilai-Borwein scalar rule, reference src/adapt_rho_gamma.jl:55-126, all arithmetic in T.
template <typename T>
void bb_rule(T d_dHh_dlh, T n_d_H_hat, T n_d_l_hat, T n_d_l, T n_d_G_hat, T d_dGh_dl, bool adjust_rho,
             bool adjust_gamma, T& rho, T& gamma) {
  const T safeguard = sizeof(T) == 8 ? T(1e-10) : T(1e-6);   // :31-35
  const T eps_correlation = T(0.3);                          // :37
  bool alpha_reliable = false, beta_reliable = false;
  T alpha_correlation = 0, beta_correlation = 0;
  if ((n_d_H_hat * n_d_l_hat) > safeguard && (n_d_H_hat * n_d_H_hat) > safeguard && d_dHh_dlh > safeguard) {
    alpha_reliable = true;
    alpha_correlation = d_dHh_dlh / (n_d_H_hat * n_d_l_hat);
  }
  if ((n_d_G_hat * n_d_l) > safeguard && (n_d_G_hat * n_d_G_hat) > safeguard && d_dGh_dl > safeguard) {
    beta_reliable = true;
    beta_correlation = d_dGh_dl / (n_d_G_hat * n_d_l);
  }
  bool alpha_comp = false, beta_comp = false;
  T alpha_hat = 0, beta_hat = 0;
  if (alpha_reliable && alpha_correlation > eps_correlation) {
    alpha_comp = true;
    const T mg = d_dHh_dlh / (n_d_H_hat * n_d_H_hat);
    const T sd = (n_d_l_hat * n_d_l_hat) / d_dHh_dlh;
    alpha_hat = (T(2) * mg) > sd ? mg : sd - mg / T(2);
  }
  if (beta_reliable && beta_correlation > eps_correlation) {
    beta_comp = true;
    const T mg = d_dGh_dl / (n_d_G_hat * n_d_G_hat);
    const T sd = (n_d_l * n_d_l) / d_dGh_dl;
    beta_hat = (T(2) * mg) > sd ? mg : sd - mg / T(2);
  }
  if (adjust_rho) {
    if (alpha_comp && beta_comp) rho = std::sqrt(alpha_hat * beta_hat);
    else if (alpha_comp) rho = alpha_hat;
    else if (beta_comp) rho = beta_hat;
  }
  if (adjust_gamma) {
    if (alpha_comp && beta_comp) gamma = T(1) + ((T(2) * std::sqrt(alpha_hat * beta_hat)) / (alpha_hat + beta_hat));
    else if (alpha_comp) gamma = T(1.9);
    else if (beta_comp) gamma = T(1.1);
    else gamma = T(1.5);
  }
}

// ---- the schedule of the main loop ------------------------------------------------------------------------------------------
// What the options switch on, as the stop rule leaves it: it switches the three adjust_* off for good once the primal
// residual grows (ind_ref: the iteration at which it did; maxit until then).
struct RuleSwitches {
  bool adjust_rho = true, adjust_gamma = true, adjust_feas_rho = true;
  int freq = 2;                      // rho_update_frequency
  int ind_ref = 0;
};

// the bits of a y/l update's flags, as include/sipx.h numbers them (SIPX_YL_FEAS, SIPX_YL_BB, SIPX_YL_FIRST)
enum { YL_FEAS = 1, YL_BB = 2, YL_FIRST = 4 };

// iteration `it` estimates the feasibility of every set and opens a new row of log.set_feasibility (update_y_l.jl:90-105)
inline bool feas_due(int it) { return it % 10 == 0; }
// ... runs the Barzilai-Borwein rule (PARSDMM.jl:182)
inline bool bb_due(const RuleSwitches& s, int it) { return (s.adjust_rho || s.adjust_gamma) && it % s.freq == 0; }
// ... doubles the rho of the least feasible set (:213-223)
inline bool feas_rho_due(const RuleSwitches& s, int it, int pp) { return s.adjust_feas_rho && feas_due(it) && it > 10 && pp > 0; }

inline int yl_flags(const RuleSwitches& s, int it) {
  return (feas_due(it) ? YL_FEAS : 0) | (it == 1 ? YL_FIRST : 0) | (bb_due(s, it) ? YL_BB : 0);
}

// The rho of the coming iteration from the rho the Barzilai-Borwein rule left (in place): the feasibility doubling on the
// latest row of log.set_feasibility, then the clamp, which runs every iteration (PARSDMM.jl:213-226).
template <typename T>
void next_rho(const RuleSwitches& s, int it, int pp, const double* feas_row, double* rho, int p) {
  if (feas_rho_due(s, it, pp)) {
    const int arg = julia_argmax(feas_row, pp);
    rho[arg] = (double)(T(2.0) * (T)rho[arg]);
  }
  for (int k = 0; k < p; ++k) rho[k] = (double)clamp_rho((T)rho[k]);
}

// Can the rules at the end of iteration `it` change rho?  Asked BEFORE the stop rule of that iteration has run, which can
// only switch rules off: "may" where nothing changes in the end is allowed, "cannot" where something does is not.
// (a rho_ini outside the clamp changes at once)
template <typename T>
bool rho_may_change(const RuleSwitches& s, int it, int pp, const double* rho, int p) {
  for (int k = 0; k < p; ++k)
    if ((T)rho[k] != clamp_rho((T)rho[k])) return true;
  return bb_due(s, it) || feas_rho_due(s, it, pp);
}

// ---- src/stop_PARSDMM.jl:23-52 -----------------------------------------------------------------------------------------------
struct LogView {                     // the arrays of the log the rule reads; entry i - 1 is iteration i
  const double* set_feasibility;     // rows of pp
  const double* obj;
  const double* evol_x;
  const double* r_pri_total;
};
template <typename T>
struct Tolerances {                  // convert_options!: the options' tolerances in T
  T evol_rel = 0, feas = 0, obj = 0;
};

// true: stop after iteration i.  counter: the row of set_feasibility the next estimate will fill, 1-based (the latest one is
// counter - 1).  Switches the adjust_* off and sets ind_ref when the primal residual exceeds its last fifty values.
template <typename T>
bool stop_rule(const LogView& log, int i, int counter, int pp, const Tolerances<T>& tol, RuleSwitches& s) {
  bool stop = false;
  if (i > 6 && pp > 0) {                                            // :23-27 feasible and the objective has settled
    const double* row = log.set_feasibility + (size_t)(counter - 2) * pp;
    if (julia_maximum(row, row + pp) < (double)tol.feas) {
      double mx = -INFINITY;
      bool nan = false;
      for (int k = i - 6; k < i; ++k) {
        const T a = (T)log.obj[k], b = (T)log.obj[k - 1];
        const T v = std::fabs((a - b) / b);
        if (std::isnan(v)) nan = true;
        mx = std::max(mx, (double)v);
      }
      if (!nan && mx < (double)tol.obj) stop = true;
    }
  }
  if (i > 5 && julia_maximum(log.evol_x + (i - 6), log.evol_x + i) < (double)tol.evol_rel) stop = true;      // :29-32
  if (i > 20 && s.adjust_rho) {                                     // :35-46
    const int lo = std::max(i - 50, 1);
    if (log.r_pri_total[i - 1] > julia_maximum(log.r_pri_total + (lo - 1), log.r_pri_total + (i - 1))) {
      s.adjust_rho = s.adjust_feas_rho = s.adjust_gamma = false;
      s.ind_ref = i;
    }
  }
  if (!s.adjust_rho && i > s.ind_ref + 25) {                        // :49-52
    const int lo = std::max(s.ind_ref, std::max(i - 50, 1));
    if (log.r_pri_total[i - 1] > julia_maximum(log.r_pri_total + (lo - 1), log.r_pri_total + (i - 1))) stop = true;
  }
  return stop;
}

}  // namespace sipx
