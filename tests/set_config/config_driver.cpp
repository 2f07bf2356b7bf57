// Host-side driver of csrc/set_config.h (tests/test_set_config_cpu.py): what a set descriptor means on a grid -- route, rows,
// vectors, refusals -- is host arithmetic, so it runs here without a GPU.  No HIP call is made.
//
// stdin, one request per line, fields as key=value in any order (numbers: decimal or hex floats; lists: comma-separated):
//   set tf=<f|d> ndim=<2|3> n=<n0,n1,n2> [h=<h0,h1,h2>] [single=<0|1>] [op= proj= pmin= pmax= mode= dir= comp= tr= ncvx=]
//       [lb=<list> | lb=fill:<count>:<value>] [ub=...]     the descriptor's vectors (absent: NULL)
//       [basis=<rows>x<cols>] [orth=<0|1>]                  a basis of ones
//       [ata=<d_i>:<offsets>]                               ata_R of N x |d_i| ones with these offsets (absent: NULL)
//       [csc=<rows>/<colptr>/<rowval> | csc=missing]        the arrays of a custom operator, nzval of ones
//       [dump=1]                                            also print host_lb / host_ub as hex floats
//       -> "error <message>" or "ok key=value ..." (see print_config)
//   mf <N> <M> <nnz>            -> check_mf_index_range: "ok" or "error <message>"
//   dwt <ndim> <n0> <n1> <n2>   -> dwt_check_grid: "ok levels=<L>" or "error <message>"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "set_config.h"

using namespace sipx;
typedef std::map<std::string, std::string> Fields;

static std::vector<std::string> split(const std::string& s, char sep) {
  std::vector<std::string> out;
  std::string item;
  std::istringstream in(s);
  while (std::getline(in, item, sep)) out.push_back(item);
  if (!s.empty() && s.back() == sep) out.push_back("");
  return out;
}
static double num(const std::string& s) { return std::strtod(s.c_str(), nullptr); }
static long long integer(const std::string& s) { return std::strtoll(s.c_str(), nullptr, 10); }
static std::string get(const Fields& f, const char* key, const char* dflt) {
  auto it = f.find(key);
  return it == f.end() ? std::string(dflt) : it->second;
}
template <typename T>
static std::vector<T> vector_of(const std::string& s) {
  std::vector<T> v;
  const std::vector<std::string> p = split(s, s.rfind("fill:", 0) == 0 ? ':' : ',');
  if (s.rfind("fill:", 0) == 0) v.assign((size_t)integer(p[1]), (T)num(p[2]));
  else for (const std::string& t : p) v.push_back((T)num(t));
  return v;
}
template <typename V>
static std::string join(const V* v, size_t n) {
  std::string s;
  for (size_t k = 0; k < n; ++k) s += (k ? "," : "") + std::to_string(v[k]);
  return s;
}
template <typename T>
static std::string hex_join(const std::vector<T>& v) {
  std::string s;
  char buf[64];
  for (size_t k = 0; k < v.size(); ++k) {
    std::snprintf(buf, sizeof buf, "%a", (double)v[k]);
    s += (k ? "," : "") + std::string(buf);
  }
  return s;
}

template <typename T>
static void print_config(const ConfigCtx& c, const SetConfig<T>& s, bool dump) {
  const bool segs = s.ext_kind && s.spec.mode != SIPX_MODE_WHOLE;
  std::printf("ok ndim=%d prox=%d ext_kind=%d two_pass=%d nblk=%d dir=%s Mtrue=%lld Mpad=%lld blk_rows=%s seg_radii=%d data_len=%lld "
              "needs_ext=%d needs_idx=%d custom=%d mfree=%d ident=%d comp=%d bmode=%d bdir=%d plo=%a phi=%a ih=%a,%a,%a "
              "spec.dims=%s spec.mode=%d spec.dir=%d spec.inner=%d spec.nblk=%d spec.bdir=%s nseg=%lld nlb=%zu nub=%zu nbasis=%zu nata=%zu "
              "ata_off=%s",
              c.ndim, s.prox, s.ext_kind, (int)s.two_pass, s.nblk, join(s.dir, 3).c_str(), s.Mtrue, s.Mpad, join(s.blk_rows, 3).c_str(),
              (int)s.seg_radii, data_len(c, s), (int)s.needs_ext_scratch, (int)s.needs_index_scratch, (int)s.custom, (int)s.mfree,
              (int)s.ident, s.comp, s.bmode, s.bdir, (double)s.plo, (double)s.phi, (double)s.ih[0], (double)s.ih[1], (double)s.ih[2],
              join(s.spec.dims, 3).c_str(), s.spec.mode, s.spec.dir, s.spec.inner, s.spec.nblk, join(s.spec.bdir, 3).c_str(),
              segs ? seg_count(s.spec) : 0ll, s.host_lb.size(), s.host_ub.size(), s.host_basis.size(), s.host_ata.size(),
              join(s.ata_off.data(), s.ata_off.size()).c_str());
  if (dump) std::printf(" host_lb=%s host_ub=%s", hex_join(s.host_lb).c_str(), hex_join(s.host_ub).c_str());
  std::printf("\n");
}

template <typename T>
static void do_set(const Fields& f) {
  int64_t n[3] = {1, 1, 1};
  double h[3] = {1, 1, 1};
  const std::vector<std::string> ns = split(get(f, "n", "1,1,1"), ','), hs = split(get(f, "h", "1,1,1"), ',');
  for (size_t a = 0; a < 3 && a < ns.size(); ++a) n[a] = integer(ns[a]);
  for (size_t a = 0; a < 3 && a < hs.size(); ++a) h[a] = num(hs[a]);
  ConfigCtx c = grid_ctx<T>((int)integer(get(f, "ndim", "2")), n, h);
  c.single_process = integer(get(f, "single", "1")) != 0;
  sipx_set_desc d{};
  d.op = (int)integer(get(f, "op", "0"));
  d.proj = (int)integer(get(f, "proj", "0"));
  d.pmin = num(get(f, "pmin", "0"));
  d.pmax = num(get(f, "pmax", "0"));
  d.mode = (int)integer(get(f, "mode", "0"));
  d.dir = (int)integer(get(f, "dir", "0"));
  d.component = (int)integer(get(f, "comp", "0"));
  d.transform = (int)integer(get(f, "tr", "0"));
  d.ncvx = (int)integer(get(f, "ncvx", "0"));
  std::vector<T> lb, ub, basis, ata, nzval;
  std::vector<int64_t> ata_off, colptr, rowval;
  if (f.count("lb")) { lb = vector_of<T>(f.at("lb")); d.lb = lb.data(); }
  if (f.count("ub")) { ub = vector_of<T>(f.at("ub")); d.ub = ub.data(); }
  if (f.count("basis")) {
    const std::vector<std::string> p = split(f.at("basis"), 'x');
    d.basis_rows = integer(p[0]);
    d.basis_cols = (int)integer(p[1]);
    d.basis_orth = (int)integer(get(f, "orth", "0"));
    basis.assign((size_t)std::max<long long>(1, d.basis_rows * d.basis_cols), T(1));
    d.basis = d.basis_rows || d.basis_cols ? basis.data() : nullptr;
  }
  int d_i = 0;
  if (f.count("ata")) {
    const std::vector<std::string> p = split(f.at("ata"), ':');
    d_i = (int)integer(p[0]);
    for (const std::string& t : split(p.size() > 1 ? p[1] : "", ',')) ata_off.push_back(integer(t));
    ata.assign((size_t)c.G.N * (size_t)std::abs(d_i) + 1, T(1));
  }
  if (f.count("csc") && f.at("csc") != "missing") {
    const std::vector<std::string> p = split(f.at("csc"), '/');
    d.csc_rows = integer(p[0]);
    for (const std::string& t : split(p[1], ',')) colptr.push_back(integer(t));
    for (const std::string& t : split(p[2], ',')) if (!t.empty()) rowval.push_back(integer(t));
    nzval.assign(rowval.size() + 1, T(1));
    d.csc_colptr = colptr.data(); d.csc_rowval = rowval.data(); d.csc_nzval = nzval.data();
  }
  const SetConfig<T> s = configure_set<T>(c, &d, f.count("ata") ? ata.data() : nullptr, ata_off.data(), d_i);
  print_config(c, s, integer(get(f, "dump", "0")) != 0);
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd, tok;
    if (!(in >> cmd)) continue;
    try {
      if (cmd == "set") {
        Fields f;
        while (in >> tok) f[tok.substr(0, tok.find('='))] = tok.substr(tok.find('=') + 1);
        if (get(f, "tf", "f") == "f") do_set<float>(f); else do_set<double>(f);
      } else if (cmd == "mf") {
        long long N, M, nnz;
        in >> N >> M >> nnz;
        check_mf_index_range(N, M, nnz);
        std::printf("ok\n");
      } else if (cmd == "dwt") {
        int ndim;
        long long n[3];
        in >> ndim >> n[0] >> n[1] >> n[2];
        dwt_check_grid(ndim, n);
        std::printf("ok levels=%d\n", dwt_levels(ndim, n));
      } else {
        std::printf("error unknown request %s\n", cmd.c_str());
      }
    } catch (const std::exception& e) {
      std::printf("error %s\n", e.what());
    }
  }
  return 0;
}
