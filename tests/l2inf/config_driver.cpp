// Host-side driver of csrc/set_config.h for the SIPX_PROJ_L2INF kinds (tests/test_l2inf_cpu.py): what their descriptors mean on a grid --
// route, rows, groups, refusals -- is host arithmetic, so it runs here without a GPU.  No HIP call is made.
//
// stdin, one request per line, fields as key=value in any order:
//   set tf=<f|d> ndim=<2|3> n=<n0,n1,n2> [single=<0|1>] [op= proj= pmin= pmax= mode= dir= comp= tr= blocks=] [lb=<count>] [ub=<count>]
//       [ubat=<index>:<value>]   one entry of ub other than 1 (inf, nan and negative numbers as strtod reads them)
//       [reserved=] [rows=<M>]   op=5: a custom operator of M rows with one stored entry (row 0 of column 0)
//       [ata=<d_i>]              ata_R of N x d_i ones with offsets 0, 1, ... (absent: NULL, the matrix-free term)
//       [old=1]                  the descriptor is filled through a struct that ends where sipx_set_desc ended before `blocks` was
//                                appended (the bytes behind it stay zero, as a zero-initialised descriptor of an older caller has them)
//   -> "error <message>" or "ok ext_kind= prox= custom= mfree= Mtrue= Mpad= spec.nblk= spec.bstride= spec.N= spec.mode= data_len= needs_ext= ncvx= two_pass="
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "set_config.h"

using namespace sipx;
typedef std::map<std::string, std::string> Fields;

// sipx_set_desc as it was before `blocks`: the same fields in the same order, up to pad_
struct old_set_desc {
  int32_t op, proj;
  double pmin, pmax;
  const void *lb, *ub;
  int32_t ncvx, reserved, mode, dir;
  const void* basis;
  int64_t basis_rows;
  int32_t basis_cols, basis_orth, component;
  const int64_t *csc_colptr, *csc_rowval;
  const void* csc_nzval;
  int64_t csc_rows;
  int32_t transform, pad_;
};
static_assert(sizeof(old_set_desc) + 8 == sizeof(sipx_set_desc), "blocks is appended behind the older fields");
static_assert(offsetof(sipx_set_desc, blocks) == sizeof(old_set_desc), "blocks is appended behind the older fields");

static std::string get(const Fields& f, const char* key, const char* dflt) {
  auto it = f.find(key);
  return it == f.end() ? std::string(dflt) : it->second;
}
static long long integer(const std::string& s) { return std::strtoll(s.c_str(), nullptr, 10); }

template <typename T>
static void do_set(const Fields& f) {
  int64_t n[3] = {1, 1, 1};
  double h[3] = {1, 1, 1};
  {
    std::istringstream in(get(f, "n", "1,1,1"));
    std::string item;
    for (int a = 0; a < 3 && std::getline(in, item, ','); ++a) n[a] = integer(item);
  }
  ConfigCtx c = grid_ctx<T>((int)integer(get(f, "ndim", "2")), n, h);
  c.single_process = integer(get(f, "single", "1")) != 0;
  sipx_set_desc d;
  std::memset(&d, 0, sizeof d);
  std::vector<T> lb, ub, nzval(1, T(1)), ata;
  std::vector<int64_t> colptr, rowval(1, 0), ata_off;
  if (f.count("lb")) lb.assign((size_t)integer(f.at("lb")), T(1));
  if (f.count("ub")) ub.assign((size_t)integer(f.at("ub")), T(1));
  if (f.count("ubat")) {
    const std::string a = f.at("ubat");
    ub.at((size_t)integer(a.substr(0, a.find(':')))) = (T)std::strtod(a.substr(a.find(':') + 1).c_str(), nullptr);
  }
  const bool old = integer(get(f, "old", "0")) != 0;
  {
    old_set_desc o;
    std::memset(&o, 0, sizeof o);
    o.op = (int)integer(get(f, "op", "0"));
    o.proj = (int)integer(get(f, "proj", "0"));
    o.pmin = std::strtod(get(f, "pmin", "0").c_str(), nullptr);
    o.pmax = std::strtod(get(f, "pmax", "0").c_str(), nullptr);
    o.mode = (int)integer(get(f, "mode", "0"));
    o.dir = (int)integer(get(f, "dir", "0"));
    o.component = (int)integer(get(f, "comp", "0"));
    o.transform = (int)integer(get(f, "tr", "0"));
    o.reserved = (int)integer(get(f, "reserved", "0"));
    if (f.count("lb")) o.lb = lb.data();
    if (f.count("ub")) o.ub = ub.data();
    if (o.op == SIPX_OP_CSC) {
      colptr.assign((size_t)c.G.N + 1, 1);
      colptr[0] = 0;
      o.csc_rows = integer(get(f, "rows", "1"));
      o.csc_colptr = colptr.data(); o.csc_rowval = rowval.data(); o.csc_nzval = nzval.data();
    }
    std::memcpy(&d, &o, sizeof o);
  }
  if (!old) d.blocks = (int)integer(get(f, "blocks", "0"));
  int d_i = 0;
  if (f.count("ata")) {
    d_i = (int)integer(f.at("ata"));
    for (int k = 0; k < d_i; ++k) ata_off.push_back(k);
    ata.assign((size_t)c.G.N * (size_t)d_i + 1, T(1));
  }
  const SetConfig<T> s = configure_set<T>(c, &d, f.count("ata") ? ata.data() : nullptr, ata_off.data(), d_i);
  std::printf("ok ext_kind=%d prox=%d custom=%d mfree=%d Mtrue=%lld Mpad=%lld spec.nblk=%d spec.bstride=%lld spec.N=%lld spec.mode=%d data_len=%lld "
              "needs_ext=%d ncvx=%d two_pass=%d\n",
              s.ext_kind, s.prox, (int)s.custom, (int)s.mfree, s.Mtrue, s.Mpad, s.spec.nblk, s.spec.bstride, (long long)s.spec.G.N, s.spec.mode,
              data_len(c, s), (int)s.needs_ext_scratch, s.ncvx, (int)s.two_pass);
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd, tok;
    if (!(in >> cmd)) continue;
    try {
      if (cmd != "set") {
        std::printf("error unknown request %s\n", cmd.c_str());
        continue;
      }
      Fields f;
      while (in >> tok) f[tok.substr(0, tok.find('='))] = tok.substr(tok.find('=') + 1);
      if (get(f, "tf", "f") == "f") do_set<float>(f); else do_set<double>(f);
    } catch (const std::exception& e) {
      std::printf("error %s\n", e.what());
    }
  }
  return 0;
}
