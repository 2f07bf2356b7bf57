// What a sipx_set_desc means on a grid, decided once and without a device: the kernel route a set takes, its rows, the vectors
// it carries, and which combinations are refused and with what words.  Host arithmetic only -- no HIP runtime call is made here,
// so tests/set_config/config_driver.cpp runs every rule on the CPU (tests/test_set_config_cpu.py).  The engine derives a ConfigCtx
// from its live state, calls configure_set at sipx_add_set and keeps the SetConfig as the base of its SetState; the stand-alone
// calls (sipx_project, sipx_segment_norms, sipx_l21_norms, sipx_apply_op) configure a throw-away SetConfig the same way.
#pragma once
#include <algorithm>
#include <cmath>

#include "dwt.h"
#include "ext_family.h"      // (sipx.h, sipx_common.h, ext_proj.h; make_segmap / seg_count)
#include "l21_groups.h"      // (the refusals and the descriptor check of the l2,1 ball over fibers / slices)
#include "l21_weighted.h"    // (the host checks of the weighted l2,1 sets)
#include "l1_weighted.h"     // (the refusals and the host checks of the weighted l1 ball)
#include "seg_simplex.h"     // (the refusals and the check of the bounds of the simplex sets)
#include "card_groups.h"     // (the refusals and the check of k of group cardinality)
#include "l20.h"             // (the refusals and the checks of k of the l2,0 sets on TV / TV_xy)
#include "l21_stacked.h"     // (the refusals and the shape check of the l2,1 ball across the blocks of a stacked operator)
#include "l2inf.h"           // (the refusals and the checks of the bounds of the l2,inf sets)

namespace sipx {

// what the rules read from a context
struct ConfigCtx {
  int ndim = 2;                      // 2 also for a 3-D grid with n3 = 1 (get_TD_operator.jl:30)
  Grid G;
  double ih[3] = {0, 0, 0};          // +-1/h as the context's type rounds it (get_discrete_Grad.jl:22-23,58-60)
  bool single_process = true;        // no communicator, no slab decomposition, no set ownership
};

// the grid of a context of type T
template <typename T>
ConfigCtx grid_ctx(int ndim, const int64_t* n, const double* h) {
  if (ndim != 2 && ndim != 3) throw std::runtime_error("ndim must be 2 or 3");
  ConfigCtx c;
  c.ndim = ndim;
  Grid& G = c.G;
  for (int a = 0; a < 3; ++a) {
    G.n[a] = a < ndim ? n[a] : 1;
    if (G.n[a] < 1) throw std::runtime_error("grid size must be positive");
    c.ih[a] = a < ndim ? (double)(T(1) / T(h[a])) : 0.0;
  }
  if (ndim == 3 && G.n[2] == 1) c.ndim = 2;
  G.N = G.n[0] * G.n[1] * G.n[2];
  G.st[0] = 1;
  G.st[1] = G.n[0];
  G.st[2] = G.n[0] * G.n[1];
  if (G.N >= (1ll << 31)) throw std::runtime_error("grids of 2^31 points or more are not supported");
  G.set_fast_div();
  return c;
}

// everything of a set that its descriptor fixes (sipx_add_set); the solve-owned remainder is the engine's SetState
template <typename T>
struct SetConfig {
  int op = 0, prox = 0, nblk = 0, ncvx = 0;
  int nblk_or1() const { return nblk > 0 ? nblk : 1; }
  bool rank_like() const { return ext_kind == EXT_RANK || ext_kind == EXT_NUCLEAR; }
  // a slice-wise rank / nuclear set on the last grid dimension of the identity: every rank can project the slices of its own z-slab
  bool sliced_on_last_dim(int ndim) const { return rank_like() && spec.mode == SIPX_MODE_SLICE && spec.dir == ndim - 1 && ident; }
  // caller-supplied sparse operator (SIPX_OP_CSC): CSC for the adjoint, a CSR copy for the forward product; s = A x is
  // materialised in sbuf and every set kernel then runs in its identity shape on a 1-D grid of M entries
  bool custom = false;
  std::vector<long long> h_colptr, h_rowval;
  std::vector<T> h_nzval;
  Grid gm;                           // the 1-D "grid" of the M rows
  // Matrix-free term of Q (ata_R = NULL at sipx_add_set): the set hands over no bands of A'A; every product with Q adds
  // rho_i A_i'(A_i p) through the kernels of kernels_sparse.hip, which also serve the set's own s = A x and A'w (one operator,
  // one arithmetic).
  bool mfree = false;
  int comp = 0;                      // Minkowski component: 0 none, 1 = [A 0], 2 = [0 A], 3 = [A A]
  int dir[3] = {0, 0, 0};
  T ih[3] = {0, 0, 0};
  long long Mtrue = 0, Mpad = 0;
  long long blk_rows[3] = {0, 0, 0};
  T plo = 0, phi = 0;
  bool ident = true, two_pass = false;
  int bmode = SIPX_MODE_WHOLE, bdir = 0;   // SIPX_PROJ_BOUNDS_VEC: one bound per row (WHOLE) or per coordinate along bdir (FIBER)
  int ext_kind = 0;                  // projector acting on a materialised vector (ext_proj.h)
  bool seg_radii = false;            // EXT_L1_SEG / L2_SEG / ANNULUS_SEG built with one radius per segment (host_lb / host_ub, then the projector's)
  bool weighted = false;             // EXT_L21 (whole array) / EXT_L21_JOINT / EXT_L21_GROUPS built with one weight per group in lb (host_lb, then the projector's);
                                     // EXT_L1_WEIGHTED: always, one weight per row of the operator
  ExtSpec spec;
  std::vector<T> host_basis;
  std::vector<long long> ata_off;
  std::vector<T> host_lb, host_ub, host_ata;
  // scratch of the context this set needs at sipx_finalize: the second whole-size vector of the materialised projectors, the
  // index array of a whole-array cardinality search
  bool needs_ext_scratch = false, needs_index_scratch = false;
};

// per-fiber bounds, one per coordinate along s.bdir, as one bound per row of A_i in the reference's row order
template <typename T>
void expand_fiber_bounds(const ConfigCtx& c, const SetConfig<T>& s, const T* per_fiber, std::vector<T>& rows) {
  long long dims[3] = {c.G.n[0], c.G.n[1], c.G.n[2]};
  if (s.nblk == 1) dims[s.dir[0]] -= 1;
  rows.resize(s.Mtrue);
  long long r = 0;
  for (long long k = 0; k < dims[2]; ++k)
    for (long long j = 0; j < dims[1]; ++j)
      for (long long i = 0; i < dims[0]; ++i, ++r) rows[r] = per_fiber[s.bdir == 0 ? i : (s.bdir == 1 ? j : k)];
}

// What only single-process contexts take.  RADII: vector radii live in the one projector of a single process, a rank of a sharded
// solve would each need its share of them.  L21: the groups of the l2,1 ball span the blocks of the TV operator, the gather route
// of a slab-decomposed solve is single-block.  TV_XY: the slab routes know TV's one block per dimension only.  L21_GROUPS: the segments
// of the l2,1 ball over fibers / slices share one budget, a rank would see its slab's segments (or its part of every slice) only.
// L1_WEIGHTED: the weights live in the one projector of a single process, in the padded layout of the whole operator.
// SIMPLEX: not built for sharded contexts yet (seg_simplex.h); a rank would see its part of every slice only.
// CARD_GROUPS: the segments compete for k places across the whole array (card_groups.h).
// L20: the gradient groups span the blocks of TV and compete for k places across the whole array (l20.h).
// L21_STACKED: the groups span the blocks of a caller-supplied operator (l21_stacked.h); no sharded route materialises its range.
// L2INF: the groups span the blocks of TV / TV_xy or of a caller-supplied operator, the bounds live in the one projector (l2inf.h).
enum class Sharded { RADII, L21, TV_XY, L21_GROUPS, L1_WEIGHTED, SIMPLEX, CARD_GROUPS, L20, L21_STACKED, L2INF };
inline void refuse_sharded(const ConfigCtx& c, Sharded which) {
  if (c.single_process) return;
  switch (which) {
    case Sharded::RADII:
      throw std::runtime_error("per-fiber / per-slice l1, l2 and annulus sets with one radius per segment take single-process contexts only, this "
                               "one has a communicator, a slab decomposition or set ownership: use a scalar radius, or a single process");
    case Sharded::L21:
      throw std::runtime_error("the l2,1 ball on the TV operator (isotropic total variation) takes single-process contexts only, this one "
                               "has a communicator, a slab decomposition or set ownership: use the l1 ball on TV, or a single process");
    case Sharded::TV_XY:
      throw std::runtime_error("the TV_xy operator takes single-process contexts only, this one has a communicator, a slab decomposition "
                               "or set ownership: use D_x and D_y sets, or a single process");
    case Sharded::L21_GROUPS:
      throw std::runtime_error(L21G_SHARDED);
    case Sharded::L1_WEIGHTED:
      throw std::runtime_error(L1W_SHARDED);
    case Sharded::SIMPLEX:
      throw std::runtime_error(SIMPLEX_SHARDED);
    case Sharded::CARD_GROUPS:
      throw std::runtime_error(CARDG_SHARDED);
    case Sharded::L20:
      throw std::runtime_error(L20_SHARDED);
    case Sharded::L21_STACKED:
      throw std::runtime_error(L21S_SHARDED);
    case Sharded::L2INF:
      throw std::runtime_error(L2INF_SHARDED);
  }
}
// every host path refuses an l1 radius that is not > 0 (project_l1_Duchi!.jl:22); device-supplied ones: seg_norm.h
template <typename T>
void check_l1_radii(const T* r, long long n) {
  for (long long k = 0; k < n; ++k)
    if (!(r[k] > T(0))) throw std::runtime_error("Radius of L1 ball is negative (segment " + std::to_string(k) + ")");
}

// the ExtSpec of an EXT_L21_STACKED projector on M rows in B blocks (checked: l21s_check_shape): the 1-D grid of the M rows, B blocks
// of G = M / B rows each.  The engine's set and its stand-alone calls (sipx_project, sipx_l21_stacked_norm) build it here.
inline void l21s_spec(ExtSpec& sp, long long M, int B) {
  sp.kind = EXT_L21_STACKED;
  sp.ndim = 2;
  sp.G = Grid{};
  sp.G.n[0] = M; sp.G.n[1] = 1; sp.G.n[2] = 1; sp.G.N = M; sp.G.st[0] = 1; sp.G.st[1] = M; sp.G.st[2] = M;
  sp.dims[0] = M; sp.dims[1] = 1; sp.dims[2] = 1;
  sp.mode = SIPX_MODE_WHOLE;
  sp.dir = 0;
  sp.nblk = B;
  sp.bstride = M / B;
  for (int q = 0; q < 3; ++q) sp.bdir[q] = 0;
}

// the l2,inf kinds (l2inf.h) and their groups: the entries of a vector of bounds
inline bool is_l2inf(int ext_kind) { return ext_kind == EXT_L2INF || ext_kind == EXT_L2INF_JOINT || ext_kind == EXT_L2INF_STACKED; }
inline long long l2inf_groups(const ConfigCtx& c, int ext_kind, const ExtSpec& sp) {
  return ext_kind == EXT_L2INF_STACKED ? sp.bstride : (ext_kind == EXT_L2INF_JOINT ? c.G.st[2] : c.G.N);
}

// the groups of a weighted l2,1 set on TV / TV_xy (l21_weighted.h): the grid points of EXT_L21, the pixels of EXT_L21_JOINT
// (EXT_L21_GROUPS: the segments of its spec, seg_count)
inline long long l21_groups(const ConfigCtx& c, int ext_kind) { return ext_kind == EXT_L21_JOINT ? c.G.st[2] : c.G.N; }

template <typename T>
void configure_op(const ConfigCtx& c, SetConfig<T>& s, int op) {
  const Grid& G = c.G;
  s.op = op;
  const int zdir = c.ndim == 2 ? 1 : 2;
  switch (op) {
    case SIPX_OP_IDENTITY: s.nblk = 0; break;
    case SIPX_OP_DX: s.nblk = 1; s.dir[0] = 0; break;
    case SIPX_OP_DY:
      if (c.ndim == 2) throw std::runtime_error("D_y needs a 3-D grid");
      s.nblk = 1; s.dir[0] = 1; break;
    case SIPX_OP_DZ: s.nblk = 1; s.dir[0] = zdir; break;
    case SIPX_OP_TV:                                   // vcat(D_z[,D_y],D_x): get_discrete_Grad.jl:31-33,69-72
      if (c.ndim == 2) { s.nblk = 2; s.dir[0] = 1; s.dir[1] = 0; }
      else { s.nblk = 3; s.dir[0] = 2; s.dir[1] = 1; s.dir[2] = 0; }
      break;
    case SIPX_OP_TV_XY:                                // vcat(D_y,D_x) on a 3-D grid: the in-plane part of TV
      if (c.ndim == 2)
        throw std::runtime_error("provided an unknown transform domain operator. check function get_TD_operator(comp_grid,TD_type,TF) "
                                 "for options (TV_xy is the in-plane gradient of a 3-D grid; on a 2-D grid TV is in-plane already)");
      s.nblk = 2; s.dir[0] = 1; s.dir[1] = 0;
      break;
    default: throw std::runtime_error("unknown operator kind");
  }
  s.ident = s.nblk == 0;
  s.Mtrue = 0;
  for (int q = 0; q < s.nblk; ++q) {
    const int a = s.dir[q];
    if (G.n[a] < 2) throw std::runtime_error("difference operator along a dimension of size 1");
    s.ih[q] = (T)c.ih[a];
    s.blk_rows[q] = G.N / G.n[a] * (G.n[a] - 1);
    s.Mtrue += s.blk_rows[q];
  }
  if (s.ident) s.Mtrue = G.N;
  s.Mpad = s.ident ? G.N : (long long)s.nblk * G.N;
}

// SIPX_OP_CSC: validate the SparseMatrixCSC arrays and keep host copies until sipx_finalize
template <typename T>
void configure_custom(const ConfigCtx& c, SetConfig<T>& s, const sipx_set_desc* d) {
  const long long N = c.G.N, M = d->csc_rows;
  if (!d->csc_colptr || !d->csc_rowval || !d->csc_nzval || M < 1) throw std::runtime_error("custom operator: CSC arrays missing");
  const long long nnz = d->csc_colptr[N];
  if (d->csc_colptr[0] != 0 || nnz < 0) throw std::runtime_error("custom operator: colptr must start at 0 (0-based arrays)");
  for (long long j = 0; j < N; ++j) {
    if (d->csc_colptr[j + 1] < d->csc_colptr[j]) throw std::runtime_error("custom operator: colptr must be non-decreasing");
    for (long long k = d->csc_colptr[j]; k < d->csc_colptr[j + 1]; ++k) {
      const long long r = d->csc_rowval[k];
      if (r < 0 || r >= M) throw std::runtime_error("custom operator: row index out of range");
      if (k > d->csc_colptr[j] && r <= d->csc_rowval[k - 1]) throw std::runtime_error("custom operator: rows must ascend inside a column");
    }
  }
  s.op = SIPX_OP_CSC;
  s.custom = true;
  s.nblk = 0;                       // the set kernels see an identity over M entries
  s.ident = false;
  s.Mtrue = s.Mpad = M;
  s.h_colptr.assign(d->csc_colptr, d->csc_colptr + N + 1);
  s.h_rowval.assign(d->csc_rowval, d->csc_rowval + nnz);
  s.h_nzval.assign((const T*)d->csc_nzval, (const T*)d->csc_nzval + nnz);
  s.gm.n[0] = M; s.gm.n[1] = 1; s.gm.n[2] = 1; s.gm.N = M; s.gm.st[0] = 1; s.gm.st[1] = M; s.gm.st[2] = M;
}
// a matrix-free term addresses its arrays with 32-bit indices: rows, columns and entries all below 2^31
inline void check_mf_index_range(long long N, long long M, long long nnz) {
  if (N >= (1ll << 31) || M >= (1ll << 31) || nnz >= (1ll << 31))
    throw std::runtime_error("custom sparse operator (SIPX_OP_CSC) without its A'A: the matrix-free term of Q uses 32-bit indices and needs "
                             "fewer than 2^31 columns, rows and stored entries (" + std::to_string(N) + ", " + std::to_string(M) + ", " +
                             std::to_string(nnz) + " given) -- split the operator into several sets");
}

// projector part of a set descriptor: validation (the reference's error messages) + routing
template <typename T>
void configure_proj(const ConfigCtx& c, SetConfig<T>& s, const sipx_set_desc* d) {
  const Grid& G = c.G;
  s.prox = d->proj;
  s.ncvx = d->ncvx;
  s.plo = (T)d->pmin;
  s.phi = (T)d->pmax;
  if (d->component < 0 || d->component > 3) throw std::runtime_error("Minkowski component must be 0, 1, 2 or 3");
  s.comp = d->component;
  const int mode = d->mode, dir = d->dir;
  if (mode != SIPX_MODE_WHOLE && mode != SIPX_MODE_FIBER && mode != SIPX_MODE_SLICE)
    throw std::runtime_error("unknown application mode");
  // the joint l2,1 ball (l21_joint.h) is one set on one operator: its refusal names the way out before any general one
  if (d->proj == SIPX_PROJ_L21_JOINT && (s.op != SIPX_OP_TV_XY || mode != SIPX_MODE_WHOLE || d->transform != SIPX_TRANSFORM_NONE))
    throw std::runtime_error(L21_JOINT_ROUTE);
  // so is total nuclear variation (tnv.h), which takes no vectors either
  if (d->proj == SIPX_PROJ_TNV) {
    if (s.op != SIPX_OP_TV_XY || mode != SIPX_MODE_WHOLE || d->transform != SIPX_TRANSFORM_NONE) throw std::runtime_error(TNV_ROUTE);
    if (d->lb || d->ub) throw std::runtime_error(TNV_NO_WEIGHTS);
  }
  // so is the l2,1 ball over fibers or slices (l21_groups.h): a one-block operator, no transform, no component, a mode
  if (d->proj == SIPX_PROJ_L21_GROUPS) {
    if (s.custom || s.nblk > 1) throw std::runtime_error(L21G_ONE_BLOCK);
    if (d->transform != SIPX_TRANSFORM_NONE) throw std::runtime_error(L21G_NO_TRANSFORM);
    if (s.comp) throw std::runtime_error(L21G_NO_MINKOWSKI);
    if (mode == SIPX_MODE_WHOLE) throw std::runtime_error(L21G_NEEDS_MODE);
  }
  // so is the weighted l1 ball (l1_weighted.h): a built-in operator, no transform, no component, the whole array
  if (d->proj == SIPX_PROJ_L1_WEIGHTED) {
    if (s.custom) throw std::runtime_error(L1W_NO_CUSTOM);
    if (d->transform != SIPX_TRANSFORM_NONE) throw std::runtime_error(L1W_NO_TRANSFORM);
    if (s.comp) throw std::runtime_error(L1W_NO_MINKOWSKI);
    if (mode != SIPX_MODE_WHOLE) throw std::runtime_error(L1W_NO_MODE);
  }
  // so are the simplex sets (seg_simplex.h): a one-block operator, no transform, no component, a mode
  if (d->proj == SIPX_PROJ_SIMPLEX) {
    if (s.custom || s.nblk > 1) throw std::runtime_error(SIMPLEX_ONE_BLOCK);
    if (d->transform != SIPX_TRANSFORM_NONE) throw std::runtime_error(SIMPLEX_NO_TRANSFORM);
    if (s.comp) throw std::runtime_error(SIMPLEX_NO_MINKOWSKI);
    if (mode == SIPX_MODE_WHOLE) throw std::runtime_error(SIMPLEX_NEEDS_MODE);
  }
  // so is group cardinality (card_groups.h): a one-block operator, no transform, no component, a mode
  if (d->proj == SIPX_PROJ_CARD_GROUPS) {
    if (s.custom || s.nblk > 1) throw std::runtime_error(CARDG_ONE_BLOCK);
    if (d->transform != SIPX_TRANSFORM_NONE) throw std::runtime_error(CARDG_NO_TRANSFORM);
    if (s.comp) throw std::runtime_error(CARDG_NO_MINKOWSKI);
    if (mode == SIPX_MODE_WHOLE) throw std::runtime_error(CARDG_NEEDS_MODE);
  }
  // so are the l2,0 sets (l20.h): the TV or TV_xy operator, no transform, no component, the whole array or (slice, z) on TV_xy
  if (d->proj == SIPX_PROJ_L20 || d->proj == SIPX_PROJ_L20_JOINT) {
    const bool jt = d->proj == SIPX_PROJ_L20_JOINT;
    if (d->transform != SIPX_TRANSFORM_NONE) throw std::runtime_error(L20_NO_TRANSFORM);
    if (jt && (s.op != SIPX_OP_TV_XY || mode != SIPX_MODE_WHOLE)) throw std::runtime_error(L20_JOINT_ROUTE);
    if (s.custom || (s.op != SIPX_OP_TV && s.op != SIPX_OP_TV_XY)) throw std::runtime_error(L20_NEEDS_TV);
    if (s.comp) throw std::runtime_error(L20_NO_MINKOWSKI);
    if (mode != SIPX_MODE_WHOLE && !(s.op == SIPX_OP_TV_XY && mode == SIPX_MODE_SLICE && dir == 2)) throw std::runtime_error(L20_MODES);
  }
  // so is the l2,1 ball across the blocks of a stacked operator (l21_stacked.h): a caller-supplied operator, the whole array, no
  // transform, no component, no vectors
  if (d->proj == SIPX_PROJ_L21_STACKED) {
    if (!s.custom) throw std::runtime_error(L21S_NEEDS_CSC);
    if (mode != SIPX_MODE_WHOLE) throw std::runtime_error(L21S_WHOLE_ONLY);
    if (d->transform != SIPX_TRANSFORM_NONE) throw std::runtime_error(L21S_NO_TRANSFORM);
    if (s.comp) throw std::runtime_error(L21S_NO_MINKOWSKI);
    if (d->lb || d->ub || d->reserved) throw std::runtime_error(L21S_NO_VECTORS);
  }
  // so are the l2,inf sets (l2inf.h): TV or TV_xy, TV_xy for the joint set, a caller-supplied operator for the stacked one; the whole
  // array, no transform, no component, no lower bound, no weights
  if (d->proj == SIPX_PROJ_L2INF || d->proj == SIPX_PROJ_L2INF_JOINT || d->proj == SIPX_PROJ_L2INF_STACKED) {
    if (d->transform != SIPX_TRANSFORM_NONE) throw std::runtime_error(L2INF_NO_TRANSFORM);
    if (d->proj == SIPX_PROJ_L2INF_JOINT && s.op != SIPX_OP_TV_XY) throw std::runtime_error(L2INF_JOINT_ROUTE);
    if (d->proj == SIPX_PROJ_L2INF_STACKED && !s.custom) throw std::runtime_error(L2INF_STACKED_NEEDS_CSC);
    if (d->proj == SIPX_PROJ_L2INF && (s.custom || (s.op != SIPX_OP_TV && s.op != SIPX_OP_TV_XY))) throw std::runtime_error(L2INF_NEEDS_TV);
    if (s.comp) throw std::runtime_error(L2INF_NO_MINKOWSKI);
    if (mode != SIPX_MODE_WHOLE) throw std::runtime_error(L2INF_MODES);
    if (d->pmin != 0) throw std::runtime_error(L2INF_MIN);
    if (d->lb) throw std::runtime_error(L2INF_NO_WEIGHTS);
  }
  if (mode != SIPX_MODE_WHOLE) {
    if (dir < 0 || dir >= c.ndim) throw std::runtime_error("application mode: direction out of range for this grid");
    // the one multi-block set with a mode of its own: the l2,1 ball per z-slice on TV_xy (l21_seg.h)
    const bool l20_frames = d->proj == SIPX_PROJ_L20;      // ((slice, z) on TV_xy: checked above)
    const bool frames = (d->proj == SIPX_PROJ_L21 && s.op == SIPX_OP_TV_XY && d->transform == SIPX_TRANSFORM_NONE) || l20_frames;
    if (frames && !(mode == SIPX_MODE_SLICE && dir == 2))
      throw std::runtime_error("the l2,1 ball on TV_xy: frames run along z -- the mode must be (slice, z), or tensor for the whole array");
    if (s.nblk > 1 && !frames) throw std::runtime_error("fiber / slice modes need an operator with one block (identity, D_x, D_y, D_z)");
  }
  auto ext = [&](int kind) {
    if (s.nblk > 1 && kind != EXT_L21 && kind != EXT_L21_SEG && kind != EXT_L21_JOINT && kind != EXT_TNV && kind != EXT_L1_WEIGHTED && kind != EXT_L20 && kind != EXT_L20_SEG && kind != EXT_L20_JOINT && kind != EXT_L2INF && kind != EXT_L2INF_JOINT) throw std::runtime_error("this projector needs an operator with one block (identity, D_x, D_y, D_z)");
    s.ext_kind = kind;
    s.spec.kind = kind;
    s.spec.ndim = c.ndim;
    s.spec.G = G;
    for (int a = 0; a < 3; ++a) s.spec.dims[a] = G.n[a];
    if (s.nblk == 1) s.spec.dims[s.dir[0]] -= 1;           // TD_n of a difference operator (get_TD_operator.jl)
    s.spec.mode = mode;
    s.spec.dir = dir;
    s.spec.pmin = d->pmin;
    s.spec.pmax = d->pmax;
    s.spec.nblk = s.nblk;                                  // EXT_L21: the blocks side by side, full padded grids
    s.spec.bstride = G.N;
    for (int q = 0; q < 3; ++q) s.spec.bdir[q] = q < s.nblk ? s.dir[q] : 0;
    s.prox = PX_EXT;
    s.needs_ext_scratch = true;
  };
  // l1 / l2 / annulus per fiber or slice: the scalars, or one radius per segment in ub (and lb: the annulus' inner radii)
  auto seg_norm = [&](int kind) {
    const bool vec = d->ub || (kind == EXT_ANNULUS_SEG && d->lb);
    if (kind == EXT_L1_SEG && !vec && !(d->pmax > 0)) throw std::runtime_error("Radius of L1 ball is negative");   // project_l1_Duchi!.jl:22
    ext(kind);
    if (!vec) return;
    refuse_sharded(c, Sharded::RADII);
    const long long nseg = seg_count(s.spec);
    s.seg_radii = true;
    if (d->ub) s.host_ub.assign((const T*)d->ub, (const T*)d->ub + nseg);
    else s.host_ub.assign((size_t)nseg, (T)d->pmax);
    if (kind == EXT_ANNULUS_SEG) {
      if (d->lb) s.host_lb.assign((const T*)d->lb, (const T*)d->lb + nseg);
      else s.host_lb.assign((size_t)nseg, (T)d->pmin);
    }
    if (kind == EXT_L1_SEG) check_l1_radii(s.host_ub.data(), nseg);
  };
  if (d->transform == SIPX_TRANSFORM_DCT) {      // x -> C' P(C x): P acts on the DCT coefficients (ext_proj.hip)
    if (d->op != SIPX_OP_IDENTITY || mode != SIPX_MODE_WHOLE)
      throw std::runtime_error("sets behind the DCT act in their own domain: TD_OP must be the identity, mode matrix/tensor");
    if (d->proj != SIPX_PROJ_BOUNDS && d->proj != SIPX_PROJ_BOUNDS_VEC && d->proj != SIPX_PROJ_L1 &&
        d->proj != SIPX_PROJ_CARDINALITY)
      throw std::runtime_error("behind the DCT: bounds, the l1 ball and cardinality are built (l2 / annulus commute with it)");
    if (d->proj == SIPX_PROJ_L1 && !(d->pmax > 0)) throw std::runtime_error("Radius of L1 ball is negative");
    if (d->proj == SIPX_PROJ_BOUNDS_VEC) {
      if (!d->lb || !d->ub) throw std::runtime_error("per-element bounds need lb and ub");
      s.host_lb.assign((const T*)d->lb, (const T*)d->lb + G.N);
      s.host_ub.assign((const T*)d->ub, (const T*)d->ub + G.N);
    }
    ext(EXT_DCT);
    s.spec.inner = d->proj;
    return;
  } else if (d->transform == SIPX_TRANSFORM_WAVELET) {      // x -> W' P(W x): P acts on the db4 wavelet coefficients (kernels_dwt.hip)
    if (d->op != SIPX_OP_IDENTITY || mode != SIPX_MODE_WHOLE)
      throw std::runtime_error("sets behind the wavelet transform act in their own domain: TD_OP must be the identity, mode matrix/tensor");
    if (d->proj != SIPX_PROJ_BOUNDS && d->proj != SIPX_PROJ_L1 && d->proj != SIPX_PROJ_CARDINALITY)
      throw std::runtime_error("behind the wavelet transform: scalar bounds, the l1 ball and cardinality are built (l2 / annulus commute "
                               "with it; per-element bounds would depend on the coefficient layout)");
    if (d->proj == SIPX_PROJ_L1 && !(d->pmax > 0)) throw std::runtime_error("Radius of L1 ball is negative");
    dwt_check_grid(c.ndim, G.n);
    ext(EXT_DWT);
    s.spec.inner = d->proj;
    return;
  } else if (d->transform != SIPX_TRANSFORM_NONE) {
    throw std::runtime_error("unknown transform");
  }
  // one weight per group in lb (l21_weighted.h): EXT_L21 on the whole array and EXT_L21_JOINT
  // (the refusals of the weighted sets are worded in l21_weighted.h, beside the rule)
  auto weights = [&](const char* set) {
    const long long n = l21_groups(c, s.ext_kind);
    l21w_check_desc(set, d->lb != nullptr, d->ub != nullptr, d->reserved, n, s.ext_kind == EXT_L21_JOINT);      // (reserved: the entries lb holds)
    if (!d->lb) return;
    check_l21_weights((const T*)d->lb, n, set);
    s.weighted = true;
    s.spec.weighted = 1;
    s.host_lb.assign((const T*)d->lb, (const T*)d->lb + n);
  };
  switch (d->proj) {
    case SIPX_PROJ_BOUNDS:
      if (mode != SIPX_MODE_WHOLE) throw std::runtime_error("scalar bounds apply to the whole array (use per-fiber vectors)");
      break;
    case SIPX_PROJ_PROX_L1:
      if (mode != SIPX_MODE_WHOLE) throw std::runtime_error("prox_l1 applies to the whole array");
      break;
    case SIPX_PROJ_BOUNDS_VEC:
      if (!d->lb || !d->ub) throw std::runtime_error("per-element bounds need lb and ub");
      if (mode == SIPX_MODE_SLICE)
        throw std::runtime_error("bound constraints per slice of a tensor currently not implemented, yet...");   // project_bounds!.jl:83
      s.bmode = mode;
      s.bdir = dir;
      if (mode == SIPX_MODE_FIBER) {      // bounds per fiber: expanded to one bound per row of A_i (reference order)
        expand_fiber_bounds(c, s, (const T*)d->lb, s.host_lb);
        expand_fiber_bounds(c, s, (const T*)d->ub, s.host_ub);
        s.plo = T(1);                       // min(max(x, LB), UB): the fiber methods clip with LB first (project_bounds!.jl:47,65)
      } else {
        s.host_lb.assign((const T*)d->lb, (const T*)d->lb + s.Mtrue);
        s.host_ub.assign((const T*)d->ub, (const T*)d->ub + s.Mtrue);
        s.plo = T(0);
      }
      break;
    // l1, l2, annulus: the whole array through the engine's own two-pass search; per fiber / slice (a gap of the reference,
    // setup_constraints.jl:65-67 "currently") on the materialised vector, every segment by the same rule (seg_norm.h)
    case SIPX_PROJ_L1:
      if (mode == SIPX_MODE_WHOLE) {
        if (!(d->pmax > 0)) throw std::runtime_error("Radius of L1 ball is negative");   // project_l1_Duchi!.jl:22
        s.two_pass = true;
      } else seg_norm(EXT_L1_SEG);
      break;
    case SIPX_PROJ_L2:
      if (mode == SIPX_MODE_WHOLE) s.two_pass = true;
      else seg_norm(EXT_L2_SEG);
      break;
    case SIPX_PROJ_ANNULUS:
      if (mode == SIPX_MODE_WHOLE) s.two_pass = true;
      else seg_norm(EXT_ANNULUS_SEG);
      break;
    case SIPX_PROJ_CARDINALITY:
      if (mode == SIPX_MODE_WHOLE) { s.two_pass = true; s.needs_index_scratch = true; }
      else ext(EXT_CARD_SEG);
      break;
    case SIPX_PROJ_L1_DFT:
      if (d->op != SIPX_OP_IDENTITY || mode != SIPX_MODE_WHOLE)
        throw std::runtime_error("the DFT-l1 projector acts in its own domain: TD_OP must be the identity, mode matrix/tensor");
      if (!(d->pmax > 0)) throw std::runtime_error("Radius of L1 ball is negative");
      ext(EXT_L1_DFT);
      break;
    case SIPX_PROJ_BOUNDS_DFT:
      if (d->op != SIPX_OP_IDENTITY || mode != SIPX_MODE_WHOLE)
        throw std::runtime_error("bounds in the DFT domain act in their own domain: TD_OP must be the identity, mode matrix/tensor");
      if (!d->ub) throw std::runtime_error("bounds in the DFT domain need the mask vector (constraint.max)");
      ext(EXT_DFT_MASK);
      s.host_ub.assign((const T*)d->ub, (const T*)d->ub + G.N);
      break;
    case SIPX_PROJ_CARD_DFT:
      if (d->op != SIPX_OP_IDENTITY || mode != SIPX_MODE_WHOLE)
        throw std::runtime_error("cardinality behind the DFT acts in its own domain: TD_OP must be the identity, mode matrix/tensor");
      if (d->pmax < 0 || d->pmax != std::floor(d->pmax))
        throw std::runtime_error("cardinality behind the DFT: k must be a non-negative integer");
      ext(EXT_CARD_DFT);
      break;
    case SIPX_PROJ_L21:        // isotropic TV: groups across the blocks of the TV operator (l21.h), on the materialised vector
      if (d->op != SIPX_OP_TV && d->op != SIPX_OP_TV_XY)
        throw std::runtime_error("the l2,1 ball acts on the range of the TV operator: TD_OP must be TV (D2D, D3D)");
      // (a mode on TV itself never gets here: more than one block; nor a grid of 2^31 points: no context has one)
      if (s.comp) throw std::runtime_error("the l2,1 ball takes no Minkowski component");
      refuse_sharded(c, Sharded::L21);
      if (mode == SIPX_MODE_WHOLE) {
        if (!(d->pmax > 0)) throw std::runtime_error("Radius of L1 ball is negative");
        ext(EXT_L21);
        weights("l21");
      } else {
        if (d->lb) l21w_refuse_frames();                 // per frame on TV_xy (checked above): the scalar, or one radius per frame in ub
        if (!d->ub && !(d->pmax > 0)) throw std::runtime_error("Radius of L1 ball is negative");
        ext(EXT_L21_SEG);
        if (d->ub) {
          s.seg_radii = true;
          s.host_ub.assign((const T*)d->ub, (const T*)d->ub + G.n[2]);
          check_l1_radii(s.host_ub.data(), G.n[2]);
        }
      }
      break;
    case SIPX_PROJ_L21_JOINT:  // vectorial TV: one group per pixel across the blocks of TV_xy and all frames (op, mode, transform: above)
      if (s.comp) throw std::runtime_error("the l2,1 ball takes no Minkowski component");
      refuse_sharded(c, Sharded::L21);
      if (!(d->pmax > 0)) throw std::runtime_error("Radius of L1 ball is negative");
      ext(EXT_L21_JOINT);
      weights("l21_joint");
      break;
    case SIPX_PROJ_TNV:        // total nuclear variation: the Jacobians of the pixels across the frames of TV_xy (op, mode, transform, vectors: above)
      if (s.comp) throw std::runtime_error("the TV_xy operator takes no Minkowski component");      // (the operator's own text, for sipx_project)
      refuse_sharded(c, Sharded::L21);
      if (!(d->pmax > 0)) throw std::runtime_error("Radius of L1 ball is negative");
      ext(EXT_TNV);
      break;
    case SIPX_PROJ_L21_GROUPS: {  // group sparsity: one group per fiber or slice of the valid block (op, transform, component, mode: above)
      if (c.ndim == 2 && mode == SIPX_MODE_SLICE) throw std::runtime_error(L21G_2D_SLICE);
      refuse_sharded(c, Sharded::L21_GROUPS);
      if (!(d->pmax > 0)) throw std::runtime_error("Radius of L1 ball is negative");
      ext(EXT_L21_GROUPS);
      const long long nseg = seg_count(s.spec);
      l21g_check_desc(d->lb != nullptr, d->ub != nullptr, d->reserved, nseg, mode == SIPX_MODE_FIBER, dir, s.spec.dims);   // (reserved: the entries lb holds)
      if (d->lb) {
        check_l21_weights((const T*)d->lb, nseg, "l21_groups");
        s.weighted = true;
        s.spec.weighted = 1;
        s.host_lb.assign((const T*)d->lb, (const T*)d->lb + nseg);
      }
      break;
    }
    case SIPX_PROJ_L1_WEIGHTED: {  // one weight per row of the operator in lb (operator, transform, component, mode: above); lb NULL: the
                                   // weights come with sipx_set_data(_dev) before the first solve, until then no row is constrained
      refuse_sharded(c, Sharded::L1_WEIGHTED);
      if (!(d->pmax > 0)) throw std::runtime_error("Radius of L1 ball is negative");
      ext(EXT_L1_WEIGHTED);
      l1w_check_desc(d->ub != nullptr, d->reserved, s.Mtrue);      // (reserved: the entries lb holds)
      s.weighted = true;
      s.spec.weighted = 1;
      if (d->lb) {
        check_l1w_weights((const T*)d->lb, s.Mtrue);
        s.host_lb.assign((const T*)d->lb, (const T*)d->lb + s.Mtrue);
      }
      break;
    }
    case SIPX_PROJ_CARD_GROUPS:  // at most pmax non-zero fibers or slices of the valid block (operator, transform, component, mode: above)
      if (c.ndim == 2 && mode == SIPX_MODE_SLICE) throw std::runtime_error(CARDG_2D_SLICE);
      if (d->lb || d->ub || d->reserved) throw std::runtime_error(CARDG_NO_VECTORS);
      refuse_sharded(c, Sharded::CARD_GROUPS);
      if (G.N >= (1ll << 31)) throw std::runtime_error(CARDG_TOO_LARGE);
      ext(EXT_CARD_GROUPS);
      cardg_check_k<T>(d->pmax, seg_count(s.spec));
      break;
    case SIPX_PROJ_L20:        // at most pmax grid points carry a gradient vector, or per frame pmax / ub[frame] pixels (operator, transform,
    case SIPX_PROJ_L20_JOINT:  // component, mode: above); at most pmax pixels carry one in any frame
      if (d->lb || d->reserved) throw std::runtime_error(L20_NO_WEIGHTS);
      if (d->ub && mode == SIPX_MODE_WHOLE) throw std::runtime_error(L20_K_VECTOR);
      refuse_sharded(c, Sharded::L20);
      if (G.N >= (1ll << 31)) throw std::runtime_error(L20_TOO_LARGE);
      if (mode == SIPX_MODE_WHOLE) {
        ext(d->proj == SIPX_PROJ_L20_JOINT ? EXT_L20_JOINT : EXT_L20);
        l20_check_k<T>(d->pmax, d->proj == SIPX_PROJ_L20_JOINT ? G.st[2] : G.N);
      } else {
        ext(EXT_L20_SEG);
        if (d->ub) {
          s.seg_radii = true;
          s.host_ub.assign((const T*)d->ub, (const T*)d->ub + G.n[2]);
          l20_check_k_vector<T>(s.host_ub.data(), G.n[2], G.n[0] * G.n[1]);
        } else {
          l20_check_k<T>(d->pmax, G.n[0] * G.n[1]);
        }
      }
      break;
    case SIPX_PROJ_L21_STACKED: {  // one group per row index of a block, across the d->blocks equal-sized blocks of the caller-supplied
                                   // operator (operator, mode, transform, component, vectors: above)
      l21s_check_shape(s.Mtrue, d->blocks);
      refuse_sharded(c, Sharded::L21_STACKED);
      if (!(d->pmax > 0)) throw std::runtime_error("Radius of L1 ball is negative");
      ext(EXT_L21_STACKED);
      l21s_spec(s.spec, s.Mtrue, d->blocks);
      break;
    }
    case SIPX_PROJ_L2INF:          // every group norm at most pmax, or ub[group] with `reserved` its entries (operator, mode, transform,
    case SIPX_PROJ_L2INF_JOINT:    // component, pmin, lb: above): the groups of SIPX_PROJ_L21, of SIPX_PROJ_L21_JOINT,
    case SIPX_PROJ_L2INF_STACKED: {  // of SIPX_PROJ_L21_STACKED
      const int kind = d->proj == SIPX_PROJ_L2INF ? EXT_L2INF : (d->proj == SIPX_PROJ_L2INF_JOINT ? EXT_L2INF_JOINT : EXT_L2INF_STACKED);
      if (kind == EXT_L2INF_STACKED) l2infs_check_shape(s.Mtrue, d->blocks);
      refuse_sharded(c, Sharded::L2INF);
      ext(kind);
      if (kind == EXT_L2INF_STACKED) {
        l21s_spec(s.spec, s.Mtrue, d->blocks);
        s.spec.kind = kind;
      }
      const long long groups = l2inf_groups(c, kind, s.spec);
      if (!d->ub) {
        if (d->reserved) throw std::runtime_error(l2inf_bad_length(d->reserved, 0) + " -- reserved counts the entries of ub, which is NULL");
        l2inf_check_c(d->pmax);
        break;
      }
      if (d->reserved != groups) throw std::runtime_error(l2inf_bad_length(d->reserved, groups));      // (reserved: the entries ub holds)
      // (a group without a member -- the last corner of the grid, of every frame of TV_xy, the last pixel -- is not looked at)
      const long long per = kind == EXT_L2INF && s.op == SIPX_OP_TV_XY ? G.st[2] : groups;
      l2inf_check_vector<T>((const T*)d->ub, groups, [&](long long p) { return kind == EXT_L2INF_STACKED || p % per != per - 1; });
      s.seg_radii = true;
      s.host_ub.assign((const T*)d->ub, (const T*)d->ub + groups);
      break;
    }
    case SIPX_PROJ_SIMPLEX:  // entries >= 0 and a sum in [pmin, pmax] per fiber or slice (operator, transform, component, mode: above)
      if (c.ndim == 2 && mode == SIPX_MODE_SLICE) throw std::runtime_error(SIMPLEX_2D_SLICE);
      if (d->lb || d->ub) throw std::runtime_error(SIMPLEX_NO_VECTORS);
      refuse_sharded(c, Sharded::SIMPLEX);
      simplex_check_bounds<T>(d->pmin, d->pmax);
      ext(EXT_SIMPLEX_SEG);
      break;
    case SIPX_PROJ_RANK: ext(EXT_RANK); break;
    case SIPX_PROJ_NUCLEAR: ext(EXT_NUCLEAR); break;
    case SIPX_PROJ_HISTOGRAM:
      if (!d->lb || !d->ub) throw std::runtime_error("histogram constraints need sorted lb and ub vectors");
      ext(EXT_HISTOGRAM);
      s.host_lb.assign((const T*)d->lb, (const T*)d->lb + s.Mtrue);     // kept on the host until the ExtProj is built
      s.host_ub.assign((const T*)d->ub, (const T*)d->ub + s.Mtrue);
      break;
    case SIPX_PROJ_SUBSPACE:
      if (d->op != SIPX_OP_IDENTITY) throw std::runtime_error("subspace constraints act on the model itself: TD_OP must be the identity");
      if (!d->basis || d->basis_cols < 1 || d->basis_rows < 1) throw std::runtime_error("subspace constraints need the matrix A");
      ext(EXT_SUBSPACE);
      s.host_basis.assign((const T*)d->basis, (const T*)d->basis + (size_t)d->basis_rows * d->basis_cols);
      s.spec.basis_rows = d->basis_rows;
      s.spec.basis_cols = d->basis_cols;
      s.spec.basis_orth = d->basis_orth;
      break;
    default: throw std::runtime_error("unknown projector kind");
  }
}

template <typename T>
std::vector<long long> default_ata_offsets(const ConfigCtx& c, const SetConfig<T>& s) {   // mat2CDS: ascending (mat2CDS.jl:9-13)
  const Grid& G = c.G;
  std::vector<long long> o = {0};
  for (int q = 0; q < s.nblk; ++q) {
    o.push_back(G.st[s.dir[q]]);
    o.push_back(-G.st[s.dir[q]]);
  }
  std::sort(o.begin(), o.end());
  o.erase(std::unique(o.begin(), o.end()), o.end());
  if (s.comp == 3) {     // [B B; B B]: every diagonal of B also shifted by -N and +N (mat2CDS of the 2N x 2N block matrix)
    std::vector<long long> all;
    for (long long sh : {-G.N, 0ll, G.N})
      for (long long v : o) all.push_back(v + sh);
    std::sort(all.begin(), all.end());
    all.erase(std::unique(all.begin(), all.end()), all.end());
    return all;
  }
  return o;
}

// entries of the vectors a set takes (sipx_add_set, sipx_set_data): radii per segment, bounds per fiber coordinate, or one per row
template <typename T>
long long data_len(const ConfigCtx& c, const SetConfig<T>& s) {
  if (s.ext_kind == EXT_L1_WEIGHTED) return s.Mtrue;
  if (is_l2inf(s.ext_kind)) return l2inf_groups(c, s.ext_kind, s.spec);
  if (s.weighted) return s.ext_kind == EXT_L21_GROUPS ? seg_count(s.spec) : l21_groups(c, s.ext_kind);
  if (s.seg_radii) return (s.ext_kind == EXT_L21_SEG || s.ext_kind == EXT_L20_SEG) ? c.G.n[2] : seg_count(s.spec);
  if (s.ext_kind || s.bmode != SIPX_MODE_FIBER) return s.Mtrue;
  return c.G.n[s.bdir] - ((s.nblk == 1 && s.dir[0] == s.bdir) ? 1 : 0);
}

// sipx_add_set: the operator, the projector and what the two must not combine; ata_R (TF[N x d_i], offsets ata_off) are the bands
// of A'A the caller supplies, NULL: the descriptor's own, or for a custom operator a matrix-free term of Q
template <typename T>
SetConfig<T> configure_set(const ConfigCtx& c, const sipx_set_desc* d, const void* ata_R, const int64_t* ata_off, int d_i) {
  SetConfig<T> s;
  if (d->op == SIPX_OP_CSC) configure_custom(c, s, d);
  else configure_op(c, s, d->op);
  if (s.op == SIPX_OP_TV_XY) {
    refuse_sharded(c, Sharded::TV_XY);
    if (d->component) throw std::runtime_error("the TV_xy operator takes no Minkowski component");
  }
  configure_proj(c, s, d);
  // (the materialised projectors a custom operator takes: the l2,1 and the l2,inf ball across its blocks, which act on s = A x as a whole)
  if (s.custom && (s.comp || (s.ext_kind && s.ext_kind != EXT_L21_STACKED && s.ext_kind != EXT_L2INF_STACKED)))
    throw std::runtime_error("custom sparse operators (SIPX_OP_CSC): Minkowski components and library-backed projectors are not available; "
                             "use one of the built-in operators for such a set");
  if (s.custom && !ata_R) {              // matrix-free term of Q: no bands, the products go through the operator itself
    check_mf_index_range(c.G.N, s.Mtrue, (long long)s.h_rowval.size());
    s.mfree = true;
  }
  if (ata_R && s.comp) throw std::runtime_error("Minkowski sets use descriptor-generated AtA (pass ata_R = NULL)");
  if (ata_R) {
    if (d_i < 1 || d_i > 9) throw std::runtime_error("AtA band count out of range (1..9 bands per set)");
    s.ata_off.assign(ata_off, ata_off + d_i);
    s.host_ata.assign((const T*)ata_R, (const T*)ata_R + (size_t)c.G.N * d_i);
  } else if (!s.mfree) {
    s.ata_off = default_ata_offsets(c, s);
  }
  return s;
}

}  // namespace sipx
