// Projectors that act on a materialised vector v (one block of the padded layout): library transforms
// (hipFFT / rocSOLVER / rocBLAS / hipCUB sort) and the per-fiber / per-slice selections; see ext_proj.hip.  EXT_L21, EXT_L21_SEG and EXT_L21_JOINT alone
// act on the nblk blocks of the TV / TV_xy operator at once (ext_group.hip), as does EXT_L1_WEIGHTED on the blocks of any built-in operator.
#pragma once
#include "sipx_common.h"

namespace sipx {

enum { EXT_L1_DFT = 1, EXT_RANK = 2, EXT_NUCLEAR = 3, EXT_CARD_SEG = 4, EXT_HISTOGRAM = 5, EXT_SUBSPACE = 6, EXT_DFT_MASK = 7, EXT_DCT = 8, EXT_DWT = 9, EXT_CARD_DFT = 10,
       EXT_L1_SEG = 11, EXT_L2_SEG = 12, EXT_ANNULUS_SEG = 13 /* l1 / l2 / annulus per fiber or slice */,
       EXT_L21 = 14 /* the l2,1 ball across the blocks of the TV / TV_xy operator (l21.h) */,
       EXT_L21_SEG = 15 /* the l2,1 ball of every z-slice across the blocks of TV_xy (l21_seg.h) */,
       EXT_L21_JOINT = 16 /* the l2,1 ball whose groups span the blocks of TV_xy and the frames (l21_joint.h) */,
       EXT_L21_GROUPS = 17 /* the l2,1 ball whose groups are the fibers or slices of a one-block operator's range (l21_groups.h) */,
       EXT_TNV = 18 /* total nuclear variation: the nuclear-norm ball on the 2 x n3 Jacobians of the pixels of TV_xy (tnv.h) */,
       EXT_L1_WEIGHTED = 19 /* the weighted l1 ball on the rows of identity, D_x, D_y, D_z, TV or TV_xy, one weight per row (l1_weighted.h) */,
       EXT_SIMPLEX_SEG = 20 /* the simplex of every fiber or slice: entries >= 0, sum in [pmin, pmax] (seg_simplex.h) */,
       EXT_CARD_GROUPS = 21 /* at most pmax non-zero fibers or slices of a one-block operator's range (card_groups.h) */,
       EXT_L20 = 22 /* at most pmax grid points with a non-zero gradient vector on the range of TV / TV_xy (l20.h) */,
       EXT_L20_SEG = 23 /* ... at most pmax (or ub[frame]) pixels in every z-slice of TV_xy */,
       EXT_L20_JOINT = 24 /* ... at most pmax pixels that carry a gradient in any frame of TV_xy */,
       EXT_L21_STACKED = 25 /* the l2,1 ball across the equal-sized blocks of a caller-supplied operator (l21_stacked.h) */,
       EXT_L2INF = 26 /* every group norm of TV / TV_xy at most pmax, or ub[grid point] (l2inf.h) */,
       EXT_L2INF_JOINT = 27 /* ... every norm of the groups of EXT_L21_JOINT at most pmax, or ub[pixel] */,
       EXT_L2INF_STACKED = 28 /* ... every norm of the groups of EXT_L21_STACKED at most pmax, or ub[row of a block] */ };

// The refusal of an EXT_L21_JOINT set off its operator or mode, worded once: set_config.h (sipx_add_set), the stand-alone calls of the
// engine and the projector's own check throw this text (its cases: tests/test_l21_joint_cpu.py, tests/test_gpu_l21_joint.py)
constexpr const char* L21_JOINT_ROUTE = "the joint l2,1 ball groups the frames of TV_xy: TD_OP must be TV_xy, mode tensor";
// The refusals of an EXT_TNV set, worded once in the same way (their cases: tests/test_tnv_cpu.py, tests/test_gpu_tnv.py): off its operator
// or mode or behind a transform, and with vectors in lb / ub
constexpr const char* TNV_ROUTE = "total nuclear variation couples the frames of TV_xy: TD_OP must be TV_xy, mode tensor, no transform";
constexpr const char* TNV_NO_WEIGHTS = "total nuclear variation (tnv) takes no weights or vectors (lb, ub): the weighted set across the frames is "
                                       "(\"l21_joint\", \"TV_xy\")";

// What an ExtProj acts on: the valid extents `dims` (TD_n of the operator) inside the padded grid G (strides G.st),
// split into segments by the application mode (whole array, fibers along `dir`, slices orthogonal to `dir`).
struct ExtSpec {
  int kind = 0;
  int ndim = 3;
  Grid G;
  long long dims[3] = {1, 1, 1};
  int mode = 0, dir = 2;          // SIPX_MODE_*, 0-based direction
  double pmin = 0, pmax = 0;
  int inner = 0;                  // EXT_DCT / EXT_DWT: the SIPX_PROJ_* kind applied to the transform coefficients
  const void* lb = nullptr;       // EXT_HISTOGRAM: host TF[prod(dims)], ascending; EXT_L1_SEG / L2_SEG / ANNULUS_SEG: host TF[nseg]
                                  // radii per segment (ub: pmax of each, lb: the annulus' pmin of each), or nullptr: the scalars
  const void* ub = nullptr;
  const void* basis = nullptr;    // EXT_SUBSPACE: host TF[basis_rows x basis_cols], column-major
  long long basis_rows = 0;
  int basis_cols = 0, basis_orth = 0;
  int nblk = 0;                   // EXT_L21(_SEG): blocks of the operator (2 or 3), block q at v + q * bstride holding the differences along bdir[q]
                                  // EXT_L21_STACKED: the B blocks (1 .. 8) of the caller-supplied operator, bstride = G their rows each, G the
                                  // 1-D grid of the M = B G rows; bdir is not looked at
                                  // EXT_L2INF, EXT_L2INF_JOINT as EXT_L21, EXT_L2INF_STACKED as EXT_L21_STACKED; ub: host TF[groups], one bound per
                                  // group, or nullptr: the scalar pmax
  long long bstride = 0;
  int bdir[3] = {0, 0, 0};
  int weighted = 0;               // EXT_L21 (whole array) / EXT_L21_JOINT / EXT_L21_GROUPS: 1: one weight per group (l21_weighted.h) -- lb: host TF[groups], or
                                  // nullptr: set_data brings them before the first projection
                                  // EXT_L1_WEIGHTED: always 1 -- lb: host TF[rows of the operator] in the reference's row order, or nullptr as above;
                                  // nblk (0: the identity, 1 .. 3), bstride == G.N and bdir as for EXT_L21
};

template <typename T>
struct ExtImpl;

template <typename T>
class ExtProj {
 public:
  ExtProj(const ExtSpec& spec, hipStream_t stream);
  ~ExtProj();
  ExtProj(const ExtProj&) = delete;
  // v <- P(v) in place (padded layout, G.N entries); feas selects the warm-start state of the feasibility estimate
  void project(T* v, bool feas, double* partials, T* maxpart, T* compact);
  // the l2,1 sets (ext_group.hip): out (device) <- what project(v, ...) would compare with the radius, summed and rounded by the
  // projector's own launches -- ||v||_2,1 for EXT_L21, the sum of the G group norms across the blocks for EXT_L21_STACKED, the sum of the n1 n2 group norms for EXT_L21_JOINT, one sum per z-slice (n3
  // entries) for EXT_L21_SEG, the weighted sum of the segment norms for EXT_L21_GROUPS, the sum of the 2 n1 n2 singular values for EXT_TNV; and sum_i w_i |v_i| for EXT_L1_WEIGHTED; one sum of the positive parts per segment (nseg entries, SegMap's order) for EXT_SIMPLEX_SEG; the l2 norm of every segment (nseg entries, the selection key) for EXT_CARD_GROUPS; the norm of every gradient group (N entries in point order, EXT_L20_JOINT: the n1 n2 pixels; the selection key) for the EXT_L20 kinds; the largest group norm (one number) for the EXT_L2INF kinds.  v and the warm starts are not written; the scratch is that of project.  The other kinds throw.
  void observe(const T* v, T* out, double* partials, T* maxpart, T* compact);
  // rank projector: calls since construction, calls served by the warm-started subspace route, calls that decomposed fully,
  // products with the Gram matrices the subspace route spent (all zero for the other kinds)
  void route_counts(long long out[4]) const;
  // the stream of the calls to come (the engine runs the slice-rank set of a long list on a lane of its own)
  void set_stream(hipStream_t s);
  // forget every warm start and counter: the projector behaves like a newly built one (sipx_reset)
  void reset();
  // replaces the vectors the projector was built with (sipx_set_data): lb / ub as in ExtSpec, host or device memory, nullptr keeps
  // that vector; queued on the projector's stream, nothing is allocated.  Kinds without such vectors throw.
  void set_data(const T* lb, const T* ub, bool on_device);
  // device bytes the projector holds
  long long device_bytes() const;

 private:
  ExtImpl<T>* impl_;
};

// out[s] <- the l1 (norm_l2 = 0) or l2 norm of segment s of v (padded layout, spec.mode FIBER / SLICE), seg_count(spec) entries
// (ext_family.h) in the order of the per-segment radii (seg_norm.h: k_seg_observe)
template <typename T>
void seg_observe(const ExtSpec& spec, int norm_l2, const T* v, T* out, hipStream_t stream);

// sipx_card_groups_route, a hook of the tests and of tools/card_groups_bench.py: the selection route of the EXT_CARD_GROUPS projectors built
// and of the EXT_L20 / EXT_L20_JOINT projectors (tools/l20_bench.py) from now on in this process -- 0: by the number of segments, 1: the small route (k_cardg_rank), 2: the engine's search
void card_groups_force_route(int route);

// sum (projected - original)^2 and sum original^2 into partial slots dst[0..NB), dst[NB..2NB)
template <typename T>
void ext_dist2(hipStream_t s, long long N, const T* projected, const T* original, double* dst);

}  // namespace sipx
