/*
 * sipx.h -- C ABI of the MI355X-native PARSDMM projection engine (libsipx.so).
 *
 * This is the drop-in boundary for ONE hot path of slimgroup/SetIntersectionProjection.jl:
 * the PARSDMM iteration body behind
 *     PARSDMM(m, AtA, TD_OP, set_Prop, P_sub, comp_grid, options[, x, l, y]) -> (x, log, l, y)
 * (reference src/PARSDMM.jl:25-35,257).  Plain pointers and sizes only; every function that
 * returns int returns 0 on success and non-zero on error (text via sipx_last_error()) -- with ONE
 * exception, sipx_add_set, which returns the index (>= 0) of the set it added and -1 on error.
 * Host arrays are
 * copied in / copied out; the library never keeps a caller pointer after a call returns
 * (reference ownership model: Julia owns every array).
 *
 * Two granularities, B built on A:
 *   A. phase level  -- one entry per step of the reference's main loop, so PARSDMM.jl's own
 *      loop, @timeit sections and stop_PARSDMM can stay in Julia and ccall each phase;
 *   B. whole solve  -- sipx_parsdmm() runs the restated loop natively.
 *
 * A handle is single-threaded (one solve at a time); different handles may live on
 * different host threads / GPUs.  All vectors are TF = float or double as chosen at
 * sipx_create().  Per-set scalars cross the ABI as double (exact for float values).
 */
#ifndef SIPX_H
#define SIPX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sipx_ctx sipx_ctx;

enum { SIPX_F32 = 0, SIPX_F64 = 1 };

/* Transform-domain operator A_i, matrix-free.  Replaces the SparseMatrixCSC TD_OP[i] built by
 * get_TD_operator / get_discrete_Grad (src/get_TD_operator.jl:12-95, src/get_discrete_Grad.jl:16-76);
 * the shim maps set_Prop.tag[i][2] ("identity","D_x","D_y","D_z","TV") + comp_grid.n/.d to it.
 * 2-D grids: D_x = dim 1, D_z = dim 2 (pass n3 = 1); TV = [D_z; D_x] (2-D), [D_z; D_y; D_x] (3-D); TV_xy = [D_y; D_x] (3-D only). */
enum { SIPX_OP_IDENTITY = 0, SIPX_OP_DX = 1, SIPX_OP_DY = 2, SIPX_OP_DZ = 3, SIPX_OP_TV = 4,
       SIPX_OP_CSC = 5 /* a caller-supplied sparse matrix (constraint.custom_TD_OP[1], setup_constraints.jl:70-72): the
                          SparseMatrixCSC arrays in sipx_set_desc.csc_*, 0-based.  Its A'A is passed in CDS when it is banded
                          (at most 9 bands of the set, 32 of Q), or not at all: with ata_R = NULL the set becomes a MATRIX-FREE
                          TERM of Q -- no bands are kept for it and every product with Q adds rho_i A_i'(A_i p) through the
                          operator's own arrays, which is what the reference does when a set is not banded: the AtA stay
                          sparse (PARSDMM_precompute_distribute.jl:51-59) and CG runs on the sparse Q (argmin_x.jl:42-51).
                          Needs N, rows and stored entries below 2^31; not available with SIPX_Q_STENCIL, a communicator,
                          Minkowski components or sipx_warm_start_from */,
       SIPX_OP_TV_XY = 6 /* the in-plane gradient of a 3-D grid, [D_y; D_x] (no counterpart in the reference): the rows of D_y
                          first, column-major over (n1, n2-1, n3), then those of D_x over (n1-1, n2, n3), entries -+fl(1/h) as in
                          D_y / D_x; A'A has the offsets {0, +-1, +-n1}.  It takes every set SIPX_OP_TV takes in mode WHOLE, and
                          SIPX_PROJ_L21 per z-slice.  A 2-D grid refuses it (there SIPX_OP_TV is in-plane already), and so do
                          contexts with a communicator, a slab decomposition or set ownership, Minkowski components and
                          sipx_warm_start_from */ };

/* Projector descriptor replacing the opaque closure P_sub[i] (src/get_projector.jl:3-103). */
enum {
  SIPX_PROJ_BOUNDS      = 0, /* project_bounds!(x, LB, UB) scalar bounds  (projectors/project_bounds!.jl:3-12)  */
  SIPX_PROJ_BOUNDS_VEC  = 1, /* mode WHOLE: per-element bounds lb/ub TF[M_i]           (project_bounds!.jl:14-25);
                                mode FIBER: per-fiber bounds lb/ub TF[TD_n[dir]]       (project_bounds!.jl:38-88) */
  /* l1 ball, l2 ball, annulus.  mode WHOLE: the whole vector.  mode FIBER / SLICE (no counterpart in the reference; op identity,
     D_x, D_y or D_z; no transform): every fiber along dir / slice orthogonal to dir of the array of shape TD_n is projected on
     its own by the same rule; a 2-D grid has fibers only.  RADII: with lb = ub = NULL all segments take the scalar pmin / pmax.  With
     ub = TF[nseg] segment s takes pmax = ub[s]; the annulus also takes lb = TF[nseg] as pmin of each (one of the two NULL: that side keeps
     its scalar for every segment).  This needs no kind of its own: the vectors travel in lb / ub like per-fiber bounds.  Segment order:
     s = sa + SA * sb, the lower remaining dimension fastest -- for a fiber set the array of shape "TD_n without the fiber's axis"
     flattened column-major, for a slice set the coordinate along dir; nseg and this order are those of sipx_segment_norms.  An entry of
     an l1 vector that is not > 0 is refused ("Radius of L1 ball is negative") by sipx_add_set and by the host form sipx_set_data.  A vector
     that arrives from device memory (sipx_set_data_dev) cannot be checked: there a segment whose radius is not > 0 (NaN included) is set
     to zero, the projection onto the ball of radius 0 -- a rule for device-supplied radii only; the kernel ends for every value.  A
     vector whose entries are all equal gives the bits of the scalar set.  Contexts with a communicator, a slab decomposition or set
     ownership refuse vector radii (use a scalar radius, or a single process). */
  SIPX_PROJ_L1          = 2, /* project_l1_Duchi!(x, pmax)                (projectors/project_l1_Duchi!.jl:21-52); WHOLE, FIBER, SLICE */
  SIPX_PROJ_L2          = 3, /* project_l2!(x, pmax)                      (projectors/project_l2!.jl:3-16);        WHOLE, FIBER, SLICE */
  SIPX_PROJ_ANNULUS     = 4, /* project_annulus!(x, pmin, pmax)           (projectors/project_annulus!.jl:3-21);   WHOLE, FIBER, SLICE */
  SIPX_PROJ_CARDINALITY = 5, /* project_cardinality!(x, k = pmax): whole vector, per fiber or per slice
                                (projectors/project_cardinality!.jl:3-146) */
  SIPX_PROJ_PROX_L1     = 6, /* prox_l1!(x, pmax)                         (src/prox_l1!.jl:8-10) */
  SIPX_PROJ_L1_DFT      = 7, /* x -> Re(F' project_l1_Duchi!(F x, pmax)), F = unitary DFT; op must be identity
                                (src/get_projector.jl:29-35 with TD_OP "DFT", src/get_TD_operator.jl:45-47,80-82) */
  SIPX_PROJ_RANK        = 8, /* project_rank!(x, r = pmax): matrix (2-D grid, mode WHOLE) or every slice orthogonal to dir
                                (3-D, mode SLICE)   (projectors/project_rank!.jl:3-48) */
  SIPX_PROJ_NUCLEAR     = 9, /* project_nuclear!(x, sigma = pmax), same modes as RANK (projectors/project_nuclear!.jl:3-62) */
  SIPX_PROJ_HISTOGRAM   = 10,/* project_histogram_relaxed!(x, lb, ub): lb/ub ascending TF[M_i]
                                (projectors/project_histogram_relaxed.jl:9-27) */
  SIPX_PROJ_SUBSPACE    = 11,/* project_subspace!(x, A, orth): whole vector, fibers of a matrix (2-D) or slices of a
                                tensor (3-D)  (projectors/project_subspace!.jl:10-125); op must be identity */
  SIPX_PROJ_BOUNDS_DFT  = 12,/* x -> Re(F' (ub .* (F x))), F = unitary DFT: bounds in the Fourier domain with a binary lower
                                bound of zeros and a mask ub TF[N] in the transform's element order
                                (project_bounds!.jl:27-36 under get_projector.jl:8-9 with TD_OP "DFT"); op must be identity */
  SIPX_PROJ_CARD_DFT    = 13,/* x -> Re(F' project_cardinality!(F x, k = pmax)), F = unitary DFT: keep the k Fourier coefficients
                                of largest magnitude, stable order on the column-major index of the spectrum; conjugate pairs count
                                as exact ties and the lower index wins; k >= N returns x bit for bit; op must be identity, mode WHOLE
                                (src/get_projector.jl:85-89 with TD_OP "DFT", projectors/project_cardinality!.jl:3-21) */
  SIPX_PROJ_L21         = 14 /* isotropic total variation (no counterpart in the reference): the l2,1 ball
                                { v : sum_p ||v_p||_2 <= pmax } on the range of the TV operator, the group of grid point p being the
                                forward differences that start at p (0 to ndim members).  op must be SIPX_OP_TV, mode WHOLE, transform
                                NONE, pmax = tau > 0.  Group norms from a float64 sum of squares rounded once to TF, the threshold of
                                SIPX_PROJ_L1 on the N group norms, every member scaled by max(g - theta, 0) / g; an input inside the
                                ball is not written (csrc/l21.h).  Holds no replaceable vectors (sipx_set_data refuses).
                                WEIGHTS (mode WHOLE, op TV or TV_XY; SIPX_PROJ_L21_JOINT alike): lb = TF[groups] (N grid points in
                                column-major order; the joint set: n1 n2 pixels), reserved = their number, ub = NULL, makes the set
                                { v : sum_p w_p ||v_p||_2 <= pmax }: group p is shrunk by theta w_p, theta from a weighted Michelot
                                iteration of its own; w_p = 0 leaves group p unconstrained and unwritten; a weight that is negative,
                                NaN or infinite is refused by every host path and counts as 0 from device memory
                                (csrc/l21_weighted.h).  sipx_set_data(_dev) replaces the weights (lb; ub refused);
                                sipx_l21_weighted_norm observes the weighted norm.  The per-frame mode takes no weights.  Contexts
                                with a communicator, a slab decomposition or set ownership refuse it.  sipx_project takes the
                                M-vector of the TV range in the reference's row order on the context's grid; sipx_l21_norm observes
                                the norm.
                                op SIPX_OP_TV_XY (3-D grids): mode WHOLE is the same ball on the in-plane gradient (groups of 0 to 2
                                members).  Mode SLICE with dir = 2 is the ball PER FRAME, { v : sum_{p in frame k} ||v_p||_2 <= tau_k
                                for every k }, frame k the grid points (., ., k): the l1 rule of a slice set (SIPX_PROJ_L1, mode SLICE)
                                on the n1 n2 group norms of every frame, a frame inside its ball is not written (csrc/l21_seg.h).
                                Radii as for the per-segment l1 ball: ub = NULL gives every frame pmax, ub = TF[n3] frame k its own,
                                replaceable through sipx_set_data(_dev); an entry that is not > 0 is refused by every host path,
                                from device memory it zeroes a frame that is not all zero.  Other fiber / slice modes are refused:
                                frames run along z.  sipx_l21_norms observes the norms */,
  SIPX_PROJ_L21_JOINT   = 15 /* joint (vectorial) isotropic total variation across frames (no counterpart in the reference): the
                                l2,1 ball { v : sum_{(i,j)} g_ij <= pmax } on the range of SIPX_OP_TV_XY, with ONE group per pixel
                                (i, j) that spans the frames: for every k the D_y difference that starts at (i, j, k) if j < n2 - 1
                                and the D_x difference if i < n1 - 1 -- 0 to 2 n3 members, so the frames share their edges.  op must
                                be SIPX_OP_TV_XY (a 3-D grid), mode WHOLE, transform NONE, no custom operator, pmax = tau > 0
                                ("Radius of L1 ball is negative" otherwise, NaN included); any other combination is refused with
                                "the joint l2,1 ball groups the frames of TV_xy: TD_OP must be TV_xy, mode tensor".  g_ij from a
                                float64 sum of squares in a fixed order (frames ascending, D_y then D_x; the z range possibly in
                                chunks that depend on the grid and TF alone) rounded once to TF, the threshold of SIPX_PROJ_L1 on
                                the n1 n2 numbers g, every member of group (i, j) in every frame scaled by max(g - theta, 0) / g;
                                an input inside the ball is not written, -0.0 included; no floating-point atomics: two calls give
                                the same bits (csrc/l21_joint.h).  Holds no replaceable vectors (sipx_set_data refuses).  Contexts
                                with a communicator, a slab decomposition or set ownership refuse it, as they refuse the
                                operator.  sipx_project takes the M-vector of the TV_xy range in the row order of SIPX_OP_TV_XY
                                and refuses any other length with both lengths; sipx_l21_joint_norm observes the norm */,
  SIPX_PROJ_L21_GROUPS  = 16 /* group sparsity over fibers or slices (no counterpart in the reference): the l2,1 ball
                                { v = A x : sum_s w_s ||v[segment s]||_2 <= pmax } on the range of a one-block operator (op IDENTITY, DX,
                                DY or DZ), the groups being the fibers along dir (mode FIBER) or the slices orthogonal to it (mode SLICE,
                                3-D grids) of the array of shape TD_n -- nseg segments in the order of sipx_segment_norms.  Segments
                                compete for ONE budget (SIPX_PROJ_L2 per segment gives every segment its own).  pmax = tau > 0
                                ("Radius of L1 ball is negative" otherwise, NaN included).  lb = NULL (every weight 1) or TF[nseg]
                                finite weights >= 0 with reserved = nseg (0 leaves its segment unconstrained and unwritten), ub =
                                NULL.  g_s from a float64 sum of squares in a fixed order rounded once to TF (fibers: the bits of
                                sipx_segment_norms with norm 1; slices: chunks of the element index, one workgroup each), the weighted
                                Michelot threshold of the weighted SIPX_PROJ_L21 on the nseg pairs (g, w) -- exact for any active set,
                                all segments active included -- every entry of segment s scaled by max(g_s - theta w_s, 0) / g_s; an
                                input inside the ball is not written, -0.0 included; pads of the layout are neither read into a sum
                                nor written; no floating-point atomics, no state: two calls give the same bits, and no weights give the
                                bits of a vector of ones (csrc/l21_groups.h).  Mode WHOLE (one group: use SIPX_PROJ_L2), multi-block
                                and custom operators, transforms, Minkowski components and contexts with a communicator, a slab
                                decomposition or set ownership are refused, each in words of its own.  sipx_set_data(_dev) replaces
                                the weights of a set built with weights (lb, nseg entries; ub refused).  sipx_project takes the
                                M-vector of the operator's range in the reference's row order; sipx_l21_groups_norm observes the norm */,
  SIPX_PROJ_TNV         = 17 /* total nuclear variation (no counterpart in the reference): the nuclear-norm ball
                                { v : sum_{(i,j)} ||J_ij||_* <= pmax } on the range of SIPX_OP_TV_XY, J_ij the 2 x n3 matrix whose column
                                k is the (D_y, D_x) pair of pixel (i, j) in frame k -- the groups, members and pads of
                                SIPX_PROJ_L21_JOINT, whose ball is the Frobenius member of the same family; here the frames share
                                the DIRECTION of their gradients, not only where the edges are.  op must be SIPX_OP_TV_XY (a 3-D
                                grid), mode WHOLE, transform NONE, no custom operator: anything else is refused with "total nuclear
                                variation couples the frames of TV_xy: TD_OP must be TV_xy, mode tensor, no transform"; lb = ub =
                                NULL (vectors are refused with a text that names SIPX_PROJ_L21_JOINT as the weighted set); pmax =
                                tau > 0 ("Radius of L1 ball is negative" otherwise, NaN included).  Per pixel the Gram matrix
                                J J' from float64 sums in the fixed order of SIPX_PROJ_L21_JOINT (Float64: in twice the working
                                precision), its two singular values sigma1 >= sigma2 rounded once to TF and the left singular
                                vector of sigma1; the threshold of SIPX_PROJ_L1 on the 2 n1 n2 numbers sigma; every frame's pair
                                multiplied by f2 I + (f1 - f2) u1 u1', f_i = max(sigma_i - theta, 0) / sigma_i; an input inside
                                the ball is not written, -0.0 included; rows a block does not have are neither used nor written;
                                no floating-point atomics: two calls give the same bits (csrc/tnv.h).  Holds no replaceable
                                vectors.  Contexts with a communicator, a slab decomposition or set ownership refuse it, as they
                                refuse the operator.  sipx_project takes the M-vector of the TV_xy range in the row order of
                                SIPX_OP_TV_XY; sipx_tnv_norm observes the norm */,
  SIPX_PROJ_L1_WEIGHTED = 18 /* the weighted l1 ball (no counterpart in the reference): { v : sum_i w_i |v_i| <= pmax } on the rows of
                                A x, one weight per row of the operator -- the set of iteratively reweighted l1, of anisotropic TV with a
                                weight per direction, of masks.  op: IDENTITY, DX, DY, DZ, TV or TV_XY, mode WHOLE, transform NONE, no
                                component, no custom operator; each of the others is refused with a text that names the way out
                                (csrc/l1_weighted.h).  lb = TF[Mtrue] finite weights >= 0 in the reference's row order (the order of A x
                                and of y_i, l_i), reserved = Mtrue (another count is refused), ub = NULL (refused); lb = NULL: the
                                weights come with sipx_set_data(_dev) before the first solve, until then no row is constrained.  A
                                negative, NaN or infinite weight is refused, naming the first offender; from device memory it counts
                                as 0.  pmax = tau > 0 ("Radius of L1 ball is negative" otherwise, NaN included).  a_i = |v_i|; asum =
                                sum w a in twice the working precision; (TF)asum <= tau: v is not written, -0.0 included; otherwise
                                theta by the weighted Michelot iteration of SIPX_PROJ_L21's weighted form on (a, w), and y_i =
                                sign(v_i) max(a_i - theta w_i, 0) with the product rounded in TF; an entry on the threshold is zeroed,
                                a row of weight 0 is neither used nor written, whatever it holds; no floating-point atomics: two
                                calls give the same bits.  sipx_set_data(_dev) replaces the weights (lb, Mtrue entries; ub refused).
                                Contexts with a communicator, a slab decomposition or set ownership refuse it.  sipx_project takes
                                the M-vector of the operator's range in the reference's row order; sipx_l1_weighted_norm observes
                                the norm */,
  SIPX_PROJ_SIMPLEX = 19 /* simplex sets (no counterpart in the reference): every fiber (mode FIBER) or slice (mode SLICE, 3-D grids) v
                            of the array of shape TD_n has v_i >= 0 and pmin <= sum_i v_i <= pmax, 0 <= pmin <= pmax, pmax > 0, both
                            finite and shared by all segments (pmin = pmax = 1: the probability simplex, pmin = 0: the capped one) --
                            material fractions, class probabilities, frames of known mass.  op: IDENTITY, DX, DY or DZ, transform NONE,
                            no component, no custom operator, lb = ub = NULL, reserved = 0; mode WHOLE, a multi-block operator, vectors
                            and sharded contexts are refused, each with a text that names the way out (csrc/seg_simplex.h).  Per
                            segment: spos = sum max(v_i, 0) and sall = sum v_i in twice the working precision, nneg = #{v_i < 0};
                            pmin <= (TF)spos <= pmax and nneg = 0: not written, -0.0 included; nneg > 0: only the negative entries
                            are written, as +0; otherwise b = pmax if (TF)spos > pmax else pmin, theta by Michelot's fixed point
                            from (sall - b) / L over A_k = {v_i > theta_k} until the integer count repeats (theta < 0 on the lower
                            side), rounded once to TF, y_i = max(v_i - theta, +0) in TF; an all-zero segment with pmin > 0 is filled
                            with pmin / L.  No floating-point atomics, no state between calls: two calls give the same bits.  Holds
                            no replaceable vectors.  sipx_project takes the M-vector of the operator's range in the reference's row
                            order; sipx_segment_sums observes (TF)spos */,
  SIPX_PROJ_CARD_GROUPS = 20 /* group cardinality (no counterpart in the reference): { v = A x : at most k segments of v are non-zero },
                                a segment being a fiber along dir (mode FIBER) or a slice orthogonal to it (mode SLICE, 3-D grids) of the
                                array of shape TD_n, nseg segments in the order of sipx_segment_norms -- the non-convex counterpart of
                                SIPX_PROJ_L21_GROUPS ("at most k traces change", "at most k frames are active"); set ncvx = 1.  op:
                                IDENTITY, DX, DY or DZ, transform NONE, no component, no custom operator.  pmax = k, an integer >= 1
                                that, where k < nseg, is exactly representable in TF (Float32: k <= 2^24); pmin is ignored, lb = ub =
                                NULL, reserved = 0.  g_s = the l2 norm of segment s, the bits SIPX_PROJ_L21_GROUPS forms (fibers: those
                                of sipx_segment_norms with norm 1); #{g_s > 0} <= k, k >= nseg included: nothing is written, -0.0
                                included; otherwise the k first segments of the stable descending order of g (magnitude descending,
                                ties to the lower segment index) are neither read again nor written, and every entry of the others is
                                written +0.  Pads of the layout are neither read nor written; no floating-point atomics: two calls give
                                the same bits (csrc/card_groups.h).  Mode WHOLE, multi-block and custom operators, transforms, Minkowski
                                components, vectors and contexts with a communicator, a slab decomposition or set ownership are
                                refused, each with a text that names the way out.  Holds no replaceable vectors (sipx_set_data
                                refuses).  sipx_project takes the M-vector of the operator's range in the reference's row order;
                                sipx_group_norms observes g.  sipx_kernel_stats_json reports "card_groups": {calls, small,
                                search, nseg}: projections since the reset, the selections run by either route (a projection with
                                k >= nseg runs none), the segments */,
  SIPX_PROJ_L20 = 21 /* the l2,0 set on total variation, L0 gradient smoothing (no counterpart in the reference): { v = TV x : at most k
                        grid points p have a non-zero gradient vector v_p }, the group of p being that of SIPX_PROJ_L21 (the forward
                        differences that start at p); the non-convex counterpart of SIPX_PROJ_L21, set ncvx = 1.  op: TV (mode WHOLE) or
                        TV_XY (mode WHOLE: one budget over the N grid points; mode SLICE with dir = 2: every z-slice has its own budget
                        over its n1 n2 pixels), transform NONE, no component, no custom operator.  pmax = k, an integer >= 1 that, where
                        it is below the number of groups, is exactly representable in TF (Float32: k <= 2^24); per frame ub may hold
                        TF[n3] such integers instead (pmax ignored), which sipx_set_data replaces; pmin is ignored, lb = NULL,
                        reserved = 0.  g_p = the group norm SIPX_PROJ_L21 forms, bit for bit; #{g_p > 0} <= k (per frame: in that frame),
                        k >= the number of groups included: nothing is written, -0.0 included, and with one k >= the number of groups
                        not one kernel is launched; otherwise the k first groups of the stable descending order of g (magnitude
                        descending, ties to the lower point index, per frame the in-frame pixel index) are neither read again nor
                        written, and every member of the others is written +0.  Pads of the layout are neither read nor written; no
                        floating-point atomics: two calls give the same bits (csrc/l20.h).  Other operators and modes, transforms,
                        components, weights, a vector k off the per-frame form, and contexts with a communicator, a slab decomposition
                        or set ownership are refused, each with a text that names the way out.  sipx_project takes the M-vector of the
                        operator's range in the reference's row order; sipx_tv_group_norms observes g.  sipx_kernel_stats_json reports
                        "l20": {calls, small, search, frames, groups}: projections since the reset, the selections run by the two routes
                        of SIPX_PROJ_CARD_GROUPS and by the per-frame kernel, the groups of the last such set */,
  SIPX_PROJ_L20_JOINT = 22 /* the joint l2,0 set: { v = TV_xy x : at most k pixels (i, j) carry a non-zero gradient in any frame }, the
                              group of a pixel being that of SIPX_PROJ_L21_JOINT -- one common edge set for all frames; set ncvx = 1.
                              op TV_XY, mode WHOLE only.  pmax = k as above with n1 n2 groups; g from the z-march of
                              SIPX_PROJ_L21_JOINT, bit for bit; ties to the lower pixel index; the rest as SIPX_PROJ_L20 */,
  SIPX_PROJ_L21_STACKED = 23 /* the l2,1 ball across the equal-sized blocks of a caller-supplied stacked operator (csrc/l21_stacked.h):
                                { v = A x : sum_p ||v_p||_2 <= pmax }, A = [A_0; ...; A_{B-1}] given as SIPX_OP_CSC with M = B G rows,
                                B = the descriptor's `blocks` (1 .. 8, M % B == 0 or the set is refused with both numbers), the group of
                                p < G being { v[q G + p] : q < B }: every row is a member, a zero row contributes nothing.  With A the
                                Hessian of the grid (the front end's named operator "Hessian": B = 3 in 2-D, 6 in 3-D, the mixed blocks
                                scaled by sqrt 2) this is second-order isotropic TV, sum_p ||H x(p)||_F <= pmax, whose null space is the
                                affine functions.  op SIPX_OP_CSC, mode WHOLE, no transform, no component, lb = ub = NULL, reserved = 0,
                                pmax > 0; pmin is ignored; ncvx = 0.  g_p, the threshold search, the Float64 refinement and the
                                unwritten inside case are those of SIPX_PROJ_L21; no floating-point atomics: two calls give the same
                                bits.  Both forms of Q work: ata_R with up to 9 bands, or ata_R = NULL, the matrix-free term (the
                                Hessian's A'A has 13 / 25 bands: it enters matrix-free).  Contexts with a communicator, a slab
                                decomposition or set ownership are refused.  sipx_project takes the M-vector itself (len = M entries,
                                `blocks` set; op and the CSC arrays are not looked at); sipx_l21_stacked_norm observes the norm */,
  SIPX_PROJ_L2INF = 24 /* the l2,inf ball on the gradient (csrc/l2inf.h): { v = TV x : ||v_p||_2 <= c_p at every grid point p }, an isotropic
                          slope bound, the group of p being that of SIPX_PROJ_L21.  op TV or TV_XY, mode WHOLE, no transform, no component,
                          pmin = 0, lb = NULL, ncvx = 0.  c is pmax > 0 (ub = NULL, reserved = 0), or ub = TF[N] bounds >= 0 in grid-point
                          order (that of sipx_tv_group_norms) with reserved = N: +inf leaves a point free, 0 flattens it, the entry of a
                          point without a member is not looked at; sipx_set_data replaces ub in a live context.  CONTRACT: g_p is the
                          group norm SIPX_PROJ_L21 forms, bit for bit; where g_p <= c_p in TF the group keeps its bits (-0.0 included),
                          otherwise every member is multiplied by c_p / g_p, quotient and products in TF; rows a block does not have are
                          never written; no search, no state between calls, no floating-point atomics: two calls give the same bits.
                          The norm observed on the output exceeds c_p by at most 4 (Float32) or m + 4 (Float64, m members) units of
                          (eps / 2) c_p (the derivation: csrc/l2inf.h).  Contexts with a communicator, a slab decomposition or set
                          ownership are refused.  sipx_project takes the M-vector of the operator's range in the reference's row order;
                          sipx_l2inf_norm observes max_p g_p */,
  SIPX_PROJ_L2INF_JOINT = 25 /* the joint l2,inf ball: the same with the group of a pixel (i, j) that of SIPX_PROJ_L21_JOINT -- its in-plane
                                differences in all frames, g from that set's z-march bit for bit.  op TV_XY, mode WHOLE only; c is pmax or
                                ub = TF[n1 n2] in pixel order with reserved = n1 n2; the rest as SIPX_PROJ_L2INF */,
  SIPX_PROJ_L2INF_STACKED = 26 /* the l2,inf ball across the equal-sized blocks of a caller-supplied stacked operator: the groups, `blocks`
                                  and the limits of SIPX_PROJ_L21_STACKED (on the Hessian a pointwise curvature bound ||H x(p)||_F <= c_p).
                                  op SIPX_OP_CSC, mode WHOLE; c is pmax or ub = TF[G], G = M / blocks, with reserved = G; the rest as
                                  SIPX_PROJ_L2INF.  sipx_project takes the M-vector itself (len = M entries, `blocks` set; op and the CSC
                                  arrays are not looked at) */
};
/* constraint.app_mode (set_definitions): ("matrix"|"tensor", _) = WHOLE, ("fiber", d), ("slice", d).
 * dir is the 0-based array dimension: "x" = 0, "y" = 1, "z" = 2 on a 3-D grid, "z" = 1 on a 2-D grid. */
enum { SIPX_MODE_WHOLE = 0, SIPX_MODE_FIBER = 1, SIPX_MODE_SLICE = 2 };
/* SIPX_TRANSFORM_WAVELET: TD_OP = "wavelet", joDWT(n1, n2, wavelet(WT.db4); L = maxtransformlevels(min(n)))
 * (src/get_TD_operator.jl:86-88; the reference has no 3-D wavelet, get_TD_operator.jl:53-54 -- here the same transform on all three
 * dimensions).  Orthonormal, periodic, separable, multilevel, db4 (8 taps), lo = the db4 decomposition low-pass (sum sqrt(2)),
 * hi[j] = (-1)^(j+1) lo[7-j].  One level along an axis of length m:
 *     a[k] = sum_j lo[j] x[(2k + 4 - j) mod m],   d[k] = sum_j hi[j] x[(2k + 4 - j) mod m],   k = 0 .. m/2-1,
 * a to positions [0, m/2), d to [m/2, m) of that axis.  L = the largest integer with 2^L dividing min(n) (over all dimensions of
 * the grid); level l transforms every axis of the box n / 2^(l-1), in place (Mallat layout: pywt.coeffs_to_array of
 * pywt.wavedecn(x, "db4", mode="periodization")).  L = 0: the identity.  A grid with a dimension not divisible by 2^L is
 * refused.  CAVEAT: the subsampling phase of Wavelets.jl (the "+4" above) is not pinned by any reference test; the l2 ball and the
 * annulus do not depend on it, the l1 ball, cardinality and scalar bounds do (the precedent of the DCT's assumed normalisation). */
enum { SIPX_TRANSFORM_NONE = 0, SIPX_TRANSFORM_DCT = 1, SIPX_TRANSFORM_WAVELET = 2 };

typedef struct {
  int32_t op;        /* SIPX_OP_*   */
  int32_t proj;      /* SIPX_PROJ_* */
  double pmin, pmax; /* constraint[i].min / .max (set_definitions, src/SetIntersectionProjection.jl:142-149) */
  const void* lb;    /* BOUNDS_VEC / HISTOGRAM: host TF vectors (see the kinds above); L1 / L2 / ANNULUS in mode FIBER / SLICE: NULL or
                        the radii per segment, TF[nseg]; L21 in mode WHOLE / L21_JOINT / L21_GROUPS: NULL or one weight per group
                        (lb alone, and `reserved` holds their number); L1_WEIGHTED: one weight per row of the operator (lb alone,
                        `reserved` holds their number); else NULL */
  const void* ub;
  int32_t ncvx;      /* set_Prop.ncvx[i] (src/setup_constraints.jl:89-97) */
  int32_t reserved;  /* 0; a weighted L21 / L21_JOINT / L21_GROUPS set: the entries of lb, refused unless it is the group count;
                        L1_WEIGHTED: the rows of the operator (Mtrue), refused otherwise; the L2INF kinds with ub: the entries of ub,
                        refused unless it is the group count */
  int32_t mode;      /* SIPX_MODE_* */
  int32_t dir;       /* direction of the fibers / normal of the slices */
  const void* basis; /* SUBSPACE: host TF[basis_rows x basis_cols], column-major (constraint.custom_TD_OP[1]) */
  int64_t basis_rows;
  int32_t basis_cols;
  int32_t basis_orth;/* constraint.custom_TD_OP[2]: A'A = I */
  int32_t component; /* Minkowski sets (src/PARSDMM_precompute_distribute_Minkowski.jl:6-173): 0 = ordinary set; 1 = the set
                        constrains the first component u (TD_OP = [A 0]); 2 = the second component v ([0 A]); 3 = their sum
                        u + v ([A A]).  Either every set of a context names a component or none does.  With components the
                        unknown is x = [u; v] (2N entries in x0 / sipx_download / sipx_apply_Q), the distance term is
                        1/2 ||u + v - m||^2, and Q is the 2N x 2N CDS matrix of the reference. */
  const int64_t* csc_colptr; /* SIPX_OP_CSC: colptr[N+1], rowval[nnz] (0-based, ascending inside a column), nzval TF[nnz] */
  const int64_t* csc_rowval;
  const void* csc_nzval;
  int64_t csc_rows;          /* rows of the matrix = length of y_i, l_i */
  int32_t transform; /* SIPX_TRANSFORM_*: an orthogonal transform folded into the projector, x -> A' P(A x) with TD_OP = I
                        (src/get_projector.jl: the branches `constraint.TD_OP in special_operator_list`,
                        src/setup_constraints.jl:54,76-80).  DCT = orthonormal DCT-II along every grid dimension; proj must be
                        BOUNDS, BOUNDS_VEC, L1 or CARDINALITY (mode WHOLE), op the identity.  WAVELET = the db4 transform above;
                        proj must be BOUNDS (scalar), L1 or CARDINALITY (mode WHOLE), op the identity.  The DFT has its own kinds above. */
  int32_t pad_;
  int32_t blocks;    /* SIPX_PROJ_L21_STACKED: B, the number of equal-sized blocks of the stacked operator (1 .. 8); 0 for every other
                        kind.  Appended behind the older fields: a descriptor zero-initialised by a caller that does not know the
                        field configures every older kind as before */
  int32_t pad2_;
} sipx_set_desc;

/* PARSDMM_options (src/SetIntersectionProjection.jl:110-128); Blas_active / parallel / FL /
 * x_min_solver / Minkowski have no native meaning (FL = dtype of the context). */
typedef struct {
  int32_t maxit;
  double evol_rel_tol, feas_tol, obj_tol;
  int32_t rho_update_frequency;
  int32_t adjust_rho, adjust_gamma, adjust_feasibility_rho;
} sipx_options;

/* log_type_PARSDMM (src/SetIntersectionProjection.jl:95-108) as flat row-major arrays the caller
 * allocates for `maxit` rows; the executed row counts come back in n_iter / n_feas_rows
 * (output_check_PARSDMM truncation, src/PARSDMM.jl:261-278). */
typedef struct {
  double* set_feasibility; /* [maxit][pp] */
  double* r_dual;          /* [maxit][p]  */
  double* r_pri;           /* [maxit][p]  */
  double* r_dual_total;    /* [maxit] */
  double* r_pri_total;     /* [maxit] */
  double* obj;             /* [maxit] */
  double* evol_x;          /* [maxit] */
  double* rho;             /* [maxit][p] */
  double* gamma;           /* [maxit][p] */
  int64_t* cg_it;          /* [maxit] */
  double* cg_relres;       /* [maxit] */
  double timing_ms[7];     /* the 7 @timeit sections of src/PARSDMM.jl:40,100,105,113,152,163,229 */
  int32_t n_iter;          /* rows filled in the per-iteration logs */
  int32_t n_feas_rows;     /* rows kept in set_feasibility (= `counter`) */
  int32_t stopped_feasible;/* 1 if the input was accepted as feasible (src/PARSDMM.jl:63-82) */
} sipx_log;

const char* sipx_last_error(void);

/* ---- construction (replaces the allocations of PARSDMM_initialize, src/PARSDMM_initialize.jl:117-184) ---- */
int sipx_create(sipx_ctx** out, int dtype, int ndim, const int64_t* n, const double* h, int device);
void sipx_destroy(sipx_ctx* ctx);

/* Adds constraint set i (call in TD_OP order).  ata_R / ata_off / d_i = AtA[i] in CDS (N x d_i,
 * column-major) with set_Prop.AtA_offsets[i] (src/PARSDMM_precompute_distribute.jl:52-59); pass
 * ata_R = NULL to have the bands generated on the device from the operator descriptor.
 * For SIPX_OP_CSC there is no descriptor to generate bands from: ata_R = NULL makes the set a matrix-free term of Q
 * (the reference's sparse Q of a set that is not banded, PARSDMM_precompute_distribute.jl:51-59, argmin_x.jl:42-51; see
 * SIPX_OP_CSC).  sipx_q_terms tells how a finalized context holds Q.
 * RETURN VALUE (unlike every other entry): the 0-based index of the new set (the i of y_i / l_i, of the rho / gamma /
 * r_pri arrays and of sipx_set_rows) on success, -1 on error -- test `rc < 0`, not `rc != 0`. */
int sipx_add_set(sipx_ctx* ctx, const sipx_set_desc* desc, const void* ata_R, const int64_t* ata_off, int d_i);

/* Rows of A_i (length of y_i / l_i) for set i; i = number of constraint sets addresses the
 * distance term appended by PARSDMM_precompute_distribute (src/PARSDMM_precompute_distribute.jl:17-26). */
int sipx_set_rows(sipx_ctx* ctx, int set, int64_t* rows);
int sipx_num_terms(sipx_ctx* ctx, int* p, int* pp);

/* Uploads m, initial rho/gamma, optional warm start (x0, l0[i], y0[i]; NULL = zeros; ignored when
 * zero_ini_guess != 0, src/PARSDMM_initialize.jl:304-313); appends the distance term unless
 * feasibility_only; assembles Q / Q_offsets (src/PARSDMM_initialize.jl:216-230); fills
 * feasibility_initial[pp] (src/PARSDMM_initialize.jl:97-99). */
int sipx_finalize(sipx_ctx* ctx, const void* m, const double* rho_ini, int n_rho, double gamma_ini,
                  int feasibility_only, int zero_ini_guess, const void* x0, const void* const* l0,
                  const void* const* y0, double* feasibility_initial);

/* The same sets on the same grid, once more: a new model m (and, optionally, another warm start and rho_ini) on a context that
 * has been finalised -- and, usually, solved -- before.  This is how the reference's callers use this entry point: PARSDMM wrapped
 * as a projector and called again and again inside an outer loop (examples/constrained_freq_FWI_simple.jl:468,
 * examples/Constraint_examples_2D.jl:222-223, examples/Dykstra_parallel_vs_PARSDMM.jl:134); every such call of the reference runs
 * PARSDMM_initialize again (src/PARSDMM.jl:58-61).  Here nothing is allocated and no plan, handle, stream or event is created:
 * every array is zero-filled, m uploaded, rho / gamma set as sipx_finalize sets them, Q assembled again (the solve updated it
 * incrementally, src/Q_update!.jl:45-48), every warm start inside the context forgotten, feasibility_initial[pp] taken again
 * (src/PARSDMM_initialize.jl:97-99).  The context is then in the state sipx_finalize leaves it in: a solve on it returns the bits a
 * newly built context returns.  Arguments as for sipx_finalize (feasibility_only stays what it was).  Not available for a rank of a
 * sharded solve. */
int sipx_reset(sipx_ctx* ctx, const void* m, const double* rho_ini, int n_rho, double gamma_ini, int zero_ini_guess,
               const void* x0, const void* const* l0, const void* const* y0, double* feasibility_initial);

/* ---- A. phase level ---- */
/* rhs = sum_i A_i'(rho_i y_i + l_i)                                   (src/rhs_compose.jl:24-36) */
int sipx_rhs_compose(sipx_ctx* ctx, const double* rho);
/* copy!(x_old,x); tolerance rule; warm-started CG on Q x = rhs        (src/PARSDMM.jl:106-107, src/argmin_x.jl:23-39, src/cg.jl:44-128) */
int sipx_argmin_x(sipx_ctx* ctx, int it, double* tol_ref_io, int64_t* cg_it, double* cg_relres, int* cg_flag);
/* y/l update for every local set                                       (src/update_y_l.jl:36-101) */
enum { SIPX_YL_FEAS = 1,  /* also log set feasibility (mod(i,10)==0)            update_y_l.jl:90-99 */
       SIPX_YL_BB = 2,    /* also accumulate the six BB sums and refresh snapshots  adapt_rho_gamma.jl:41-53, PARSDMM.jl:192-206 */
       SIPX_YL_FIRST = 4  /* first iteration: set snapshots                    PARSDMM.jl:164-180 */ };
int sipx_update_y_l(sipx_ctx* ctx, int it, int flags, const double* rho, const double* gamma,
                    double* r_pri, double* r_dual, double* feas /* [pp], written iff SIPX_YL_FEAS */);
/* obj = 1/2||x-m||^2, evol_x = ||x_old-x||/||x||                      (src/PARSDMM.jl:140,145) */
int sipx_log_scalars(sipx_ctx* ctx, double* obj, double* evol_x);
/* Barzilai-Borwein rule from the sums gathered by the last sipx_update_y_l(SIPX_YL_BB)  (src/adapt_rho_gamma.jl:55-126) */
int sipx_adapt_rho_gamma(sipx_ctx* ctx, int adjust_rho, int adjust_gamma, double* rho_io, double* gamma_io);
/* Q += (rho_new - rho_old) AtA_i for changed sets; rebinds the distance prox  (src/Q_update!.jl:45-48, src/PARSDMM.jl:230-243).
 * A matrix-free term has no bands to update: its rho_i is replaced by rho_new[i]. */
int sipx_q_update(sipx_ctx* ctx, const double* rho_new, const double* rho_old);
/* copy out x, l[i], y[i] (any pointer may be NULL)                     (src/PARSDMM.jl:257) */
int sipx_download(sipx_ctx* ctx, void* x, void* const* l, void* const* y);

/* ---- the same boundary for data that lives on the GPU ----
 * The reference's callers use PARSDMM as a projector inside a loop whose data is already on the device (an FWI iterate per gradient
 * step, examples/constrained_freq_FWI_simple.jl:468; the output of a network per training step,
 * examples/GeneralizedMinkowski/ConstrainedNeuralNetworkSegmentation_*.jl).  sipx_finalize_dev / sipx_reset_dev / sipx_download_dev
 * are sipx_finalize / sipx_reset / sipx_download with every VECTOR argument -- m, x0, l0[i], y0[i], x, l[i], y[i] -- a pointer to
 * device memory on the context's GPU (the pointer arrays l0 / y0 / l / y themselves, rho_ini and feasibility_initial stay host
 * memory); same lengths, same row order, same meaning, and the context is left in the same state: a solve gives the same bits
 * whichever form started it, and the two forms may be mixed on one context.  No vector crosses PCIe, nothing is allocated, and one
 * launch moves all vectors of a call between the caller's buffers and the padded arrays of the context.
 * ORDERING.  The engine works on streams of its own.  sipx_set_caller_stream names the stream the caller produces m (and the warm
 * start) on and consumes the results on (a hipStream_t; NULL, the default, is the default stream); it holds until changed.
 *   - The import of _finalize_dev / _reset_dev waits, on the device, for an event recorded on the caller's stream when the call is
 *     made: work queued there before the call is seen.  Both calls end with the host wait of the initial feasibility, as their
 *     host forms do; when they return the caller's input buffers have been read and may be reused.
 *   - sipx_download_dev first lets the engine wait for the caller's stream (so that work still reading the result buffers
 *     finishes first), writes the results on the engine stream, records an event there and makes the caller's stream wait for
 *     it.  It returns without waiting on the host: the results are valid for work queued on the caller's stream after the call
 *     (for the host: after synchronising that stream).
 * Single-process contexts only: with a communicator attached, a slab decomposition requested or set ownership given, the three
 * calls fail with a message (use the host forms there).  Every set kind, both precisions, Minkowski contexts (x of length 2N)
 * and feasibility_only are taken. */
int sipx_set_caller_stream(sipx_ctx* ctx, void* stream);
int sipx_finalize_dev(sipx_ctx* ctx, const void* m, const double* rho_ini, int n_rho, double gamma_ini, int feasibility_only,
                      int zero_ini_guess, const void* x0, const void* const* l0, const void* const* y0,
                      double* feasibility_initial);
int sipx_reset_dev(sipx_ctx* ctx, const void* m, const double* rho_ini, int n_rho, double gamma_ini, int zero_ini_guess,
                   const void* x0, const void* const* l0, const void* const* y0, double* feasibility_initial);
int sipx_download_dev(sipx_ctx* ctx, void* x, void* const* l, void* const* y);

/* ---- new vectors for a set of a context that stays alive ----
 * The reference's application examples learn their constraints once, build one list of sets and project many images through it;
 * the last set is a data-fit box LBD <= A x <= UBD around the current image and between images only that projector is replaced:
 * P_sub[end] = x -> project_bounds!(x, LBD, UBD) (examples/Indonesia_desaturation/image_desaturation_by_constraint_learning.jl:264,
 * examples/Ecuador_denoising_deblurring_inpainting/denoising_deblurring_inpainting_by_constraint_learning_SA.jl:302).
 * sipx_set_data replaces lb / ub of set `set` (the index sipx_add_set returned) by host TF vectors, sipx_set_data_dev by TF vectors
 * in device memory of the context's GPU; a NULL pointer keeps that vector.  Lengths, order and meaning are those of sipx_add_set:
 *   SIPX_PROJ_BOUNDS_VEC, transform NONE, mode WHOLE:  TF[M_i] in the reference's row order
 *   SIPX_PROJ_BOUNDS_VEC, transform NONE, mode FIBER:  TF[TD_n[dir]]
 *   SIPX_PROJ_HISTOGRAM:                               TF[M_i], ascending (unchecked, as in sipx_add_set)
 *   SIPX_PROJ_L1 / L2 / ANNULUS, mode FIBER / SLICE, built with a vector of radii:  TF[nseg]; ub = the radii (pmax of each segment),
 *                                                      lb = the annulus' inner radii (refused for l1 / l2).  One copy per vector on the
 *                                                      set's stream into the arrays the projector was built with.  The host form refuses
 *                                                      an l1 radius that is not > 0; for the device form see SIPX_PROJ_L1.  A set built
 *                                                      with scalars holds no replaceable vectors.
 * behind every operator sipx_add_set takes for these kinds (SIPX_OP_CSC with banded or matrix-free A'A included; per-fiber bounds
 * need a built-in operator).
 * REFUSED, with a message that names the way out (build a new context): every other kind -- scalars, vector bounds behind the DCT,
 * the DFT mask, subspace bases --, the distance term, an index out of range, and a context with a communicator, a slab
 * decomposition, set ownership or Minkowski components.  A refused call changes nothing.
 * WHEN.  From the moment sipx_add_set returned the index.  Before sipx_finalize(_dev) the call replaces what sipx_add_set was given
 * and finalize uses the latest data, so a first build can take its vectors from device memory (sipx_add_set still wants lb and ub:
 * placeholders of the right length will do).  On a finalized context the device arrays are overwritten in place: nothing is
 * allocated, no handle, plan, stream or event is created.
 * CONTRACT.  sipx_set_data* followed by sipx_reset(_dev) leaves the context in the state sipx_finalize leaves a new context built
 * with that data; the solve that follows returns the same bits.  (Without the reset the state of a solve in progress is undefined:
 * the host form stages through scratch of the engine.)
 * BYTES.  The host form on a finalized context adds the vectors it was given to the host-to-device count of sipx_io_bytes (before
 * sipx_finalize the upload, and its count, are finalize's); the device form adds nothing.
 * ORDERING of the device form: as for sipx_reset_dev / sipx_download_dev.  The engine stream waits for an event recorded on the
 * caller's stream (sipx_set_caller_stream) when the call is made, so work queued there before the call is seen; after the transfer
 * it records an event the caller's stream waits for, so work queued there afterwards may overwrite the buffers.  The host waits
 * for nothing.  The host form returns when the caller's arrays have been read.
 * Both vectors of a call move in one launch of the transfer kernel of the device-resident calls: a whole-mode vector through one
 * unpack segment per operator block, per-fiber bounds through a broadcast segment (the padded entry of a row takes the bound of its
 * coordinate along dir) -- bit for bit what sipx_add_set's expansion on the host gives. */
int sipx_set_data(sipx_ctx* ctx, int set, const void* lb, const void* ub);
int sipx_set_data_dev(sipx_ctx* ctx, int set, const void* lb, const void* ub);
/* Bytes of the N-sized transfers between host and device that sipx_finalize, sipx_reset and sipx_download (and their _dev forms)
 * have made on this context since it was created or since the last call with reset != 0: m, x, l_i, y_i, bound vectors and
 * explicit A'A bands, and what sipx_set_data uploads.  The _dev forms add nothing for m, x, l_i, y_i, sipx_set_data_dev nothing
 * at all.  Either pointer may be NULL. */
int sipx_io_bytes(sipx_ctx* ctx, int64_t* host_to_device, int64_t* device_to_host, int reset);

/* Multilevel (src/PARSDMM_multi_level.jl:61-83, src/interpolate_y_l.jl:16-94): warm start of a finalized context on a finer
 * grid from a solved context on a coarser one, DEVICE TO DEVICE -- x, every l_i and y_i are resampled (nearest neighbour,
 * the set-by-set block arithmetic of interpolate_y_l) without visiting the host.  Both contexts hold the same sets, in the
 * same precision, on the same device.  Overwrites whatever start sipx_finalize gave the fine context.  Ranks of a sharded
 * solve: both contexts slab-decomposed (sipx_set_decomp); the call is then a collective -- the coarse slabs are all-gathered on
 * the device and every rank resamples the whole iterate. */
int sipx_warm_start_from(sipx_ctx* fine, sipx_ctx* coarse);

/* ---- B. whole solve (src/PARSDMM.jl:97-257 restated natively) ---- */
int sipx_parsdmm(sipx_ctx* ctx, const sipx_options* opt, sipx_log* log);
/* the same solve advanced in pieces: begin, then up to nsteps iterations per call (done = 1 once a stop rule or maxit
 * ended it; the log arrays given to _begin must stay alive) */
int sipx_parsdmm_begin(sipx_ctx* ctx, const sipx_options* opt, sipx_log* log);
int sipx_parsdmm_steps(sipx_ctx* ctx, int nsteps, int* done);

/* ---- kernel-level entry points used by the parity tests and bench (same kernels as above) ---- */
/* y = R x for an arbitrary CDS matrix (CDS_MVp_MT + fill!, src/CDS_MVp_MT.jl:9-25, src/argmin_x.jl:72-78) */
int sipx_cds_spmv(int dtype, int64_t N, int d, const void* R, const int64_t* off, const void* x, void* y, int device);
/* s = A x (op descriptor) and t = A' v on the context grid */
int sipx_apply_op(sipx_ctx* ctx, int op, const void* x, void* s);
int sipx_apply_op_adj(sipx_ctx* ctx, int op, const void* v, void* t);
/* in-place projector on a host vector of length len (src/projectors/project_X.jl) */
int sipx_project(sipx_ctx* ctx, const sipx_set_desc* desc, void* v, int64_t len);
/* The norms of the fibers / slices of A x: out[s] = ||segment s of A x||_1 (norm = 0) or _2 (norm = 1), TF[nseg], for op = identity, D_x,
 * D_y or D_z, mode = SIPX_MODE_FIBER / SLICE and dir as in sipx_set_desc, on the 2-D or 3-D grid of the context (which needs no sets and no
 * finalize).  nseg and the order of the segments are those of the per-segment radii (SIPX_PROJ_L1): what this call returns can be
 * passed as ub / lb of such a set.  *nseg receives the count (may be NULL); with x = NULL or out = NULL only the count is returned.  The
 * operator / mode combinations the sets refuse are refused here with the same messages.  A x comes from the engine's operator product
 * into scratch of the call; one kernel then reads it once, with the tile mapping and the first-pass reduction of the projector -- float64
 * sums in a fixed order, rounded to TF once, sqrt in float64 for l2.  CONTRACT: the numbers are the ones the projector compares with
 * its radii, so radii observed on x make A x a point the projector does not write (l1, l2, annulus with lb = ub = observed); an all-zero
 * segment gives exactly 0 (as an l1 radius that is refused: give such a segment any positive radius).  x, out: host memory; the _dev
 * form takes both in device memory of the context's GPU, ordered like sipx_download_dev against the caller's stream (sipx_set_caller_stream),
 * and nothing crosses PCIe.  Learning from several arrays is a loop with an element-wise maximum / minimum over the results. */
int sipx_segment_norms(sipx_ctx* ctx, int op, int mode, int dir, int norm, const void* x, void* out, int64_t* nseg);
int sipx_segment_norms_dev(sipx_ctx* ctx, int op, int mode, int dir, int norm, const void* x, void* out, int64_t* nseg);
/* The sums of the positive parts of the fibers / slices of A x: out[s] = (TF) sum_i max((A x)_i, 0) over segment s, TF[nseg], arguments,
 * count, order, queries and the _dev form as sipx_segment_norms.  Summed in twice the working precision by pass 1 of the
 * SIPX_PROJ_SIMPLEX projector on (op, mode, dir), by the route that projector takes there (csrc/seg_simplex.h).  CONTRACT: the numbers
 * are the very ones that projector compares with pmin and pmax, so a nonnegative A x is not written by a set built with pmin = the
 * smallest and pmax = the largest of them.  Refused where the set is refused. */
int sipx_segment_sums(sipx_ctx* ctx, int op, int mode, int dir, const void* x, void* out, int64_t* nseg);
int sipx_segment_sums_dev(sipx_ctx* ctx, int op, int mode, int dir, const void* x, void* out, int64_t* nseg);
/* The l2 norms of the fibers / slices of A x as SIPX_PROJ_CARD_GROUPS selects on them: out[s] = g_s, TF[nseg], arguments, count, order,
 * queries and the _dev form as sipx_segment_norms.  Formed by the norms launch of that projector on (op, mode, dir)
 * (csrc/card_groups.h) -- fibers: the bits of sipx_segment_norms with norm 1; slices: chunked compensated sums, within one unit of TF of
 * the exactly summed norm.  CONTRACT: the array is the selection key itself: the projector keeps the first k segments of its stable
 * descending order, and the count it compares with k is the number of non-zero entries of out.  Refused where the set is refused. */
int sipx_group_norms(sipx_ctx* ctx, int op, int mode, int dir, const void* x, void* out, int64_t* nseg);
int sipx_group_norms_dev(sipx_ctx* ctx, int op, int mode, int dir, const void* x, void* out, int64_t* nseg);
/* A hook of the tests and of tools/card_groups_bench.py, not for applications: the selection route of the SIPX_PROJ_CARD_GROUPS projectors
 * built from now on in this process.  0: by the number of segments (the default), 1: the one-workgroup rank count (refused for more than
 * CARDG_SMALL_MAX segments), 2: the engine's cardinality search.  Both routes give the same bits. */
int sipx_card_groups_route(int route);
/* The norms of the gradient groups of A x as SIPX_PROJ_L20 (joint = 0) or SIPX_PROJ_L20_JOINT (joint != 0) selects on them: out[p] = g_p,
 * TF[*ngroups]; op TV or TV_XY (joint: TV_XY); ngroups = N in point order, joint: n1 n2 in pixel order (the per-frame set selects on the
 * same N numbers as the whole-array set, frame by frame); x TF[N]; x = out = NULL asks for *ngroups alone.  Formed by the norms launch of
 * that projector (csrc/l20.h), which is the one of SIPX_PROJ_L21 / SIPX_PROJ_L21_JOINT.  CONTRACT: the array is the selection key itself:
 * the projector keeps the first k groups of its stable descending order, and the count it compares with k is the number of non-zero
 * entries of out.  The _dev form takes device pointers, ordered against the caller's stream.  Refused where the set is refused. */
int sipx_tv_group_norms(sipx_ctx* ctx, int op, int joint, const void* x, void* out, int64_t* ngroups);
int sipx_tv_group_norms_dev(sipx_ctx* ctx, int op, int joint, const void* x, void* out, int64_t* ngroups);
/* The isotropic total variation of x: *out = ||TV x||_2,1 as one TF, x TF[N] on the 2-D or 3-D grid of the context (which needs no sets
 * and no finalize).  TV x comes from the engine's operator product into scratch of the call; the group norms are formed by the kernel of
 * SIPX_PROJ_L21 and summed by the first pass of its threshold search.  CONTRACT: the value is the very number the projector compares
 * with pmax, so a radius observed on x makes TV x a point the projector does not write.  x, out: host memory; the _dev form takes both
 * in device memory of the context's GPU, ordered like sipx_download_dev against the caller's stream. */
int sipx_l21_norm(sipx_ctx* ctx, const void* x, void* out);
int sipx_l21_norm_dev(sipx_ctx* ctx, const void* x, void* out);
/* The same behind an operator and per application mode of SIPX_PROJ_L21: op SIPX_OP_TV or SIPX_OP_TV_XY with mode WHOLE writes one TF,
 * op SIPX_OP_TV_XY with mode SLICE, dir = 2 writes the n3 numbers (TF)asum_k, the sums of the group norms of every frame -- the very
 * values the per-frame projector compares with its radii, so radii observed on x leave [D_y; D_x] x unwritten.  *nseg (if not NULL)
 * receives the number of values; x = out = NULL only asks for it.  Every other combination is refused as sipx_add_set refuses it. */
int sipx_l21_norms(sipx_ctx* ctx, int op, int mode, int dir, const void* x, void* out, int64_t* nseg);
int sipx_l21_norms_dev(sipx_ctx* ctx, int op, int mode, int dir, const void* x, void* out, int64_t* nseg);
/* The norm SIPX_PROJ_L21_STACKED compares with pmax: *out = one TF, the sum over p < G of the group norms of A x, A the SIPX_OP_CSC
 * operator of the descriptor d (op, csc_* and blocks are read; proj may be left 0), x TF[N] on the grid of the context (which needs no
 * sets and no finalize).  A x comes from the engine's sparse product into scratch of the call, the group norms from the kernel of the
 * projector, the sum from the first pass of its threshold search.  CONTRACT: the value is the very number the projector compares with
 * pmax, so a radius observed on x leaves A x unwritten.  x, out: host memory; the _dev form takes both in device memory of the
 * context's GPU, ordered like sipx_l21_norm_dev against the caller's stream.  Refused where the set is refused. */
int sipx_l21_stacked_norm(sipx_ctx* ctx, const sipx_set_desc* d, const void* x, void* out);
int sipx_l21_stacked_norm_dev(sipx_ctx* ctx, const sipx_set_desc* d, const void* x, void* out);
/* The largest group norm of the SIPX_PROJ_L2INF kinds: *out = one TF, max_p g_p of A x, x TF[N] on the grid of the context (which needs no
 * sets and no finalize).  The descriptor d names the set: proj SIPX_PROJ_L2INF with op TV or TV_XY, SIPX_PROJ_L2INF_JOINT with op TV_XY, or
 * SIPX_PROJ_L2INF_STACKED with op SIPX_OP_CSC, its csc_* arrays and blocks; pmin, pmax, lb, ub and reserved are not looked at.  The norms
 * come from the norms launch of the projector (the arithmetic of its clip kernels), the maximum from a two-stage reduction in a fixed
 * order.  CONTRACT: a set built with the value as its scalar bound leaves A x unwritten.  x, out: host memory; the _dev form takes both
 * in device memory of the context's GPU, ordered like sipx_l21_norm_dev against the caller's stream.  Refused where the set is refused. */
int sipx_l2inf_norm(sipx_ctx* ctx, const sipx_set_desc* d, const void* x, void* out);
int sipx_l2inf_norm_dev(sipx_ctx* ctx, const sipx_set_desc* d, const void* x, void* out);
/* The joint total variation of the frames of x: *out = one TF, the sum over the pixels (i, j) of the group norms g_ij of SIPX_PROJ_L21_JOINT
 * on [D_y; D_x] x, x TF[N] on the 3-D grid of the context.  The norms come from the z-march of the projector, the sum from the first
 * pass of its threshold search.  CONTRACT: the value is the very number the projector compares with pmax, so a radius observed on x
 * leaves [D_y; D_x] x unwritten.  x, out: host memory; the _dev form takes both in device memory of the context's GPU, ordered like
 * sipx_l21_norm_dev against the caller's stream.  Refused where the set is refused (2-D grids, sharded contexts). */
int sipx_l21_joint_norm(sipx_ctx* ctx, const void* x, void* out);
int sipx_l21_joint_norm_dev(sipx_ctx* ctx, const void* x, void* out);
/* The total nuclear variation of the frames of x: *out = one TF, the sum over the pixels of the two singular values of SIPX_PROJ_TNV on
 * [D_y; D_x] x, x TF[N] on the 3-D grid of the context: the Gram march and the decomposition of the projector, the sum from the first
 * pass of its threshold search.  CONTRACT: the value is the very number the projector compares with pmax, so a radius observed on x
 * leaves [D_y; D_x] x unwritten.  x, out: host memory; the _dev form takes both in device memory of the context's GPU, ordered like
 * sipx_l21_norm_dev against the caller's stream.  Refused where the set is refused (2-D grids, sharded contexts). */
int sipx_tnv_norm(sipx_ctx* ctx, const void* x, void* out);
int sipx_tnv_norm_dev(sipx_ctx* ctx, const void* x, void* out);
/* The weighted total variation of x: *out = one TF, (TF) sum_p w_p g_p over the groups of SIPX_PROJ_L21 behind op (SIPX_OP_TV or
 * SIPX_OP_TV_XY; joint = 0, w TF[N] in the grid's column-major point order) or of SIPX_PROJ_L21_JOINT (joint != 0, op SIPX_OP_TV_XY, w
 * TF[n1 n2] in pixel order), summed by the first pass of the weighted projector (csrc/l21_weighted.h).  CONTRACT: the value is the
 * very number that projector compares with pmax, so a radius observed on x leaves A x unwritten.  x, w, out: host memory, a weight
 * that is negative, NaN or infinite is refused; the _dev form takes all three in device memory of the context's GPU, ordered like
 * sipx_l21_norm_dev against the caller's stream, and there such a weight counts as 0.  Refused where the set is refused. */
int sipx_l21_weighted_norm(sipx_ctx* ctx, int op, int joint, const void* x, const void* w, void* out);
int sipx_l21_weighted_norm_dev(sipx_ctx* ctx, int op, int joint, const void* x, const void* w, void* out);
/* The group norm of x over fibers or slices: *out = one TF, (TF) sum_s w_s g_s over the segments of SIPX_PROJ_L21_GROUPS behind op
 * (IDENTITY, DX, DY, DZ) with (mode, dir); w = TF[nseg] in the order of sipx_segment_norms, or NULL: every weight 1.  Summed by the norms
 * launch and the first pass of the projector (csrc/l21_groups.h).  CONTRACT: the value is the very number the projector compares with
 * pmax, so a set built with pmax = *out leaves A x unwritten.  A negative, NaN or infinite weight is refused on the host path; _dev: x,
 * w and out device pointers, ordered like sipx_l21_norm_dev against the caller's stream, and there such a weight counts as 0.  Refused
 * where the set is refused. */
int sipx_l21_groups_norm(sipx_ctx* ctx, int op, int mode, int dir, const void* x, const void* w, void* out);
int sipx_l21_groups_norm_dev(sipx_ctx* ctx, int op, int mode, int dir, const void* x, const void* w, void* out);
/* The weighted l1 norm of A x: *out = one TF, (TF) sum_i w_i |(A x)_i| over the rows of op (IDENTITY, DX, DY, DZ, TV, TV_XY), w TF[Mtrue]
 * in the reference's row order, summed by the first pass of the SIPX_PROJ_L1_WEIGHTED projector (csrc/l1_weighted.h).  CONTRACT: the value
 * is the very number that projector compares with pmax, so a radius observed on x leaves A x unwritten.  x, w, out: host memory, a
 * weight that is negative, NaN or infinite is refused; the _dev form takes all three in device memory of the context's GPU, ordered like
 * sipx_l21_norm_dev against the caller's stream, and there such a weight counts as 0.  Refused where the set is refused. */
int sipx_l1_weighted_norm(sipx_ctx* ctx, int op, const void* x, const void* w, void* out);
int sipx_l1_weighted_norm_dev(sipx_ctx* ctx, int op, const void* x, const void* w, void* out);
/* nearest-neighbour resampling of an array of shape nc to shape nf, the grid transfer of PARSDMM_multi_level:
 * out[k] = in[round(1 + (k-1)(nc-1)/(nf-1))] per axis (Interpolations.BSpline(Constant()) evaluated on
 * range(1, stop=nc, length=nf); src/PARSDMM_multi_level.jl:41-45,61-65, src/interpolate_y_l.jl:32-88) */
int sipx_resample_nn(int dtype, int ndim, const int64_t* nc, const int64_t* nf, const void* in, void* out, int device);
/* the wavelet transform of SIPX_TRANSFORM_WAVELET on its own, out = W in (inverse = 0) or W' in (inverse != 0), on host arrays of the
 * grid n (ndim = 2 or 3, column-major), through the kernels of the projector -- W x sets a radius (the reference's constraint
 * learning, src/constraint_learning_by_observation.jl:68,114) */
int sipx_dwt(int dtype, int ndim, const int64_t* n, int inverse, const void* in, void* out, int device);

/* Constraint learning (src/constraint_learning_by_observation.jl:8-163, constraint_learning_by_obseration): statistics of
 * n_train training images on the 2-D grid n (n1, n2 >= 2) with spacings h.  Image i is m_train[i*s0 + a*s1 + b*s2] at grid
 * point (a, b), strides in elements (s0 = image, s1 = dim 1, s2 = dim 2); the layout must be dense with the image index
 * slowest (C-like blocks per image) or fastest (Julia's m_train[i,:,:]).  N = n1 n2, M = (n1-1) n2 + n1 (n2-1), D_x / D_z
 * are the forward differences along dim 1 / dim 2 with entries -+fl(1/h) in TF (the TDOperator's bits), TV = [D_z; D_x], F
 * the unitary 2-D DFT, W the transform of sipx_dwt, sigma the singular values in descending order.  TF is the dtype, TI is
 * int32 for SIPX_F32 and int64 for SIPX_F64.  Each field is a caller-owned host array, NULL = not wanted (that work is not
 * done).  Per image (n_train entries):
 *   nuclear_norm, nuclear_Dx, nuclear_Dz  TF  sum sigma of the image, of D_x img as (n1-1) x n2, of D_z img as n1 x (n2-1)
 *   rank_095                              TI  first 1-based k with cumsum(sigma)[k] / sum(sigma) > 0.95 (0 if sigma = 0)
 *   TV, Dx_l1, Dz_l1                      TF  ||TV img||_1, ||D_x img||_1, ||D_z img||_1
 *   wavelet_l1                            TF  ||W img||_1 if n1 == n2, else 0
 *   DFT_l1                                TF  ||F img||_1 over all N coefficients
 *   DFT_card_095, TV_card_095             TI  len(c) - k, k the first 1-based index with cumsum(sort(|c|))/sum > 0.05, c = F img
 *                                             or TV img (0 if c = 0)
 *   annulus, TV_annulus, D_l2             TF  ||img||_2, ||TV img||_2, ||TV img||_2
 *   D_x_min, D_x_max, D_z_min, D_z_max    TF  extrema of D_x img and D_z img
 * Across images (element-wise over the batch, the reference's starting values included):
 *   hist_min (N), hist_TV_min (M)         float64  min(1e8, sort(img)), min(1e8, sort(TV img))
 *   hist_max (N), hist_TV_max (M)         TF       max(0, sort(img)), max(0, sort(TV img))
 *   DCT_x_LB (n1), DCT_y_LB (n2)          float64  min(1e8, orthonormal DCT-II along dim 1 / dim 2, over the other dim)
 *   DCT_x_UB (n1), DCT_y_UB (n2)          TF       max(0, the same)
 * Sums run in float64 and round to TF once.  The images go through in chunks of max_batch (0 = sized from free device
 * memory); the results are bit-identical for every chunking. */
typedef struct {
  void* nuclear_norm; void* nuclear_Dx; void* nuclear_Dz; void* rank_095; void* TV; void* wavelet_l1; void* Dx_l1;
  void* Dz_l1; void* DFT_l1; void* DFT_card_095; void* TV_card_095; void* annulus; void* TV_annulus; void* D_l2;
  void* D_x_min; void* D_x_max; void* D_z_min; void* D_z_max; void* DCT_x_LB; void* DCT_x_UB; void* DCT_y_LB;
  void* DCT_y_UB; void* hist_min; void* hist_max; void* hist_TV_min; void* hist_TV_max;
} sipx_observations;
int sipx_learn_observations(int dtype, const int64_t* n, const double* h, int64_t n_train, const void* m_train,
                            const int64_t* strides, int64_t max_batch, sipx_observations* out, int device);
/* The BANDED part of Q as assembled / updated (N x d column-major) and its offsets: the sum over the sets that handed over
 * or generated CDS bands.  Matrix-free terms (SIPX_OP_CSC with ata_R = NULL) are not in it; sipx_apply_Q applies all of Q. */
int sipx_get_Q(sipx_ctx* ctx, void* Q, int64_t* offsets, int* d);
/* How the finalized context holds Q = sum_i rho_i A_i'A_i: *bands = bands of the CDS part (what sipx_get_Q returns as d),
 * *matrix_free = number of sets applied as matrix-free terms.  Either pointer may be NULL. */
int sipx_q_terms(sipx_ctx* ctx, int* bands, int* matrix_free);
/* device-side timing of the dominant kernel: runs cds_spmv on Q `reps` times, returns avg ms (HIP events on the engine stream) */
int sipx_time_spmv(sipx_ctx* ctx, int reps, double* avg_ms);
/* HIP-event timing of the engine's kernels, bracketed on the stream each launch goes to.  launches / total_ms report what
 * was gathered for the product of the CG iteration (cds_spmv fused with the dot product, src/CDS_MVp_MT.jl:9-25 + cg.jl:85-88)
 * since the last call; `enable` then (re)starts the collection: 0 = off, 1 = that kernel only (two event records per CG
 * iteration: cheap enough for a timed region), 2 = EVERY kernel (about 5 us per launch: for a window of its own). */
int sipx_kernel_stats(sipx_ctx* ctx, int enable, int64_t* launches, double* total_ms);
/* The same collection as a JSON text, one entry per kernel that ran: {"mode", "event_pair_overhead_ms", "kernels": [{"name",
 * "launches", "total_ms", "bytes_survey" (SURVEY 8d's algorithmic bytes of the reference function the kernel replaces, summed
 * over the launches), "bytes_moved" (what the kernel has to move at least), "gated" (some launches return at once on a
 * device-side condition), "inclusive" (the interval contains other listed kernels)}]}.  The pointer stays valid until the next
 * call on this context; NULL on error (sipx_last_error).  `enable` as above. */
const char* sipx_kernel_stats_json(sipx_ctx* ctx, int enable);
/* diagnostics: state of the projector-scalar search of set `set` (which = 0: prox, 1: feasibility) as 16 doubles:
 * need, theta, theta_prev, hw, spec_lo, spec_hi, lo, hi, asum, vmax, gathered, overflow, spec_ok, michelot_its, refine, 0 */
int sipx_debug_proj(sipx_ctx* ctx, int set, int which, double* out16);
/* engine stream handle (hipStream_t) so a host harness can order its own work / collectives against it */
void* sipx_stream(sipx_ctx* ctx);
/* device pointers of rhs / x (TF[N]) for in-place collectives on the sharded path.
 * sipx_dev_x: x lives in a ring of three buffers -- every x-step that changes x (sipx_argmin_x, sipx_parsdmm_steps) moves it to
 * another one and leaves the old iterate behind as x_old.  The pointer is therefore valid ONLY UNTIL THE NEXT x-step: ask again
 * after every step, never cache it (a cached pointer names x_old, or the Barzilai-Borwein snapshot, one step later).  Before the
 * first x-step x_old names x itself (the zero / warm start): evol_x of an update taken then is ||x - x|| = 0. */
void* sipx_dev_rhs(sipx_ctx* ctx);
void* sipx_dev_x(sipx_ctx* ctx);
/* rhs as composed by the last sipx_rhs_compose (host TF[N]; TF[2N] in Minkowski mode)           (src/rhs_compose.jl:24-36) */
int sipx_get_rhs(sipx_ctx* ctx, void* rhs);
/* x = (x*rho + m) / (rho + 1.0) on host vectors of length n, through the device function the y/l update applies for the
 * distance term (src/prox_l2s!.jl:3-6: numerator in TF, division in Float64) */
int sipx_prox_l2s(int dtype, int64_t n, void* x, double rho, const void* m, int device);
/* restricts y/l work and rhs contributions to sets with owner[i] != 0 (set sharding); Q stays global */
int sipx_set_owned(sipx_ctx* ctx, const int32_t* owned);

/* ---- sharded solve: one process per GPU ----
 * Replaces the reference's parallel mode (one Julia worker per set, src/PARSDMM.jl:114-131,183-197; the (+) reduction of
 * the partial right-hand sides, src/rhs_compose.jl:17-20; x shipped to every worker, src/update_y_l_parallel.jl:6-90).
 * With a communicator attached (before sipx_finalize) a context is one RANK of the solve:
 *   - the y/l work and the rhs contributions of the sets are split over the ranks (sipx_set_owned; default: set i on rank
 *     i mod world),
 *   - sipx_rhs_compose ends with a reduce-scatter of the partial rhs by z-slab (slabs of ceil(n_last / world) planes),
 *   - sipx_argmin_x runs CG on the rank's slab of rows of Q (one halo plane from each neighbour per product, the dot
 *     products through an all-reduce of the float64 block partials) and ends with an all-gather of x,
 *   - sipx_update_y_l ends with one all-reduce of the packed per-set sums, so every rank returns the r_pri / r_dual /
 *     feasibility of every set and takes the same rho / gamma / stop decisions; sipx_parsdmm runs the whole loop that way.
 *   - a rank / nuclear-norm set on the slices orthogonal to the last grid dimension (project_rank!.jl:23-47 applied slice
 *     by slice) is projected by ALL ranks: the owner scatters v by slab, every rank factorises the slices of its slab, a
 *     gather returns the projected v (the one set of BASELINE config 4 that outweighs all others together).
 * Every rank must make the same sequence of calls.  Q is maintained for the slab rows only (sipx_get_Q refuses), x is
 * complete on every rank, y_i / l_i live on the owner.  Not available with Minkowski components, the stencil form of Q or
 * operators whose A'A reaches further than one plane of the grid.
 *
 * sipx_set_comm_rccl: collectives by RCCL on the engine's own streams.  id128 = the 128-byte ncclUniqueId that rank 0
 * obtained from sipx_rccl_unique_id and the host side handed to every rank (torch.distributed store, MPI, a file ...). */
int sipx_rccl_unique_id(void* id128);
/* sipx_set_decomp (before sipx_finalize, with a communicator attached): how the ranks divide the work.
 *   SIPX_DECOMP_SETS (default): by constraint set, as described above -- the reference's own split.
 *   SIPX_DECOMP_SLAB: by z-slab of the grid, for the WHOLE iteration: every rank holds every set and works on its planes of
 *     the (globally indexed) arrays.  No N-vector crosses the fabric: the right-hand side needs no reduction, x no all-gather
 *     (one halo plane to each neighbour instead), the threshold searches all-reduce their 19 probe sums and all-gather the few
 *     magnitudes inside the final bracket, and every per-set sum goes through the one all-reduce of sipx_update_y_l.  Sets
 *     whose projector only needs sums over the grid -- bounds, l1 / l2 ball, annulus, prox_l1 on the identity or on D_x / D_y /
 *     D_z / TV -- work that way; since round 5 the others are taken too (y_i, l_i on the slabs as well): slice-wise rank /
 *     nuclear norm on z-slices by every rank on its own slices, cardinality by a search over the same collectives, the l1 ball
 *     behind the DFT on a 3-D grid by a slab-decomposed transform (one all-to-all each way), any other projector by an owner
 *     rank on the gathered vector (two fan exchanges for that set).  Refused: caller-supplied sparse operators, Minkowski
 *     contexts, the stencil form of Q.  sipx_set_owned is ignored; sipx_download is then a collective (every rank calls it: it
 *     gathers the slabs of x, y_i, l_i). */
#define SIPX_DECOMP_SETS 0
#define SIPX_DECOMP_SLAB 1
/* the same decomposition with FULL-size arrays on every rank: SIPX_DECOMP_SLAB backs every N-sized array of a rank with memory for
 * its planes and the halo planes around them only (device bytes per rank fall with the number of ranks; the levels of a multilevel
 * solve included since round 5); this mode is the A/B switch and the fallback when mapped memory cannot be exchanged */
#define SIPX_DECOMP_SLAB_FULL 2
int sipx_set_decomp(sipx_ctx* ctx, int mode);
int sipx_set_comm_rccl(sipx_ctx* ctx, const void* id128, int world, int rank);
/* sipx_set_comm: the same operations supplied by the caller.  Each callback enqueues its operation on `stream`
 * (a hipStream_t; or completes it before returning) and returns 0 on success; dtype is SIPX_F32 / SIPX_F64; all buffers are
 * device memory.  In place on `buf` of world * chunk elements:
 *   allreduce_sum:      buf[0 .. count) <- sum over ranks (identical bits on every rank)
 *   reduce_scatter_sum: buf[rank*chunk .. (rank+1)*chunk) <- sum over ranks of that range
 *   allgather:          buf[r*chunk .. (r+1)*chunk) <- that range of rank r, for every r
 *   halo_exchange:      send `count` elements to, and receive as many from, rank prev and rank next (-1 = no neighbour)
 *   scatter / gather:   in place on world * chunk elements: rank r receives buf[r*chunk .. (r+1)*chunk) of rank `root`, or
 *                       rank `root` receives that range of every rank r.  On a rank OTHER than `root` only its own range
 *                       buf[rank*chunk .. (rank+1)*chunk) is memory the callback may touch (round 5: with sparse arrays the rest of
 *                       the exchange layout is not backed there) */
typedef struct {
  void* user;
  int32_t world, rank;
  int (*allreduce_sum)(void* user, void* buf, int64_t count, int32_t dtype, void* stream);
  int (*reduce_scatter_sum)(void* user, void* buf, int64_t chunk, int32_t dtype, void* stream);
  int (*allgather)(void* user, void* buf, int64_t chunk, int32_t dtype, void* stream);
  int (*halo_exchange)(void* user, const void* send_prev, void* recv_prev, int32_t prev, const void* send_next, void* recv_next,
                       int32_t next, int64_t count, int32_t dtype, void* stream);
  int (*scatter)(void* user, void* buf, int64_t chunk, int32_t dtype, int32_t root, void* stream);
  int (*gather)(void* user, void* buf, int64_t chunk, int32_t dtype, int32_t root, void* stream);
} sipx_comm;
int sipx_set_comm(sipx_ctx* ctx, const sipx_comm* comm);
/* What the attached communicator itself reports: the ranks it spans and this rank's number in it (RCCL: ncclCommCount /
 * ncclCommUserRank -- asked of the library, not echoed from sipx_set_comm_rccl's arguments), its version as text ("rccl
 * 2.x.y" from ncclGetVersion, "callbacks (sipx_set_comm)", "none" without a communicator; version_len bytes incl. the
 * terminator), and the decomposition in force (SIPX_DECOMP_*).  So that "did RCCL see N ranks" can be answered from a log. */
int sipx_comm_info(sipx_ctx* ctx, int* nranks, int* rank, char* version, int version_len, int* decomposition);
/* Device memory: bytes this context holds (its own arrays and the buffers of its library-backed projectors; library
 * workspaces are not seen), and what the runtime reports for the whole device (used, total).  A slab-decomposed rank holds its
 * planes only (plus halo planes), so context_bytes falls with the number of ranks -- the figure the bench line carries as
 * comm.device_bytes_per_rank.  (No reference counterpart: Julia's GC owns the reference's arrays.) */
int sipx_device_bytes(sipx_ctx* ctx, int64_t* context_bytes, int64_t* device_used, int64_t* device_total);
/* this rank's slab of the x-step: rows [row0, row1) of Q / entries of x, and the elements per rank (chunk) of the padded
 * exchange buffers; without a communicator row0 = 0, row1 = chunk = N */
int sipx_slab(sipx_ctx* ctx, int64_t* row0, int64_t* row1, int64_t* chunk);

/* How the x-step applies Q = sum_i rho_i A_i'A_i.  SIPX_Q_CDS (default): explicit bands in CDS storage, the
 * reference's arithmetic (PARSDMM_initialize.jl:216-230, CDS_MVp_MT.jl:9-25, Q_update!.jl:45-48), (d+2) N w bytes per
 * product.  SIPX_Q_STENCIL ("beyond CDS"): coefficients generated from rho_i, h and the boundary
 * masks, 2 N w bytes per product and no Q_update! traffic; every set must use a descriptor-generated AtA
 * (ata_R = NULL).  Results agree with the CDS mode to rounding, not bit for bit.  Call before sipx_finalize. */
enum { SIPX_Q_CDS = 0, SIPX_Q_STENCIL = 1 };
int sipx_set_q_mode(sipx_ctx* ctx, int mode);
/* y = Q x (host TF[N] in and out) through the kernels the x-step uses, in either mode: the banded (or stencil) product plus
 * rho_i A_i'(A_i x) of every matrix-free term */
int sipx_apply_Q(sipx_ctx* ctx, const void* x, void* y);

#ifdef __cplusplus
}
#endif
#endif /* SIPX_H */
