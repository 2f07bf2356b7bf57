"""Host-side mirror of the reference's interface for the PARSDMM path, over the C ABI of
libsipx.so (include/sipx.h).  Same names, argument meaning and error behaviour as

    setup_constraints(constraint, comp_grid, TF)              src/setup_constraints.jl:17-102
    PARSDMM_precompute_distribute(TD_OP, set_Prop, grid, opt) src/PARSDMM_precompute_distribute.jl:6-77
    PARSDMM(m, AtA, TD_OP, set_Prop, P_sub, comp_grid, options[, x, l, y]) -> (x, log, l, y)
                                                              src/PARSDMM.jl:25-35,257

so that the parity tests read like the reference's own.  What differs, by design: TD_OP[i] is
a matrix-free operator DESCRIPTOR (TDOperator) instead of a SparseMatrixCSC and P_sub[i] is a
projector DESCRIPTOR (Projector) instead of an opaque closure -- both still behave like the
originals (``A @ x``, ``A.T @ v``, ``P(v)`` run the device kernels).  Nothing here computes on
the CPU; without libsipx.so or without a GPU every call raises SipxError.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import Any, List, Optional, Sequence, Tuple

import numpy as np

LIB_PATH = os.environ.get("SIPX_LIBRARY") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libsipx.so")

# every entry point declared in include/sipx.h
EXPORTED_SYMBOLS = [
    "sipx_last_error", "sipx_create", "sipx_destroy", "sipx_add_set", "sipx_set_rows", "sipx_num_terms",
    "sipx_finalize", "sipx_rhs_compose", "sipx_argmin_x", "sipx_update_y_l", "sipx_log_scalars",
    "sipx_adapt_rho_gamma", "sipx_q_update", "sipx_download", "sipx_parsdmm", "sipx_parsdmm_begin",
    "sipx_parsdmm_steps", "sipx_cds_spmv",
    "sipx_apply_op", "sipx_apply_op_adj", "sipx_project", "sipx_get_Q", "sipx_time_spmv", "sipx_kernel_stats",
    "sipx_debug_proj", "sipx_resample_nn", "sipx_set_q_mode", "sipx_apply_Q",
    "sipx_stream",
    "sipx_dev_rhs", "sipx_dev_x", "sipx_set_owned", "sipx_get_rhs", "sipx_prox_l2s",
    "sipx_rccl_unique_id", "sipx_set_comm_rccl", "sipx_set_comm", "sipx_slab", "sipx_warm_start_from", "sipx_set_decomp",
    "sipx_kernel_stats_json", "sipx_comm_info", "sipx_device_bytes", "sipx_reset", "sipx_dwt",
    "sipx_learn_observations",
    "sipx_finalize_dev", "sipx_reset_dev", "sipx_download_dev", "sipx_set_caller_stream", "sipx_io_bytes",
    "sipx_q_terms", "sipx_set_data", "sipx_set_data_dev", "sipx_segment_norms", "sipx_segment_norms_dev",
    "sipx_l21_norm", "sipx_l21_norm_dev", "sipx_l21_norms", "sipx_l21_norms_dev",
    "sipx_l21_joint_norm", "sipx_l21_joint_norm_dev", "sipx_l21_weighted_norm", "sipx_l21_weighted_norm_dev",
    "sipx_l21_groups_norm", "sipx_l21_groups_norm_dev", "sipx_tnv_norm", "sipx_tnv_norm_dev",
    "sipx_l1_weighted_norm", "sipx_l1_weighted_norm_dev", "sipx_segment_sums", "sipx_segment_sums_dev",
    "sipx_group_norms", "sipx_group_norms_dev", "sipx_card_groups_route", "sipx_tv_group_norms", "sipx_tv_group_norms_dev",
    "sipx_l21_stacked_norm", "sipx_l21_stacked_norm_dev", "sipx_l2inf_norm", "sipx_l2inf_norm_dev",
]

SIPX_F32, SIPX_F64 = 0, 1
OPS = {"identity": 0, "D_x": 1, "D_y": 2, "D_z": 3, "TV": 4, "D2D": 4, "D3D": 4, "custom": 5, "TV_xy": 6}
PROJ = {"bounds": 0, "bounds_vec": 1, "l1": 2, "l2": 3, "annulus": 4, "cardinality": 5, "prox_l1": 6, "l1_dft": 7, "rank": 8,
        "nuclear": 9, "histogram": 10, "subspace": 11, "bounds_dft": 12, "card_dft": 13, "l21": 14, "l21_joint": 15, "l21_groups": 16,
        "tnv": 17, "l1_weighted": 18, "simplex": 19, "card_groups": 20, "l20": 21, "l20_joint": 22, "l21_stacked": 23,
        "l2inf": 24, "l2inf_joint": 25, "l2inf_stacked": 26}
TV_OPERATORS = ("TV", "D2D", "D3D")      # one name per grid dimension count for the same operator (get_TD_operator.jl)
# the engine's refusal of the l2,1 ball off the TV operator (csrc/set_config.h, configure_proj), word for word; a mode on TV the
# engine refuses as it does for every multi-block operator, the front end in words of the set's own
L21_NEEDS_TV = "the l2,1 ball acts on the range of the TV operator: TD_OP must be TV (D2D, D3D)"
L21_WHOLE_ONLY = "the l2,1 ball applies to the whole array (mode matrix/tensor)"
# TV_xy = vcat(D_y, D_x), the in-plane gradient of a 3-D grid (include/sipx.h, SIPX_OP_TV_XY): the engine's own, with its refusals
L21_FRAMES_Z = "the l2,1 ball on TV_xy: frames run along z -- the mode must be (slice, z), or tensor for the whole array"
# the joint l2,1 ball (csrc/l21_joint.h): one group per pixel across the frames of TV_xy; the engine's refusal, word for word
L21_JOINT_NEEDS_TV_XY = "the joint l2,1 ball groups the frames of TV_xy: TD_OP must be TV_xy, mode tensor"
# total nuclear variation (csrc/tnv.h): the nuclear-norm ball on the 2 x n3 Jacobians of the pixels of TV_xy; the engine's refusals
# (csrc/ext_proj.h), word for word
TNV_NEEDS_TV_XY = "total nuclear variation couples the frames of TV_xy: TD_OP must be TV_xy, mode tensor, no transform"
TNV_NO_WEIGHTS = ("total nuclear variation (tnv) takes no weights or vectors (lb, ub): the weighted set across the frames is "
                  "(\"l21_joint\", \"TV_xy\")")
# one weight per group (csrc/l21_weighted.h): what takes them, and what to do where they are refused
L21_WEIGHTS_WHERE = ("weights belong to the l2,1 sets on the whole array -- (\"l21\", \"TV\"), (\"l21\", \"TV_xy\") in tensor mode and "
                     "(\"l21_joint\", \"TV_xy\"): drop them, or use one of these sets")
L21_WEIGHTS_NO_FRAMES = ("the l2,1 ball per frame takes no weights: use (\"l21\", \"TV_xy\") in tensor mode or (\"l21_joint\", \"TV_xy\"), "
                         "which take one weight per group")
L21_WEIGHTS_NO_COARSE = ("multilevel: a weighted l2,1 set has no rule that takes its weights to a coarser grid yet -- solve on one level, "
                         "or drop the weights")
# group sparsity over fibers or slices (csrc/l21_groups.h): one l2,1 ball whose groups are the fibers / slices of a one-block operator's
# range; the engine's refusals, word for word, and the front end's own
ONE_BLOCK_OPERATORS = ("identity", "D_x", "D_y", "D_z")
L21G_ONE_BLOCK = ("the l2,1 ball over fibers or slices (l21_groups) groups the range of a one-block operator: TD_OP must "
                  "be the identity, D_x, D_y or D_z (on TV use the l21 sets, whose groups are the grid points)")
L21G_NEEDS_MODE = ("the l2,1 ball over fibers or slices (l21_groups) needs a fiber or slice mode: on the whole array it has "
                   "one group and is the l2 ball -- use the l2 set")
L21G_2D_SLICE = "for 2D models, the mode of application for l21_groups sets needs to be (fiber,x) or (fiber,z)"
L21G_NO_TRANSFORM = "the l2,1 ball over fibers or slices (l21_groups) takes no transform: it acts on A x itself"
L21G_NO_MINKOWSKI = "the l2,1 ball over fibers or slices (l21_groups) takes no Minkowski component"
L21G_NO_CUSTOM = ("the l2,1 ball over fibers or slices (l21_groups) takes no custom operator: its segments are the fibers / slices of a "
                  "grid-shaped range -- TD_OP must be the identity, D_x, D_y or D_z")
L21G_NO_COARSE = ("multilevel: the l2,1 ball over fibers or slices (l21_groups) has no rule that takes its radius to a coarser grid yet -- "
                  "solve on one level")
# the weighted l1 ball (csrc/l1_weighted.h): one weight per row of identity, D_x, D_y, D_z, TV or TV_xy; the engine's refusals, word for
# word, and the front end's own
L1W_OPERATORS = ("identity", "D_x", "D_y", "D_z", "TV", "D2D", "D3D", "TV_xy")
L1W_NO_MODE = ("the weighted l1 ball (l1_weighted) applies to the whole array (matrix / tensor mode): per fiber or slice use "
               "(\"l1\", op, mode) with segment_norms=True, which takes one radius per segment")
L1W_NO_TRANSFORM = ("the weighted l1 ball (l1_weighted) takes no transform (DFT, DCT, wavelet): its weights are one per row of "
                    "identity, D_x, D_y, D_z, TV or TV_xy -- behind a transform use the plain (\"l1\", transform)")
L1W_NO_CUSTOM = ("the weighted l1 ball (l1_weighted) takes no custom operator: its weights follow the rows of identity, D_x, "
                 "D_y, D_z, TV or TV_xy -- scale the rows of the operator and use the plain (\"l1\", op)")
L1W_NO_MINKOWSKI = "the weighted l1 ball (l1_weighted) takes no Minkowski component: use the plain (\"l1\", op) there"
L1W_NEEDS_WEIGHTS = ("the weighted l1 ball (l1_weighted) needs weights, one per row of the operator: without weights the set is the "
                     "plain (\"l1\", op)")
L1W_NO_COARSE = ("multilevel: the weighted l1 ball (l1_weighted) has no rule that takes its weights to a coarser grid yet -- solve on one "
                 "level, or use the plain (\"l1\", op)")
L1W_WEIGHTS_ARE_LB = ("set_data: the weights of the weighted l1 ball are its lb; it has no ub (the radius is fixed when the set is built)")
# simplex sets (csrc/seg_simplex.h): entries >= 0 and a sum in [min, max] on every fiber / slice of the range of a one-block operator; the
# engine's refusals, word for word, and the front end's own
SIMPLEX_NEEDS_MODE = ("the simplex set (simplex) on the whole array is not built yet: it constrains every fiber or slice -- use a "
                      "(\"fiber\", d) or (\"slice\", d) mode, or (\"bounds\") together with (\"l1\") on the whole array as a stand-in")
SIMPLEX_2D_SLICE = "for 2D models, the mode of application for simplex sets needs to be (fiber,x) or (fiber,z)"
SIMPLEX_ONE_BLOCK = ("the simplex set (simplex) constrains the fibers or slices of the range of a one-block operator: TD_OP must "
                     "be the identity, D_x, D_y or D_z -- for TV or a custom operator use one set per direction")
SIMPLEX_NO_TRANSFORM = ("the simplex set (simplex) takes no transform (DFT, DCT, wavelet): it acts on A x itself -- use it "
                        "with TD_OP identity, D_x, D_y or D_z")
SIMPLEX_NO_MINKOWSKI = ("the simplex set (simplex) takes no Minkowski component: constrain the sum of the components "
                        "with a set on the identity instead")
SIMPLEX_NO_VECTORS = ("the simplex set (simplex) takes one pair of scalars (min, max) for all segments for now and no lb / ub "
                      "vectors: use (\"l1\", op, mode) with one radius per segment beside (\"bounds\")")
SIMPLEX_BAD_BOUNDS = ("the simplex set (simplex) needs 0 <= min <= max, max > 0, both finite: every segment has entries >= 0 "
                      "and a sum in [min, max] (min = max = 1: the probability simplex, min = 0: the capped one)")
SIMPLEX_NO_WEIGHTS = "the simplex set (simplex) takes no weights: scale the array, or use (\"l1_weighted\", op) beside (\"bounds\")"
SIMPLEX_NO_COARSE = ("multilevel: the simplex set (simplex) has no rule that takes its segments to a coarser grid yet -- solve on one level")
# group cardinality (csrc/card_groups.h): at most k non-zero fibers / slices of the range of a one-block operator; the engine's refusals,
# word for word, and the front end's own
CARDG_NEEDS_MODE = ("group cardinality (card_groups) needs a fiber or slice mode: on the whole array it has one group, which "
                    "every k >= 1 keeps -- drop the set, or count entries with the cardinality set")
CARDG_2D_SLICE = "for 2D models, the mode of application for card_groups sets needs to be (fiber,x) or (fiber,z)"
CARDG_ONE_BLOCK = ("group cardinality (card_groups) counts the fibers or slices of the range of a one-block operator: TD_OP "
                   "must be the identity, D_x, D_y or D_z (on TV or a custom operator use the cardinality set, which counts "
                   "entries)")
CARDG_NO_TRANSFORM = ("group cardinality (card_groups) takes no transform (DFT, DCT, wavelet): it acts on A x itself -- use "
                      "the cardinality set behind the transform, which counts coefficients")
CARDG_NO_MINKOWSKI = "group cardinality (card_groups) takes no Minkowski component: constrain the sum of the components"
CARDG_NO_VECTORS = ("group cardinality (card_groups) takes one k for the whole array and no lb / ub / weights: a segment is kept "
                    "or dropped whole -- for weights per segment use the l21_groups set")
CARDG_NO_SET_DATA = ("group cardinality (card_groups) holds no vectors to replace: k is fixed when the set is added -- build a "
                     "new context for another k")
CARDG_SHARDED = ("group cardinality (card_groups) takes single-process contexts only, this one has a communicator, a slab "
                 "decomposition or set ownership: its segments compete for k places across the whole array -- use a "
                 "single process")
CARDG_BAD_K = ("group cardinality (card_groups) needs an integer k >= 1, the number of fibers or slices kept (k = 0 is the "
               "zero array: use bounds)")
CARDG_K_INEXACT = ("group cardinality (card_groups): a k below the number of segments must be exactly representable in the "
                   "working precision, since the search reads k from it -- Float32: k <= 2^24; use Float64")
CARDG_TOO_LARGE = "group cardinality (card_groups): the grid needs fewer than 2^31 points -- split the array"
CARDG_NO_COARSE = ("multilevel: group cardinality (card_groups) has no rule that takes k to a grid with another number of segments -- "
                   "solve on one level")
# the l2,0 sets on total variation (csrc/l20.h): at most k grid points (pixels) carry a gradient vector; the engine's refusals, word for word
L20_NEEDS_TV = ("the l2,0 set (l20) counts the gradient vectors of the TV operator: TD_OP must be TV (D2D, D3D) or TV_xy, not a "
                "one-block or custom operator (there use the cardinality set, which counts entries, or card_groups)")
L20_JOINT_ROUTE = ("the joint l2,0 set (l20_joint) needs the TV_xy operator of a 3-D grid in tensor mode: its groups span "
                   "the frames -- for one budget over all grid points use (\"l20\", \"TV_xy\"), per frame (\"l20\", \"TV_xy\", "
                   "(\"slice\", \"z\"))")
L20_MODES = ("the l2,0 set (l20) applies to the whole array (matrix / tensor mode), or per frame as (\"slice\", \"z\") on TV_xy: "
             "fiber modes and other slices have no gradient groups -- use card_groups on D_x, D_y or D_z there")
L20_NO_TRANSFORM = ("the l2,0 set (l20, l20_joint) takes no transform (DFT, DCT, wavelet): it acts on TV x itself -- use the "
                    "cardinality set behind the transform, which counts coefficients")
L20_NO_MINKOWSKI = "the l2,0 set (l20, l20_joint) takes no Minkowski component: constrain the sum of the components"
L20_NO_WEIGHTS = ("the l2,0 set (l20, l20_joint) takes no weights and no lb: a group is kept or dropped whole by its plain "
                  "norm -- for weighted groups use the l21 set with weights")
L20_K_VECTOR = ("the l2,0 set (l20) takes one k, or per frame -- (\"slice\", \"z\") on TV_xy -- a vector of n3 integers in max; "
                "every other form has one budget: pass a scalar")
L20_NO_SET_DATA = ("the l2,0 set (l20, l20_joint) built with a scalar k holds no vectors to replace -- build the per-frame "
                   "set with a vector of n3 budgets to replace them, or a new context for another k")
L20_SET_DATA_UB = "the l2,0 set (l20) per frame: the budgets are its ub, n3 integers >= 1; it has no lb"
L20_SHARDED = ("the l2,0 set (l20, l20_joint) takes single-process contexts only, this one has a communicator, a slab "
               "decomposition or set ownership: its groups span the blocks of TV and compete for k places across the "
               "whole array -- use a single process")
L20_NO_COARSE = ("multilevel: the l2,0 set (l20, l20_joint) has no rule that takes k to a grid with another number of "
                 "points -- solve on one level")
L20_BAD_K = ("the l2,0 set (l20, l20_joint) needs an integer k >= 1, the number of grid points that may carry a gradient "
             "(k = 0 is the constant array: use bounds on TV)")
L20_K_INEXACT = ("the l2,0 set (l20, l20_joint): a k below the number of groups must be exactly representable in the "
                 "working precision, since the search reads k from it -- Float32: k <= 2^24; use Float64")
L20_TOO_LARGE = "the l2,0 set (l20, l20_joint): the grid needs fewer than 2^31 points -- split the array"
# the l2,1 ball across the equal-sized blocks of a stacked operator (csrc/l21_stacked.h): the engine's refusals, word for word
L21S_MAX_BLOCKS = 8
L21S_NEEDS_CSC = ("the stacked l2,1 ball (l21_stacked) groups the rows of a caller-supplied sparse operator across its blocks: "
                  "the operator must be SIPX_OP_CSC (custom_TD_OP, or the named \"Hessian\") -- on the built-in TV operator "
                  "the set is (\"l21\", \"TV\")")
L21S_WHOLE_ONLY = ("the stacked l2,1 ball (l21_stacked) applies to the whole array (matrix / tensor mode): its groups are the "
                   "rows p, G + p, 2 G + p, ... of the operator, fibers and slices have no meaning there")
L21S_NO_TRANSFORM = "the stacked l2,1 ball (l21_stacked) takes no transform (DFT, DCT, wavelet): it acts on A x itself"
L21S_NO_MINKOWSKI = "the stacked l2,1 ball (l21_stacked) takes no Minkowski component: custom operators have none"
L21S_NO_VECTORS = "the stacked l2,1 ball (l21_stacked) takes no weights and no vectors (lb, ub): weights per group are not built"
L21S_SHARDED = ("the stacked l2,1 ball (l21_stacked) takes single-process contexts only, this one has a communicator, a slab "
                "decomposition or set ownership: its groups span the blocks of a caller-supplied operator -- use a single process")
L21S_NO_COARSE = ("multilevel: the stacked l2,1 ball (l21_stacked, (\"l21\", \"Hessian\")) is not built for PARSDMM_multi_level: "
                  "solve on one level")
HESSIAN_SMALL_GRID = ("the Hessian operator needs at least 3 grid points along every dimension (a second difference has three "
                      "points), this grid is {n}")


def l21s_bad_blocks(B):
    return (f"the stacked l2,1 ball (l21_stacked): blocks = {B}, the number of equal-sized blocks of the operator must be 1 .. "
            f"{L21S_MAX_BLOCKS}")


def l21s_bad_rows(M, B):
    return (f"the stacked l2,1 ball (l21_stacked): the operator has M = {M} rows, not a multiple of blocks = {B} -- every block needs "
            "the same number of rows (pad a shorter block with zero rows)")


# the l2,inf ball: pointwise bounds on the group norms of TV / TV_xy, of the joint groups or of a stacked operator (csrc/l2inf.h): the
# engine's refusals, word for word
L2INF_KINDS = ("l2inf", "l2inf_joint", "l2inf_stacked")
L2INF_NEEDS_TV = ("the l2,inf ball (l2inf) bounds the gradient magnitude at every grid point: TD_OP must be TV (D2D, D3D), TV_xy "
                  "or the named \"Hessian\" -- a bound on one difference direction is (\"bounds\", \"D_z\"), a caller-supplied "
                  "stacked operator takes (\"l2inf_stacked\", name, 0, c, mode, custom_TD_OP=(A, False), blocks=B)")
L2INF_JOINT_ROUTE = ("the joint l2,inf ball (l2inf_joint) groups the frames of TV_xy: TD_OP must be TV_xy, mode tensor -- per "
                     "frame bounds are (\"l2inf\", \"TV_xy\")")
L2INF_STACKED_NEEDS_CSC = ("the stacked l2,inf ball (l2inf_stacked) groups the rows of a caller-supplied sparse operator across its "
                           "blocks: the operator must be SIPX_OP_CSC (custom_TD_OP, or the named \"Hessian\") -- on the built-in TV "
                           "operator the set is (\"l2inf\", \"TV\")")
L2INF_MIN = ("the l2,inf ball (l2inf, l2inf_joint, l2inf_stacked) bounds the group norms from above only: min must be 0 -- a lower "
             "bound on the gradient magnitude is not convex and not built")
L2INF_BAD_C = ("the l2,inf ball (l2inf, l2inf_joint, l2inf_stacked) needs a bound c > 0 as a scalar (c = 0 is the constant array: "
               "use bounds on TV, or a vector of zeros to flatten chosen points)")
L2INF_MODES = ("the l2,inf ball (l2inf, l2inf_joint, l2inf_stacked) applies to the whole array (matrix / tensor mode), fibers and "
               "slices are not built: (\"slice\", \"z\") on TV_xy is the vector form with c constant within every frame -- pass "
               "max = np.repeat(c_frames, n1 * n2)")
L2INF_NO_TRANSFORM = ("the l2,inf ball (l2inf, l2inf_joint, l2inf_stacked) takes no transform (DFT, DCT, wavelet): it acts on the "
                      "differences of x themselves")
L2INF_NO_WEIGHTS = ("the l2,inf ball (l2inf, l2inf_joint, l2inf_stacked) takes no weights (lb): a weight per group is its bound, pass "
                    "the vector of bounds as max (ub)")
L2INF_NO_MINKOWSKI = "the l2,inf ball (l2inf, l2inf_joint, l2inf_stacked) takes no Minkowski component: bound the sum itself"
L2INF_SHARDED = ("the l2,inf ball (l2inf, l2inf_joint, l2inf_stacked) takes single-process contexts only, this one has a "
                 "communicator, a slab decomposition or set ownership: its groups span the blocks of the operator -- use "
                 "(\"bounds\", \"TV\"), or a single process")
L2INF_NO_COARSE = ("multilevel: the l2,inf ball (l2inf, l2inf_joint, l2inf_stacked) is not built for PARSDMM_multi_level: a bound on "
                   "the gradient magnitude does not carry over to a coarser grid unchanged -- solve on one level")
L2INF_NO_SET_DATA = ("this l2,inf set was built with a scalar bound, which is fixed at sipx_add_set: build it with a vector of bounds "
                     "(ub) to replace them in a live context")


def l2inf_bad_length(given, groups):
    return (f"the l2,inf ball (l2inf, l2inf_joint, l2inf_stacked): the vector of bounds has {given} entries, the set has "
            f"{groups} groups (one bound per grid point, per pixel of the joint set, or per row of one block)")


def l2inf_bad_entry(p):
    return (f"the l2,inf ball (l2inf, l2inf_joint, l2inf_stacked): bound {p} is negative or NaN -- every bound must be >= 0 "
            "(+inf leaves a point free, 0 flattens it)")


def l2inf_bad_blocks(B):
    return f"the stacked l2,inf ball (l2inf_stacked): blocks = {B}, the number of equal-sized blocks of the operator must be 1 .. 8"


def l2inf_bad_rows(M, B):
    return (f"the stacked l2,inf ball (l2inf_stacked): the operator has M = {M} rows, not a multiple of blocks = {B} -- every block needs "
            "the same number of rows (pad a shorter block with zero rows)")


def _check_l2inf_bounds(c, per, stacked):
    """A host vector of bounds of an l2,inf set (csrc/l2inf.h, l2inf_check_vector): every entry >= 0, NaN refused; the entry of a group
    without a member -- index per - 1 of every run of per entries; a stacked operator has none -- is not looked at."""
    c = np.asarray(c)
    bad = ~(c >= 0)
    if not stacked and per:
        bad[per - 1::per] = False
    if bad.any():
        raise SipxError(l2inf_bad_entry(int(np.flatnonzero(bad)[0])))


UNKNOWN_OPERATOR = "provided an unknown transform domain operator. check function get_TD_operator(comp_grid,TD_type,TF) for options"
TV_XY_NEEDS_3D = UNKNOWN_OPERATOR + " (TV_xy is the in-plane gradient of a 3-D grid; on a 2-D grid TV is in-plane already)"
TV_XY_NO_MINKOWSKI = "the TV_xy operator takes no Minkowski component"
TV_XY_NO_MULTILEVEL = "the TV_xy operator is not built for PARSDMM_multi_level: solve on one level"
MODES = {"matrix": 0, "tensor": 0, "fiber": 1, "slice": 2}
TRANSFORMS = {"DCT": 1, "wavelet": 2}
SPECIAL_OPERATORS = ("DFT", "DCT", "wavelet", "curvelet")     # src/setup_constraints.jl:54
YL_FEAS, YL_BB, YL_FIRST = 1, 2, 4
Q_MODES = {"cds": 0, "stencil": 1}
MAX_Q_BANDS = 32        # bands the engine keeps of Q in CDS form (MAXD, csrc/sipx_common.h)
MAX_SET_BANDS = 9       # bands of A'A one set may hand over (csrc/set_config.h, configure_set)


class SipxError(RuntimeError):
    pass


class _SetDesc(C.Structure):
    _fields_ = [("op", C.c_int32), ("proj", C.c_int32), ("pmin", C.c_double), ("pmax", C.c_double),
                ("lb", C.c_void_p), ("ub", C.c_void_p), ("ncvx", C.c_int32), ("reserved", C.c_int32),
                ("mode", C.c_int32), ("dir", C.c_int32), ("basis", C.c_void_p), ("basis_rows", C.c_int64),
                ("basis_cols", C.c_int32), ("basis_orth", C.c_int32), ("component", C.c_int32),
                ("csc_colptr", C.c_void_p), ("csc_rowval", C.c_void_p), ("csc_nzval", C.c_void_p), ("csc_rows", C.c_int64),
                ("transform", C.c_int32), ("pad_", C.c_int32), ("blocks", C.c_int32), ("pad2_", C.c_int32)]


class _Options(C.Structure):
    _fields_ = [("maxit", C.c_int32), ("evol_rel_tol", C.c_double), ("feas_tol", C.c_double),
                ("obj_tol", C.c_double), ("rho_update_frequency", C.c_int32), ("adjust_rho", C.c_int32),
                ("adjust_gamma", C.c_int32), ("adjust_feasibility_rho", C.c_int32)]


class _Log(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("set_feasibility", "r_dual", "r_pri", "r_dual_total", "r_pri_total",
                                           "obj", "evol_x", "rho", "gamma", "cg_it", "cg_relres")] + \
               [("timing_ms", C.c_double * 7), ("n_iter", C.c_int32), ("n_feas_rows", C.c_int32),
                ("stopped_feasible", C.c_int32)]


_lib = None
_default_device = 0


def set_default_device(device: int):
    """GPU used by contexts that are created implicitly (operator products, stand-alone projector calls)."""
    global _default_device
    _default_device = int(device)


def lib():
    """The loaded libsipx.so.  Raises when it has not been built: the product never falls back."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SipxError(f"{LIB_PATH} is missing -- run `python -c 'import __graft_entry__ as g; g.build()'`; "
                            "the engine has no CPU fallback")
        L = C.CDLL(LIB_PATH)
        L.sipx_last_error.restype = C.c_char_p
        for name in ("sipx_stream", "sipx_dev_rhs", "sipx_dev_x"):
            getattr(L, name).restype = C.c_void_p
            getattr(L, name).argtypes = [C.c_void_p]
        L.sipx_kernel_stats_json.restype = C.c_char_p
        L.sipx_kernel_stats_json.argtypes = [C.c_void_p, C.c_int]
        L.sipx_destroy.restype = None
        L.sipx_destroy.argtypes = [C.c_void_p]
        _lib = L
    return _lib


def _chk(rc):
    if rc != 0:
        raise SipxError(lib().sipx_last_error().decode())


def _dtype_code(TF):
    TF = np.dtype(TF).type
    if TF == np.float32:
        return SIPX_F32
    if TF == np.float64:
        return SIPX_F64
    raise SipxError("FL must be Float32 or Float64")


def _ptr(a):
    """The data of a numpy array as a void pointer (None: the null pointer)."""
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _tensor_ptr(t):
    """The same for a torch tensor."""
    return None if t is None else C.c_void_p(t.data_ptr())


def _ptr_array(lst, ptr=_ptr):
    """A C array of void pointers, one per vector of the list (None: the null pointer).  The caller keeps the vectors alive."""
    return None if lst is None else (C.c_void_p * len(lst))(*[ptr(a) for a in lst])


# --------------------------------------------------------------------------------------------------
# boundary types (src/SetIntersectionProjection.jl:95-149)
# --------------------------------------------------------------------------------------------------
@dataclass
class compgrid:
    d: Tuple
    n: Tuple


@dataclass
class PARSDMM_options:
    x_min_solver: str = "CG_normal"
    maxit: int = 200
    evol_rel_tol: float = 1e-3
    feas_tol: float = 5e-2
    obj_tol: float = 1e-3
    rho_ini: Sequence[float] = (10.0,)
    rho_update_frequency: int = 2
    gamma_ini: float = 1.0
    adjust_rho: bool = True
    adjust_gamma: bool = True
    adjust_feasibility_rho: bool = True
    Blas_active: bool = True
    feasibility_only: bool = False
    FL: Any = np.float32
    parallel: bool = False
    zero_ini_guess: bool = True
    Minkowski: bool = False
    Q_mode: str = "cds"     # engine extension (not a reference field): "cds" = the reference's banded Q, "stencil" = sipx_set_q_mode(SIPX_Q_STENCIL)


def default_PARSDMM_options(options: PARSDMM_options, TF) -> PARSDMM_options:
    """src/default_PARSDMM_options.jl:6-34."""
    d = PARSDMM_options(FL=TF)
    for k, v in d.__dict__.items():
        setattr(options, k, v)
    return options


@dataclass
class set_definitions:
    set_type: str
    TD_OP: str
    min: Any
    max: Any
    app_mode: Tuple[str, str]
    custom_TD_OP: Tuple[Any, bool] = ((), False)
    weights: Any = None      # the l2,1 sets on the whole array: one weight >= 0 per group (csrc/l21_weighted.h), None: the plain ball;
                             # l21_groups: one per fiber / slice, in the order of segment_norms (csrc/l21_groups.h);
                             # l1_weighted: one per row of the operator, in the order of A @ x (csrc/l1_weighted.h), required
    blocks: Any = None       # l21_stacked: B, the number of equal-sized blocks of the stacked operator (csrc/l21_stacked.h), 1 .. 8;
                             # None: that of the named operator ("Hessian": 3 on a 2-D grid, 6 on a 3-D one)


@dataclass
class set_properties:
    ncvx: List[bool] = field(default_factory=list)
    AtA_diag: List[bool] = field(default_factory=list)
    dense: List[bool] = field(default_factory=list)
    TD_n: List[Tuple] = field(default_factory=list)
    tag: List[Tuple[str, str, str, str]] = field(default_factory=list)
    banded: List[bool] = field(default_factory=list)
    AtA_offsets: List[Any] = field(default_factory=list)


@dataclass
class log_type_PARSDMM:
    set_feasibility: np.ndarray
    r_dual: np.ndarray
    r_pri: np.ndarray
    r_dual_total: np.ndarray
    r_pri_total: np.ndarray
    obj: np.ndarray
    evol_x: np.ndarray
    rho: np.ndarray
    gamma: np.ndarray
    cg_it: np.ndarray
    cg_relres: np.ndarray
    timing: Any = None


TIMING_SECTIONS = ("initialization", "form rhs for linear system", "argmin x", "argmin y and l update",
                   "stopping conditions check", "adjust rho and gamma", "Q-update")   # src/PARSDMM.jl @timeit names


def _grid(comp_grid):
    n = tuple(int(v) for v in comp_grid.n)
    if len(n) == 3 and n[2] == 1:
        n = n[:2]
    return n, tuple(float(v) for v in comp_grid.d[:len(n)])


# --------------------------------------------------------------------------------------------------
# descriptors standing in for TD_OP[i] and P_sub[i]
# --------------------------------------------------------------------------------------------------
class TDOperator:
    """Matrix-free stand-in for the SparseMatrixCSC a difference/identity TD_OP is in the reference."""

    def __init__(self, kind: str, comp_grid, TF, adjoint=False, component=0):
        if kind not in OPS:
            raise SipxError("provided an unknown transform domain operator. check function "
                            "get_TD_operator(comp_grid,TD_type,TF) for options")
        self.kind, self.comp_grid, self.TF, self.adjoint = kind, comp_grid, np.dtype(TF).type, adjoint
        n, _ = _grid(comp_grid)
        self.n = n
        if kind == "TV_xy" and len(n) != 3:
            raise SipxError(TV_XY_NEEDS_3D)
        if kind == "TV_xy" and component:
            raise SipxError(TV_XY_NO_MINKOWSKI)
        N = int(np.prod(n))
        if kind == "identity":
            rows = N
        else:
            dirs = {"D_x": [0], "D_y": [1], "D_z": [len(n) - 1], "TV": list(range(len(n))), "D2D": list(range(len(n))),
                    "D3D": list(range(len(n))), "TV_xy": [0, 1]}[kind]
            rows = sum(N // n[a] * (n[a] - 1) for a in dirs)
        # Minkowski block rows [A 0] (1), [0 A] (2), [A A] (3) act on [u; v]  (PARSDMM_precompute_distribute_Minkowski.jl:91-103)
        self.component = int(component)
        cols = 2 * N if self.component else N
        self.shape = (cols, rows) if adjoint else (rows, cols)

    @property
    def T(self):
        return TDOperator(self.kind, self.comp_grid, self.TF, not self.adjoint, self.component)

    def __matmul__(self, v):
        v = np.ascontiguousarray(v, dtype=self.TF)
        if v.shape != (self.shape[1],):
            raise SipxError("dimension mismatch")
        if self.component:
            plain = TDOperator(self.kind, self.comp_grid, self.TF, self.adjoint)
            N = int(np.prod(self.n))
            if self.adjoint:
                t = plain @ v
                z = np.zeros(N, self.TF)
                return np.concatenate([t if self.component in (1, 3) else z, t if self.component in (2, 3) else z])
            u, w = v[:N], v[N:]
            return plain @ (u if self.component == 1 else (w if self.component == 2 else (u + w).astype(self.TF)))
        out = np.empty(self.shape[0], self.TF)
        ctx = Context(self.comp_grid, self.TF)
        try:
            f = lib().sipx_apply_op_adj if self.adjoint else lib().sipx_apply_op
            _chk(f(ctx.h, OPS[self.kind], _ptr(v), _ptr(out)))
        finally:
            ctx.close()
        return out

    __mul__ = __matmul__


class CustomOperator:
    """A caller-supplied sparse TD_OP (constraint.custom_TD_OP[1], src/setup_constraints.jl:70-72): kept as a scipy CSC
    matrix on the host, shipped to the engine as SIPX_OP_CSC.  Behaves like the matrix for `@` and `.T` (host arithmetic,
    used by setup code only)."""
    kind = "custom"
    component = 0

    def __init__(self, A, comp_grid, TF):
        import scipy.sparse as sp
        self.TF = np.dtype(TF).type
        self.comp_grid = comp_grid
        self.n, _ = _grid(comp_grid)
        A = sp.csc_matrix(A, dtype=self.TF)
        A.sort_indices()
        if A.shape[1] != int(np.prod(self.n)):
            raise SipxError("custom TD_OP: the number of columns must equal the number of grid points")
        self.A = A
        self.shape = A.shape

    @property
    def T(self):
        return self.A.T.tocsc()

    def __matmul__(self, v):
        return (self.A @ np.asarray(v, self.TF)).astype(self.TF)

    def ata_cds(self):
        """mat2CDS(TD_OP' * TD_OP) (PARSDMM_precompute_distribute.jl:52-59, mat2CDS.jl:7-32) in the working precision."""
        G = (self.A.T @ self.A).tocsc().astype(self.TF)
        G.sort_indices()
        N = G.shape[0]
        coo = G.tocoo()
        diag = coo.col.astype(np.int64) - coo.row.astype(np.int64)
        offs = np.unique(diag)
        R = np.zeros((N, len(offs)), self.TF, order="F")
        R[coo.row, np.searchsorted(offs, diag)] = coo.data      # (sorted indices, duplicates summed: every (row, band) once)
        return R, offs.astype(np.int64)

    def ata_diagonals(self):
        """Number of distinct diagonals of TD_OP' * TD_OP, from the sparsity patterns alone."""
        import scipy.sparse as sp
        P = sp.csc_matrix((np.ones(self.A.nnz, np.int64), self.A.indices, self.A.indptr), shape=self.A.shape)
        coo = (P.T @ P).tocoo()
        return len(np.unique(coo.col.astype(np.int64) - coo.row.astype(np.int64)))


class Projector:
    """Descriptor of P_sub[i] (src/get_projector.jl:3-103); calling it projects in place on the device."""

    def __init__(self, constraint: set_definitions, comp_grid, TF):
        self.TF = np.dtype(TF).type
        self.comp_grid = comp_grid
        st = constraint.set_type
        n, _ = _grid(comp_grid)
        am = tuple(constraint.app_mode)
        if am[0] not in MODES:
            raise SipxError(f"unknown application mode {am!r}")
        self.mode, self.dir = MODES[am[0]], 0
        if am == ("slice", "z") and len(comp_grid.n) == 3 and int(comp_grid.n[2]) == 1:
            self.mode = MODES["matrix"]      # a tensor of one plane is handled as a 2-D grid (_grid): its one z-slice is the array itself
        if self.mode:
            dirs = {"x": 0, "z": len(n) - 1} if len(n) == 2 else {"x": 0, "y": 1, "z": 2}
            if am[1] not in dirs:
                raise SipxError(f"application mode {am!r}: direction must be one of {sorted(dirs)} on this grid")
            self.dir = dirs[am[1]]
        if self.mode and st in ("l1", "l2", "annulus"):
            # l1 / l2 / annulus per fiber or slice (csrc/seg_norm.h): on the array itself or behind D_x / D_y / D_z only
            if constraint.TD_OP in SPECIAL_OPERATORS or constraint.TD_OP in ("DCT", "wavelet"):
                raise SipxError(f"{st} sets behind the {constraint.TD_OP} apply to the whole array (matrix / tensor mode)")
            if len(n) == 2 and self.mode == MODES["slice"]:
                raise SipxError(f"for 2D models, the mode of application for {st} sets needs to be (fiber,x) or (fiber,z), "
                                "or matrix for the whole array")
        self.lb = self.ub = self.basis = None
        self.basis_orth = False
        self.pmin = self.pmax = 0.0
        self.transform = 0
        self.weighted = False        # an l2,1 set built with one weight per group (in lb)
        self.blocks = 0              # l21_stacked: the equal-sized blocks of the operator the groups run across
        self.rows = None             # l21_stacked: the rows M of that operator, the length of the vector a stand-alone call projects
        if st == "tnv":
            # total nuclear variation: the Jacobians of the pixels across the frames of TV_xy (csrc/tnv.h); max is the radius
            cust = constraint.custom_TD_OP[0]
            if constraint.TD_OP != "TV_xy" or not (isinstance(cust, (tuple, list)) and len(cust) == 0):
                raise SipxError(TNV_NEEDS_TV_XY)
            if len(n) != 3:
                raise SipxError(TV_XY_NEEDS_3D)
            if self.mode:
                raise SipxError(TNV_NEEDS_TV_XY)
            if getattr(constraint, "weights", None) is not None or np.ndim(constraint.max) != 0 or np.ndim(constraint.min) != 0:
                raise SipxError(TNV_NO_WEIGHTS)
            if not float(constraint.max) > 0:
                raise SipxError("Radius of L1 ball is negative")
            self.seg_radii = False
            self.kind, self.pmax, self.op = "tnv", float(constraint.max), "TV_xy"
            return
        if getattr(constraint, "weights", None) is not None and st == "simplex":
            raise SipxError(SIMPLEX_NO_WEIGHTS)
        if getattr(constraint, "weights", None) is not None and st == "card_groups":
            raise SipxError(CARDG_NO_VECTORS)
        if getattr(constraint, "weights", None) is not None and st in ("l20", "l20_joint"):
            raise SipxError(L20_NO_WEIGHTS)
        if getattr(constraint, "weights", None) is not None and st in L2INF_KINDS:
            raise SipxError(L2INF_NO_WEIGHTS)
        if getattr(constraint, "weights", None) is not None and st not in ("l21", "l21_joint", "l21_groups", "l1_weighted"):
            raise SipxError(f"set type {st!r} takes no weights: " + L21_WEIGHTS_WHERE)
        self.seg_radii = False       # an l1 / l2 / annulus set per fiber or slice built with one radius per segment (in ub; lb: the annulus' inner radii)
        self.op = None               # the operator a stand-alone call of the projector acts behind (l21: the TV range), None: the identity
        if st == "l1_weighted":
            # the weighted l1 ball: one weight per row of a built-in operator (csrc/l1_weighted.h); max is the radius
            cust = constraint.custom_TD_OP[0]
            if not (isinstance(cust, (tuple, list)) and len(cust) == 0):
                raise SipxError(L1W_NO_CUSTOM)
            if constraint.TD_OP in SPECIAL_OPERATORS:
                raise SipxError(L1W_NO_TRANSFORM)
            if constraint.TD_OP not in L1W_OPERATORS:
                raise SipxError(L1W_NO_CUSTOM if constraint.TD_OP == "D_xz" else UNKNOWN_OPERATOR)
            if constraint.TD_OP == "TV_xy" and len(n) != 3:
                raise SipxError(TV_XY_NEEDS_3D)
            if constraint.TD_OP == "D_y" and len(n) == 2:
                raise SipxError(UNKNOWN_OPERATOR)
            if self.mode:
                raise SipxError(L1W_NO_MODE)
            if np.ndim(constraint.max) != 0:
                raise SipxError("the weighted l1 ball takes one radius (constraint.max a scalar)")
            if not float(constraint.max) > 0:
                raise SipxError("Radius of L1 ball is negative")
            if getattr(constraint, "weights", None) is None:
                raise SipxError(L1W_NEEDS_WEIGHTS)
            self.kind, self.pmax, self.op = "l1_weighted", float(constraint.max), constraint.TD_OP
            self._take_weights(constraint, TDOperator(constraint.TD_OP, comp_grid, self.TF).shape[0],
                               f"row of {constraint.TD_OP}, in the order of A @ x")
            return
        if st == "simplex":
            # entries >= 0 and min <= sum <= max on every fiber / slice of the range of a one-block operator (csrc/seg_simplex.h)
            cust = constraint.custom_TD_OP[0]
            if not (isinstance(cust, (tuple, list)) and len(cust) == 0):
                raise SipxError(SIMPLEX_ONE_BLOCK)
            if constraint.TD_OP in SPECIAL_OPERATORS:
                raise SipxError(SIMPLEX_NO_TRANSFORM)
            if constraint.TD_OP not in ONE_BLOCK_OPERATORS:
                raise SipxError(SIMPLEX_ONE_BLOCK)
            if constraint.TD_OP == "D_y" and len(n) == 2:
                raise SipxError(UNKNOWN_OPERATOR)
            if not self.mode:
                raise SipxError(SIMPLEX_NEEDS_MODE)
            if len(n) == 2 and self.mode == MODES["slice"]:
                raise SipxError(SIMPLEX_2D_SLICE)
            if np.ndim(constraint.max) != 0 or np.ndim(constraint.min) != 0:
                raise SipxError(SIMPLEX_NO_VECTORS)
            lo, hi = self.TF(constraint.min), self.TF(constraint.max)
            if not (lo >= 0 and lo <= hi and hi > 0 and np.isfinite(hi)):
                raise SipxError(SIMPLEX_BAD_BOUNDS)
            self.kind, self.pmin, self.pmax, self.op = "simplex", float(constraint.min), float(constraint.max), constraint.TD_OP
            return
        if st == "card_groups":
            # at most k = max non-zero fibers / slices of the range of a one-block operator (csrc/card_groups.h); min is ignored
            cust = constraint.custom_TD_OP[0]
            if not (isinstance(cust, (tuple, list)) and len(cust) == 0):
                raise SipxError(CARDG_ONE_BLOCK)
            if constraint.TD_OP in SPECIAL_OPERATORS:
                raise SipxError(CARDG_NO_TRANSFORM)
            if constraint.TD_OP not in ONE_BLOCK_OPERATORS:
                raise SipxError(CARDG_ONE_BLOCK)
            if constraint.TD_OP == "D_y" and len(n) == 2:
                raise SipxError(UNKNOWN_OPERATOR)
            if not self.mode:
                raise SipxError(CARDG_NEEDS_MODE)
            if len(n) == 2 and self.mode == MODES["slice"]:
                raise SipxError(CARDG_2D_SLICE)
            if np.ndim(constraint.max) != 0:
                raise SipxError(CARDG_NO_VECTORS)
            if int(np.prod(n)) >= 2 ** 31:
                raise SipxError(CARDG_TOO_LARGE)
            k = constraint.max
            if isinstance(k, (bool, np.bool_)) or not np.isfinite(float(k)) or float(k) != np.floor(float(k)) or float(k) < 1:
                raise SipxError(CARDG_BAD_K)
            self.kind, self.pmax, self.op = "card_groups", float(k), constraint.TD_OP
            if self.pmax < self.nseg(TDOperator(constraint.TD_OP, comp_grid, self.TF)) and float(self.TF(self.pmax)) != self.pmax:
                raise SipxError(CARDG_K_INEXACT)
            return
        if st == "l21_groups":
            # group sparsity: one l2,1 ball whose groups are the fibers / slices of the range of a one-block operator (csrc/l21_groups.h);
            # max is the radius, weights one per segment in the order of segment_norms()
            cust = constraint.custom_TD_OP[0]
            if not (isinstance(cust, (tuple, list)) and len(cust) == 0):
                raise SipxError(L21G_NO_CUSTOM)
            if constraint.TD_OP in SPECIAL_OPERATORS:
                raise SipxError(L21G_NO_TRANSFORM)
            if constraint.TD_OP not in ONE_BLOCK_OPERATORS:
                raise SipxError(L21G_ONE_BLOCK)
            if constraint.TD_OP == "D_y" and len(n) == 2:
                raise SipxError(UNKNOWN_OPERATOR)
            if not self.mode:
                raise SipxError(L21G_NEEDS_MODE)
            if len(n) == 2 and self.mode == MODES["slice"]:
                raise SipxError(L21G_2D_SLICE)
            if np.ndim(constraint.max) != 0:
                raise SipxError("the l2,1 ball over fibers or slices takes one radius (constraint.max a scalar): its segments share it")
            if not float(constraint.max) > 0:
                raise SipxError("Radius of L1 ball is negative")
            self.kind, self.pmax, self.op = "l21_groups", float(constraint.max), constraint.TD_OP
            tdn = list(n)
            if constraint.TD_OP != "identity":
                tdn[{"D_x": 0, "D_y": 1, "D_z": len(n) - 1}[constraint.TD_OP]] -= 1
            nseg = int(np.prod(tdn)) // int(tdn[self.dir]) if self.mode == MODES["fiber"] else int(tdn[self.dir])
            what = "fiber along" if self.mode == MODES["fiber"] else "slice orthogonal to"
            self._take_weights(constraint, nseg, f"segment, a segment being a {what} dimension {self.dir + 1} of the array of shape "
                                                 f"{tuple(tdn)} (TD_n), in the order of segment_norms()")
            return
        if st in ("l20", "l20_joint"):
            # at most k = max grid points (pixels) carry a gradient vector of TV / TV_xy (csrc/l20.h); min is ignored
            joint = st == "l20_joint"
            cust = constraint.custom_TD_OP[0]
            if constraint.TD_OP in SPECIAL_OPERATORS:
                raise SipxError(L20_NO_TRANSFORM)
            if not (isinstance(cust, (tuple, list)) and len(cust) == 0):
                raise SipxError(L20_JOINT_ROUTE if joint else L20_NEEDS_TV)
            if joint and (constraint.TD_OP != "TV_xy" or self.mode):
                raise SipxError(L20_JOINT_ROUTE)
            if constraint.TD_OP not in TV_OPERATORS + ("TV_xy",):
                raise SipxError(L20_NEEDS_TV)
            if constraint.TD_OP == "TV_xy" and len(n) != 3:
                raise SipxError(TV_XY_NEEDS_3D)
            if self.mode and not (constraint.TD_OP == "TV_xy" and (self.mode, self.dir) == (MODES["slice"], 2)):
                raise SipxError(L20_MODES)
            if np.ndim(constraint.min) != 0:
                raise SipxError(L20_NO_WEIGHTS)
            if int(np.prod(n)) >= 2 ** 31:
                raise SipxError(L20_TOO_LARGE)
            self.kind, self.op = st, ("TV_xy" if constraint.TD_OP == "TV_xy" else "TV")
            ngroups = int(n[0]) * int(n[1]) if (joint or self.mode) else int(np.prod(n))
            if np.ndim(constraint.max) != 0:
                if not self.mode or np.ndim(constraint.max) != 1:
                    raise SipxError(L20_K_VECTOR)
                ks = [_check_l20_k(k, ngroups, self.TF) for k in np.asarray(constraint.max).tolist()]
                self.seg_radii = True
                self.ub = np.ascontiguousarray(ks, self.TF)
                self.pmax = float(max(ks)) if ks else 1.0
            else:
                self.pmax = _check_l20_k(constraint.max, ngroups, self.TF)
            return
        if st in L2INF_KINDS:
            # every group norm at most max, one number or one per group (csrc/l2inf.h); ("l2inf", "Hessian") is the stacked set on the
            # named operator
            cust = constraint.custom_TD_OP[0]
            has_cust = not (isinstance(cust, (tuple, list)) and len(cust) == 0)
            if constraint.TD_OP in SPECIAL_OPERATORS:
                raise SipxError(L2INF_NO_TRANSFORM)
            stacked = st == "l2inf_stacked" or (st == "l2inf" and constraint.TD_OP == "Hessian" and not has_cust)
            if st == "l2inf_joint" and (has_cust or constraint.TD_OP != "TV_xy"):
                raise SipxError(L2INF_JOINT_ROUTE)
            if st == "l2inf_stacked" and not has_cust and constraint.TD_OP != "Hessian":
                raise SipxError(L2INF_STACKED_NEEDS_CSC)
            if st == "l2inf" and not stacked and (has_cust or constraint.TD_OP not in TV_OPERATORS + ("TV_xy",)):
                raise SipxError(L2INF_NEEDS_TV)
            if not stacked and constraint.TD_OP == "TV_xy" and len(n) != 3:
                raise SipxError(TV_XY_NEEDS_3D)
            if self.mode:
                raise SipxError(L2INF_MODES)
            if np.ndim(constraint.min) != 0:
                raise SipxError(L2INF_NO_WEIGHTS)
            if constraint.min != 0:
                raise SipxError(L2INF_MIN)
            if stacked:
                B = getattr(constraint, "blocks", None)
                if has_cust:
                    if B is None:
                        raise SipxError("the stacked l2,inf ball (l2inf_stacked) on a caller-supplied operator needs blocks, the number of "
                                        "its equal-sized blocks")
                    M = int(cust.shape[0])
                else:
                    _hessian_check_grid(n)
                    nb = len(n) * (len(n) + 1) // 2
                    if B is not None and int(B) != nb:
                        raise SipxError(f"the Hessian of this grid has {nb} blocks, blocks = {B} was given (leave it None)")
                    B, M = nb, nb * int(np.prod(n))
                if isinstance(B, (float, np.floating)) and B != int(B):
                    raise SipxError(l2inf_bad_blocks(B))
                B = int(B)
                if B < 1 or B > L21S_MAX_BLOCKS:
                    raise SipxError(l2inf_bad_blocks(B))
                if M % B:
                    raise SipxError(l2inf_bad_rows(M, B))
                self.kind, self.op, self.blocks, self.rows = "l2inf_stacked", "custom", B, M
                groups = per = M // B
            else:
                self.kind, self.op = st, ("TV_xy" if constraint.TD_OP == "TV_xy" else "TV")
                per = int(n[0]) * int(n[1]) if self.op == "TV_xy" else int(np.prod(n))
                groups = per if st == "l2inf_joint" else int(np.prod(n))
            self.groups, self.per = groups, per
            if np.ndim(constraint.max) != 0:
                c = np.ascontiguousarray(constraint.max, self.TF)
                if c.ndim != 1 or c.shape[0] != groups:
                    raise SipxError(l2inf_bad_length(int(c.size), groups))
                _check_l2inf_bounds(c, per, stacked)
                self.seg_radii, self.ub, self.pmax = True, c, 1.0
            else:
                if not float(constraint.max) > 0:
                    raise SipxError(L2INF_BAD_C)
                self.pmax = float(self.TF(constraint.max))
            return
        if st == "l21_stacked" or (st == "l21" and constraint.TD_OP == "Hessian"):
            # the l2,1 ball across the blocks of a stacked operator (csrc/l21_stacked.h); ("l21", "Hessian"): second-order isotropic TV
            cust = constraint.custom_TD_OP[0]
            has_cust = not (isinstance(cust, (tuple, list)) and len(cust) == 0)
            if getattr(constraint, "weights", None) is not None or np.ndim(constraint.max) != 0 or np.ndim(constraint.min) != 0:
                raise SipxError(L21S_NO_VECTORS)
            if constraint.TD_OP in SPECIAL_OPERATORS:
                raise SipxError(L21S_NO_TRANSFORM)
            if st == "l21" and has_cust:
                raise SipxError(L21_NEEDS_TV)
            if not has_cust and constraint.TD_OP != "Hessian":
                raise SipxError(L21S_NEEDS_CSC)
            if self.mode:
                raise SipxError(L21S_WHOLE_ONLY)
            B = getattr(constraint, "blocks", None)
            if has_cust:
                if B is None:
                    raise SipxError("the stacked l2,1 ball (l21_stacked) on a caller-supplied operator needs blocks, the number of its "
                                    "equal-sized blocks")
                M = int(cust.shape[0])
            else:
                _hessian_check_grid(n)
                nb = len(n) * (len(n) + 1) // 2
                if B is not None and int(B) != nb:
                    raise SipxError(f"the Hessian of this grid has {nb} blocks, blocks = {B} was given (leave it None)")
                B, M = nb, nb * int(np.prod(n))
            if isinstance(B, (float, np.floating)) and B != int(B):
                raise SipxError(l21s_bad_blocks(B))
            B = int(B)
            if B < 1 or B > L21S_MAX_BLOCKS:
                raise SipxError(l21s_bad_blocks(B))
            if M % B:
                raise SipxError(l21s_bad_rows(M, B))
            if not float(constraint.max) > 0:
                raise SipxError("Radius of L1 ball is negative")
            self.kind, self.pmax, self.op, self.blocks, self.rows = "l21_stacked", float(constraint.max), "custom", B, M
            return
        if st == "l21_joint":
            # joint (vectorial) total variation: one group per pixel across the frames of TV_xy (csrc/l21_joint.h); max is the radius
            cust = constraint.custom_TD_OP[0]
            if constraint.TD_OP != "TV_xy" or not (isinstance(cust, (tuple, list)) and len(cust) == 0):
                raise SipxError(L21_JOINT_NEEDS_TV_XY)
            if len(n) != 3:
                raise SipxError(TV_XY_NEEDS_3D)
            if self.mode:
                raise SipxError(L21_JOINT_NEEDS_TV_XY)
            if np.ndim(constraint.max) != 0:
                raise SipxError("the joint l2,1 ball takes one radius (constraint.max a scalar)")
            if not float(constraint.max) > 0:
                raise SipxError("Radius of L1 ball is negative")
            self.kind, self.pmax, self.op = "l21_joint", float(constraint.max), "TV_xy"
            self._take_weights(constraint, int(n[0]) * int(n[1]), "pixel (n1 n2, pixel order)")
            return
        if st == "l21":
            # isotropic total variation: the l2,1 ball on the range of the TV operator (csrc/l21.h); max is the radius
            cust = constraint.custom_TD_OP[0]
            if constraint.TD_OP not in TV_OPERATORS + ("TV_xy",) or not (isinstance(cust, (tuple, list)) and len(cust) == 0):
                raise SipxError(L21_NEEDS_TV)
            if constraint.TD_OP == "TV_xy":
                # on the in-plane gradient of a 3-D grid: the whole array, or every z-slice on its own (csrc/l21_seg.h) with one
                # radius for all frames or a vector of n3
                if len(n) != 3:
                    raise SipxError(TV_XY_NEEDS_3D)
                if self.mode and (self.mode, self.dir) != (MODES["slice"], 2):
                    raise SipxError(L21_FRAMES_Z)
                if np.ndim(constraint.max) > (1 if self.mode else 0):
                    raise SipxError("the l2,1 ball on TV_xy takes one radius, or per frame a vector of n3 (constraint.max)")
                self.kind, self.op = "l21", "TV_xy"
                if self.mode and getattr(constraint, "weights", None) is not None:
                    raise SipxError(L21_WEIGHTS_NO_FRAMES)
                if not self.mode:
                    self._take_weights(constraint, int(np.prod(n)), "grid point (column-major order)")
                if np.ndim(constraint.max) == 1:
                    self.seg_radii = True
                    self.ub = np.ascontiguousarray(constraint.max, self.TF)
                    _check_l1_radii("l1", self.ub)
                    self.pmax = float(self.ub.max()) if len(self.ub) else 0.0
                else:
                    if not float(constraint.max) > 0:
                        raise SipxError("Radius of L1 ball is negative")
                    self.pmax = float(constraint.max)
                return
            if self.mode:
                raise SipxError(L21_WHOLE_ONLY)
            if np.ndim(constraint.max) != 0:
                raise SipxError("the l2,1 ball takes one radius (constraint.max a scalar)")
            if not float(constraint.max) > 0:
                raise SipxError("Radius of L1 ball is negative")
            self.kind, self.pmax, self.op = "l21", float(constraint.max), "TV"
            self._take_weights(constraint, int(np.prod(n)), "grid point (column-major order)")
            return
        if constraint.TD_OP == "DCT":
            # x -> C' P(C x) with the orthonormal DCT-II (get_projector.jl, special_operator_list branches); the l2 ball and
            # the annulus commute with an orthogonal transform and are applied to x itself
            if st in ("l2", "annulus"):
                self.kind, self.pmax = st, float(constraint.max)
                self.pmin = float(constraint.min) if st == "annulus" else 0.0
            elif st in ("l1", "cardinality"):
                self.kind, self.pmax, self.transform = st, float(constraint.max), TRANSFORMS["DCT"]
            elif st == "bounds" and np.ndim(constraint.min) == 0:
                self.kind, self.pmin, self.pmax, self.transform = "bounds", float(constraint.min), float(constraint.max), TRANSFORMS["DCT"]
            elif st == "bounds":
                self.kind, self.transform = "bounds_vec", TRANSFORMS["DCT"]
                self.lb = np.ascontiguousarray(constraint.min, self.TF)
                self.ub = np.ascontiguousarray(constraint.max, self.TF)
            else:
                raise SipxError(f"set type {st!r} behind the DCT is not built")
            if self.mode:
                raise SipxError("sets behind the DCT apply to the whole array (matrix / tensor mode)")
        elif constraint.TD_OP == "wavelet":
            # x -> W' P(W x) with the orthonormal periodic db4 transform (sipx.h, SIPX_TRANSFORM_WAVELET); the l2 ball and the
            # annulus commute with it and are applied to x itself
            if st in ("l2", "annulus"):
                self.kind, self.pmax = st, float(constraint.max)
                self.pmin = float(constraint.min) if st == "annulus" else 0.0
            elif st == "l1":
                self.kind, self.pmax, self.transform = st, float(constraint.max), TRANSFORMS["wavelet"]
            elif st == "cardinality":
                self.kind, self.pmax, self.transform = st, float(int(constraint.max)), TRANSFORMS["wavelet"]
            elif st == "bounds" and np.ndim(constraint.min) == 0:
                self.kind, self.pmin, self.pmax, self.transform = "bounds", float(constraint.min), float(constraint.max), TRANSFORMS["wavelet"]
            else:
                raise SipxError(f"set type {st!r} behind the wavelet transform is not built: scalar bounds, l1, cardinality, "
                                "l2 and annulus are")
            if self.mode:
                raise SipxError("sets behind the wavelet transform apply to the whole array (matrix / tensor mode)")
            if self.transform:
                _dwt_check_grid(n)
        elif constraint.TD_OP in SPECIAL_OPERATORS:
            if constraint.TD_OP == "DFT" and st == "l1":
                self.kind, self.pmax = "l1_dft", float(constraint.max)
            elif constraint.TD_OP == "DFT" and st == "bounds" and np.ndim(constraint.min) == 1:
                lb = np.asarray(constraint.min)
                ub = np.ascontiguousarray(constraint.max, self.TF)
                if np.any(lb != 0) or len(np.unique(ub)) != 2:        # project_bounds!.jl:31-32 (@assert)
                    raise SipxError("bounds in the DFT domain: LB must be all zeros and UB a two-valued mask")
                self.kind, self.ub = "bounds_dft", ub
            elif constraint.TD_OP == "DFT" and st in ("l2", "annulus"):
                # ||F x||_2 = ||x||_2 for the unitary DFT and the projection is a rescaling (or, for the zero vector of an
                # annulus, a constant fill whose DC-only spectrum transforms back to a constant): x -> Re(F' P(F x)) is
                # P applied to x itself, without the FFT round trip of get_projector.jl:39,47
                self.kind, self.pmax = st, float(constraint.max)
                self.pmin = float(constraint.min) if st == "annulus" else 0.0
            elif constraint.TD_OP == "DFT" and st == "cardinality":
                # x -> Re(F' project_cardinality!(F x, k)) (get_projector.jl:85-89): the k Fourier coefficients of largest
                # magnitude, conjugate pairs as exact ties (sipx.h, SIPX_PROJ_CARD_DFT)
                if self.mode:
                    raise SipxError("cardinality behind the DFT applies to the whole array (matrix / tensor mode)")
                k = float(constraint.max)
                if k != int(k):                          # convert(Integer, constraint.max), get_projector.jl:88
                    raise SipxError(f"InexactError: Int64({constraint.max!r})")
                if k < 0:                                # sort_ind[k+1:end] (project_cardinality!.jl:19)
                    raise SipxError(f"cardinality behind the DFT: k = {int(k)} is negative (BoundsError: sort_ind[{int(k) + 1}:end])")
                self.kind, self.pmax = "card_dft", k
            else:
                raise SipxError("of the orthogonal-transform sets only the l1 ball, cardinality (matrix / tensor mode), masking "
                                "bounds, the l2 ball and the annulus in the DFT domain are built")
        elif st == "rank":
            self.kind, self.pmax = "rank", float(int(constraint.max))
        elif st == "nuclear":
            self.kind, self.pmax = "nuclear", float(constraint.max)
        elif st == "bounds":
            if np.ndim(constraint.min) == 0:
                self.kind, self.pmin, self.pmax = "bounds", float(constraint.min), float(constraint.max)
            else:
                self.kind = "bounds_vec"
                self.lb = np.ascontiguousarray(constraint.min, self.TF)
                self.ub = np.ascontiguousarray(constraint.max, self.TF)
        elif st == "histogram":
            self.kind = "histogram"
            self.lb = np.ascontiguousarray(constraint.min, self.TF)
            self.ub = np.ascontiguousarray(constraint.max, self.TF)
        elif st == "subspace":
            A, orth = constraint.custom_TD_OP
            self.kind = "subspace"
            self.basis = np.asfortranarray(A, dtype=self.TF)
            if self.basis.ndim != 2:
                raise SipxError("subspace constraints need a matrix A in custom_TD_OP[0]")
            self.basis_orth = bool(orth)
        elif self.mode and st in ("l1", "l2", "annulus") and (np.ndim(constraint.max) or (st == "annulus" and np.ndim(constraint.min))):
            self._segment_radii(st, constraint)
        elif st in ("l1", "l2", "prox_l1"):
            self.kind, self.pmax = st, float(constraint.max)
        elif st == "annulus":
            self.kind, self.pmin, self.pmax = st, float(constraint.min), float(constraint.max)
        elif st == "cardinality":
            self.kind, self.pmax = st, float(int(constraint.max))
        else:
            raise SipxError(f"set type {st!r} is not part of this engine")

    def _take_weights(self, constraint, groups, what):
        """constraint.weights of an l2,1 set on the whole array: a 1-D numpy vector of the working precision with one finite weight >= 0
        per group, kept as lb (csrc/l21_weighted.h).  None: the plain ball."""
        w = getattr(constraint, "weights", None)
        if w is None:
            return
        name = f"{constraint.set_type} weights"
        if not isinstance(w, np.ndarray):
            raise SipxError(f"{name} must be a numpy array, not {type(w).__name__}")
        if w.dtype.type != self.TF:
            raise SipxError(f"{name} have dtype {w.dtype}: not the working precision ({np.dtype(self.TF).name})")
        if w.shape != (groups,):
            raise SipxError(f"{name} have shape {w.shape}: ({groups},) is needed -- one per {what}")
        _check_l21_weights(constraint.set_type, w)
        self.lb, self.weighted = np.ascontiguousarray(w), True

    def _segment_radii(self, st, constraint):
        """One radius per segment (csrc/seg_norm.h): max -- and for the annulus min and / or max -- a vector of nseg entries in the order of
        segment_norms(); a scalar beside a vector is repeated.  The length is checked against the operator in check_rows."""
        vec = {}
        for name, a in (("min", constraint.min), ("max", constraint.max)):
            if name == "min" and st != "annulus":
                continue
            if np.ndim(a) > 1:
                raise SipxError(f"{st} radii per segment: {name} must be a scalar or a 1-D vector, not of shape {np.shape(a)}")
            vec[name] = np.ascontiguousarray(a, self.TF) if np.ndim(a) == 1 else None
        length = max(len(v) for v in vec.values() if v is not None)
        for name, a in (("min", constraint.min), ("max", constraint.max)):
            if name in vec and vec[name] is None:
                vec[name] = np.full(length, self.TF(a), self.TF)
        self.kind, self.seg_radii = st, True
        self.ub, self.lb = vec["max"], vec.get("min")
        _check_l1_radii(st, self.ub)
        self.pmax = float(self.ub.max()) if len(self.ub) else 0.0
        self.pmin = float(self.lb.min()) if self.lb is not None and len(self.lb) else 0.0

    def nseg(self, op) -> int:
        """Fibers / slices of the array of shape TD_n this set splits behind operator `op` (0: a whole-array set)."""
        if not self.mode:
            return 0
        n = list(op.n)
        if self.kind in ("l21", "l20"):          # frames of the grid itself
            return int(n[2])
        if op.kind in ("D_x", "D_y", "D_z"):
            n[{"D_x": 0, "D_y": 1, "D_z": len(n) - 1}[op.kind]] -= 1
        return int(np.prod(n)) // int(n[self.dir]) if self.mode == MODES["fiber"] else int(n[self.dir])

    def check_rows(self, op: "TDOperator"):
        """Host-side shape checks of the vectors the descriptor points at (the engine reads them unchecked)."""
        n = list(op.n)
        if self.kind == "l21" and (op.kind != "TV_xy" if self.op == "TV_xy" else op.kind not in TV_OPERATORS):
            raise SipxError(L21_NEEDS_TV)
        if self.kind == "l21_joint" and op.kind != "TV_xy":
            raise SipxError(L21_JOINT_NEEDS_TV_XY)
        if self.kind == "tnv" and op.kind != "TV_xy":
            raise SipxError(TNV_NEEDS_TV_XY)
        if self.kind == "l20" and (op.kind != "TV_xy" if self.op == "TV_xy" else op.kind not in TV_OPERATORS):
            raise SipxError(L20_NEEDS_TV)
        if self.kind == "l20_joint" and op.kind != "TV_xy":
            raise SipxError(L20_JOINT_ROUTE)
        if self.kind in ("l20", "l20_joint") and getattr(op, "component", 0):
            raise SipxError(L20_NO_MINKOWSKI)
        if self.kind == "l21_groups":
            if op.kind == "custom":
                raise SipxError(L21G_NO_CUSTOM)
            if op.kind != self.op:
                raise SipxError(L21G_ONE_BLOCK + f" -- this set was built for {self.op}, the operator is {op.kind}")
            if getattr(op, "component", 0):
                raise SipxError(L21G_NO_MINKOWSKI)
        if self.kind == "card_groups":
            if op.kind != self.op:
                raise SipxError(CARDG_ONE_BLOCK + f" -- this set was built for {self.op}, the operator is {op.kind}")
            if getattr(op, "component", 0):
                raise SipxError(CARDG_NO_MINKOWSKI)
        if self.kind == "simplex":
            if op.kind != self.op:
                raise SipxError(SIMPLEX_ONE_BLOCK + f" -- this set was built for {self.op}, the operator is {op.kind}")
            if getattr(op, "component", 0):
                raise SipxError(SIMPLEX_NO_MINKOWSKI)
        if self.kind == "l2inf" and (op.kind != "TV_xy" if self.op == "TV_xy" else op.kind not in TV_OPERATORS):
            raise SipxError(L2INF_NEEDS_TV)
        if self.kind == "l2inf_joint" and op.kind != "TV_xy":
            raise SipxError(L2INF_JOINT_ROUTE)
        if self.kind in L2INF_KINDS and getattr(op, "component", 0):
            raise SipxError(L2INF_NO_MINKOWSKI)
        if self.kind == "l2inf_stacked":
            if op.kind != "custom":
                raise SipxError(L2INF_STACKED_NEEDS_CSC)
            if int(op.shape[0]) % self.blocks:
                raise SipxError(l2inf_bad_rows(int(op.shape[0]), self.blocks))
            if int(op.shape[0]) != self.rows:
                raise SipxError(l2inf_bad_length(self.groups, int(op.shape[0]) // self.blocks))
        if self.kind in L2INF_KINDS and self.seg_radii and self.ub.shape != (self.groups,):
            raise SipxError(l2inf_bad_length(int(self.ub.shape[0]), self.groups))
        if self.kind == "l21_stacked":
            if op.kind != "custom":
                raise SipxError(L21S_NEEDS_CSC)
            if getattr(op, "component", 0):
                raise SipxError(L21S_NO_MINKOWSKI)
            if self.blocks < 1 or self.blocks > L21S_MAX_BLOCKS:
                raise SipxError(l21s_bad_blocks(self.blocks))
            if int(op.shape[0]) % self.blocks:
                raise SipxError(l21s_bad_rows(int(op.shape[0]), self.blocks))
        if self.kind == "l1_weighted":
            if op.kind == "custom":
                raise SipxError(L1W_NO_CUSTOM)
            if OPS[op.kind] != OPS[self.op]:
                raise SipxError(f"the weighted l1 ball (l1_weighted) was built with one weight per row of {self.op}, the operator is {op.kind}")
            if getattr(op, "component", 0):
                raise SipxError(L1W_NO_MINKOWSKI)
        if op.kind == "custom" and (self.mode or self.transform or self.kind in ("l1_dft", "bounds_dft", "card_dft", "rank",
                                                                                     "nuclear", "histogram", "subspace")):
            raise SipxError("custom sparse operators take the whole-array projectors only")
        if op.kind in ("D_x", "D_y", "D_z"):
            n[{"D_x": 0, "D_y": 1, "D_z": len(n) - 1}[op.kind]] -= 1
        rows = op.shape[0]
        if self.kind == "bounds_vec":
            if self.mode == MODES["slice"]:
                raise SipxError("bound constraints per slice of a tensor currently not implemented, yet...")
            want = n[self.dir] if self.mode == MODES["fiber"] else rows
            if self.lb.shape != (want,) or self.ub.shape != (want,):
                raise SipxError(f"bounds vectors need {want} entries for this operator / application mode")
        if self.kind in L2INF_KINDS:
            pass                                   # (checked above)
        elif self.seg_radii and self.kind == "l20":
            if self.ub.shape != (n[2],):
                raise SipxError(f"l20 budgets per frame: max has {self.ub.shape[0]} entries, n3 = {n[2]} are needed -- one per z-slice "
                                f"of the grid of shape {tuple(n)}")
        elif self.seg_radii and self.kind == "l21":
            if self.ub.shape != (n[2],):
                raise SipxError(f"l21 radii per frame: max has {self.ub.shape[0]} entries, n3 = {n[2]} are needed -- one per z-slice "
                                f"of the grid of shape {tuple(n)}")
        elif self.seg_radii:
            want = self.nseg(op)
            for name, a in (("min", self.lb), ("max", self.ub)):
                if a is not None and a.shape != (want,):
                    what = "fiber along" if self.mode == MODES["fiber"] else "slice orthogonal to"
                    raise SipxError(f"{self.kind} radii per segment: {name} has {a.shape[0]} entries, nseg = {want} are needed -- one per "
                                    f"segment, a segment being a {what} dimension {self.dir + 1} of the array of shape {tuple(n)} (TD_n)")
        if self.kind == "bounds_dft" and self.ub.shape != (rows,):
            raise SipxError(f"the DFT-domain mask needs {rows} entries")
        if self.kind == "histogram" and (self.lb.shape != (rows,) or self.ub.shape != (rows,)):
            raise SipxError(f"histogram bounds need {rows} sorted entries")

    def data_len(self, op) -> Optional[int]:
        """Entries of each vector sipx_set_data takes for this set behind operator `op`; None: the set holds no replaceable data."""
        if self.kind == "histogram":
            return int(op.shape[0])
        if self.weighted:
            return int(self.lb.shape[0])
        if self.seg_radii and self.kind in L2INF_KINDS:
            return int(self.groups)
        if self.seg_radii:
            return self.nseg(op)
        if self.kind != "bounds_vec" or self.transform:
            return None
        if self.mode != MODES["fiber"]:
            return int(op.shape[0])
        n = list(op.n)
        if op.kind in ("D_x", "D_y", "D_z"):
            n[{"D_x": 0, "D_y": 1, "D_z": len(n) - 1}[op.kind]] -= 1
        return int(n[self.dir])

    def desc(self, op: str, ncvx: bool) -> _SetDesc:
        d = _SetDesc()
        d.op, d.proj = OPS[op], PROJ[self.kind]
        d.pmin, d.pmax = self.pmin, self.pmax
        d.lb, d.ub = _ptr(self.lb), _ptr(self.ub)
        d.ncvx, d.reserved = int(bool(ncvx)), (int(self.lb.shape[0]) if self.weighted else 0)
        if self.kind in L2INF_KINDS and self.seg_radii:
            d.reserved = int(self.ub.shape[0])       # (the entries ub holds)
        d.mode, d.dir = self.mode, self.dir
        d.transform = self.transform
        d.blocks = self.blocks
        if self.basis is not None:
            d.basis, d.basis_rows, d.basis_cols = _ptr(self.basis), self.basis.shape[0], self.basis.shape[1]
            d.basis_orth = int(self.basis_orth)
        return d

    def __call__(self, v):
        if v.dtype.type != self.TF or not v.flags.c_contiguous:
            raise SipxError("projector input must be a contiguous vector of the working precision")
        grid_kind = self.mode != 0 or self.transform != 0 or self.kind in ("l1_dft", "bounds_dft", "card_dft", "rank", "nuclear", "histogram",
                                                                              "subspace", "l21", "l21_joint", "l21_groups", "tnv", "l1_weighted",
                                                                              "simplex", "card_groups", "l20", "l20_joint", "l2inf", "l2inf_joint")
        l21 = self.kind in ("l21", "l21_joint", "l21_groups", "tnv", "l1_weighted", "simplex", "card_groups", "l20", "l20_joint", "l2inf",
                            "l2inf_joint")
        if self.kind in ("l21_stacked", "l2inf_stacked"):      # the M-vector of the stacked operator's range itself: blocks blocks of M / blocks entries
            if v.shape != (self.rows,):
                what = "l2,1" if self.kind == "l21_stacked" else "l2,inf"
                raise SipxError(f"the stacked {what} ball projects a vector of the operator's range: {self.rows} entries, {v.size} given")
            ctx = Context(self.comp_grid, self.TF)
            try:
                d = self.desc("custom", False)
                _chk(lib().sipx_project(ctx.h, C.byref(d), _ptr(v), C.c_int64(len(v))))
            finally:
                ctx.close()
            return v
        if l21:                      # the M-vector of the TV range (l21_groups: of its operator's) in the reference's row order, on the grid
            op = TDOperator(self.op, self.comp_grid, self.TF)
            rows = op.shape[0]
            if v.shape != (rows,):
                what = {"l1_weighted": "weighted l1 ball", "simplex": "simplex set", "card_groups": "group cardinality set", "l20": "l2,0 set",
                        "l20_joint": "l2,0 set", "l2inf": "l2,inf ball", "l2inf_joint": "l2,inf ball"}.get(self.kind, "l2,1 ball")
                raise SipxError(f"the {what} projects a vector of the {self.op} range: {rows} entries on this grid, {v.size} given")
            self.check_rows(op)
        ctx = Context(self.comp_grid if grid_kind else compgrid((1.0, 1.0), (max(len(v), 1), 1)), self.TF)
        try:
            if l21:
                d = self.desc(self.op, False)
                _chk(lib().sipx_project(ctx.h, C.byref(d), _ptr(v), C.c_int64(len(v))))
                return v
            if grid_kind:
                self.check_rows(TDOperator("identity", self.comp_grid, self.TF))
            elif self.kind == "bounds_vec" and (self.lb.shape != v.shape or self.ub.shape != v.shape):
                raise SipxError("bounds vectors must match the projected vector")
            d = self.desc("identity", False)
            _chk(lib().sipx_project(ctx.h, C.byref(d), _ptr(v), C.c_int64(len(v))))
        finally:
            ctx.close()
        return v


# --------------------------------------------------------------------------------------------------
# one-off setup
# --------------------------------------------------------------------------------------------------
def get_TD_operator(comp_grid, TD_type: str, TF):
    """src/get_TD_operator.jl:12-95 for the banded operators."""
    n, _ = _grid(comp_grid)
    if TD_type in ("DFT", "DCT", "wavelet"):   # src/get_TD_operator.jl:45-51,80-88; setup_constraints.jl:76-80 swaps in the identity
        return TDOperator("identity", comp_grid, TF), True, True, n, False
    if TD_type == "D_xz":      # src/get_TD_operator.jl:66-70 (2-D only): TD_OP = D_z * D_x, shipped as a sparse matrix
        if len(n) != 2:
            raise SipxError("provided an unknown transform domain operator. check function "
                            "get_TD_operator(comp_grid,TD_type,TF) for options")
        import scipy.sparse as sp
        TFt = np.dtype(TF).type
        _, h = _grid(comp_grid)

        def fwd(k, hk):       # (k-1) x k forward difference with entries -+fl(1/h)   (get_discrete_Grad.jl:22-23)
            ih = TFt(1) / TFt(hk)
            return sp.diags([np.full(k - 1, -ih, TFt), np.full(k - 1, ih, TFt)], [0, 1], shape=(k - 1, k), dtype=TFt, format="csc")
        n1, n2 = n
        Dx = sp.kron(sp.identity(n2, dtype=TFt, format="csc"), fwd(n1, h[0]), format="csc")            # on (n1, n2)
        Dz = sp.kron(fwd(n2, h[1]), sp.identity(n1 - 1, dtype=TFt, format="csc"), format="csc")        # on (n1-1, n2)
        return CustomOperator((Dz @ Dx).astype(TFt), comp_grid, TF), False, False, (n1 - 1, n2 - 1), True
    if TD_type == "Hessian":
        return hessian_operator(comp_grid, TF), False, False, n, True
    if TD_type == "TV_xy" and len(n) != 3:
        raise SipxError(TV_XY_NEEDS_3D)
    A = TDOperator(TD_type, comp_grid, TF)
    if TD_type == "identity":
        return A, True, False, n, True
    if len(n) == 2:
        n1, n2 = n
        TD_n = {"TV": ((n1 - 1) + n1, n2 + (n2 - 1)), "D2D": ((n1 - 1) + n1, n2 + (n2 - 1)), "D_z": (n1, n2 - 1),
                "D_x": (n1 - 1, n2)}[TD_type]
    else:
        n1, n2, n3 = n
        TD_n = {"TV": (3 * n1 - 1, 3 * n2 - 1, 3 * n3 - 1), "D3D": (3 * n1 - 1, 3 * n2 - 1, 3 * n3 - 1),
                "D_z": (n1, n2, n3 - 1), "D_y": (n1, n2 - 1, n3), "D_x": (n1 - 1, n2, n3),
                "TV_xy": (2 * n1 - 1, 2 * n2 - 1, n3)}[TD_type]      # (bookkeeping only, as the TV entries are)
    return A, False, False, TD_n, True


def _hessian_check_grid(n):
    if len(n) not in (2, 3) or min(n) < 3:
        raise SipxError(HESSIAN_SMALL_GRID.format(n=tuple(n)))


def hessian_operator(comp_grid, TF):
    """The named operator "Hessian" (csrc/l21_stacked.h): a CustomOperator of B N rows, B = 3 on a 2-D grid (D_11, D_22, sqrt(2) D_12)
    and 6 on a 3-D one (D_11, D_22, D_33, sqrt(2) D_12, sqrt(2) D_13, sqrt(2) D_23); row q N + p is entry q of the Hessian at grid
    point p, a zero row where the stencil leaves the grid.  Assembled in TF from the forward-difference factors -+fl(1/h) of D_xz:
    D_aa = the product of two of them, (x[i-1] - 2 x[i] + x[i+1]) ih_a^2 centred at 1 <= i <= n_a - 2; D_ab = the forward difference
    along a of the forward difference along b that starts at p (the reference's D_z * D_x), scaled by fl(sqrt(2)) so that the group
    norm is the Frobenius norm of the symmetric Hessian."""
    import scipy.sparse as sp
    n, h = _grid(comp_grid)
    _hessian_check_grid(n)
    TFt = np.dtype(TF).type
    nd = len(n)

    def fwd(k, hk):       # (k-1) x k forward difference with entries -+fl(1/h)   (get_discrete_Grad.jl:22-23)
        ih = TFt(1) / TFt(hk)
        return sp.diags([np.full(k - 1, -ih, TFt), np.full(k - 1, ih, TFt)], [0, 1], shape=(k - 1, k), dtype=TFt, format="csc")

    def rows_into(k, first, count):      # k x count: row first + i takes row i (the other rows stay empty)
        return sp.csc_matrix((np.ones(count, TFt), (np.arange(count) + first, np.arange(count))), shape=(k, count), dtype=TFt)

    def along(factors):      # the operator on the grid from one k x k factor per axis (column-major: axis 0 fastest)
        out = factors[0]
        for f in factors[1:]:
            out = sp.kron(f, out, format="csc")
        return out.astype(TFt)
    eye = [sp.identity(k, dtype=TFt, format="csc") for k in n]
    first = [(rows_into(k, 0, k - 1) @ fwd(k, hk)).astype(TFt) for k, hk in zip(n, h)]               # starts at i, empty last row
    second = [(rows_into(k, 1, k - 2) @ (fwd(k - 1, hk) @ fwd(k, hk))).astype(TFt) for k, hk in zip(n, h)]   # centred at i, empty first and last row
    blocks = [along([second[c] if c == a else eye[c] for c in range(nd)]) for a in range(nd)]
    r2 = TFt(np.sqrt(TFt(2)))
    for a in range(nd):
        for b in range(a + 1, nd):
            D = along([first[c] if c in (a, b) else eye[c] for c in range(nd)])
            blocks.append((D * r2).astype(TFt))
    H = sp.vstack(blocks, format="csc", dtype=TFt)
    H.eliminate_zeros()
    op = CustomOperator(H, comp_grid, TF)
    op.named = "Hessian"
    return op


def setup_constraints(constraint: List[set_definitions], comp_grid, TF, segment_norms=False):
    """src/setup_constraints.jl:17-102 -> (P_sub, TD_OP, set_Prop).

    segment_norms=True takes l1, l2 and annulus sets with app_mode ("fiber", d) / ("slice", d): every fiber along d (slice
    orthogonal to d) of the array of shape TD_n is projected on its own, on the identity, D_x, D_y or D_z -- all with the scalar
    min / max, or each with its own: max (for the annulus min and / or max) a vector of nseg entries in the order segment_norms()
    returns them, a scalar beside a vector repeated.  The reference has no such projector ("only available for matrix or tensor mode, currently"); without the keyword its
    error stays.

    ("l21", "TV") in matrix / tensor mode -- isotropic total variation, the l2,1 ball of radius max on the TV range (csrc/l21.h) --
    is the engine's own too and needs no keyword: the reference has no error to preserve there.  So are ("l21", "TV_xy") on the
    in-plane gradient of a 3-D grid -- the whole array or per z-slice (csrc/l21_seg.h) -- and ("l21_joint", "TV_xy") in tensor mode,
    the ball whose groups span the frames: one budget on the sum over pixels of the l2 norm of all in-plane differences at that
    pixel in all frames (vectorial total variation, csrc/l21_joint.h).  ("tnv", "TV_xy") in tensor mode is total nuclear variation
    (csrc/tnv.h): one budget on the sum over the pixels of the nuclear norm of the 2 x n3 matrix of that pixel's in-plane gradients in
    all frames, so that the frames share the direction of their gradients and not only where the edges are; it takes no weights.

    ("l21_groups", op, ("fiber", d) / ("slice", d)) on the identity, D_x, D_y or D_z is group sparsity (csrc/l21_groups.h): ONE ball of
    radius max on the sum over the fibers / slices of the array of shape TD_n of their l2 norms, optionally with one weight per segment
    (weights, in the order of segment_norms()).  ("l2", op, same mode) gives every segment a ball of its own instead.

    ("l1_weighted", op, matrix / tensor) on the identity, D_x, D_y, D_z, TV or TV_xy is the weighted l1 ball (csrc/l1_weighted.h):
    sum_i w_i |(A x)_i| <= max with one finite weight >= 0 per row of A in the order of A @ x (weights, required; 0 leaves a row free) --
    the set of iteratively reweighted l1 and of anisotropic TV with a weight per direction.

    ("simplex", op, min, max, ("fiber", d) / ("slice", d)) on the identity, D_x, D_y or D_z makes every fiber / slice of the array of shape
    TD_n nonnegative with a sum in [min, max] (csrc/seg_simplex.h): min = max = 1 is the probability simplex of material fractions and
    class probabilities along the frame axis, min = 0 the capped one; one pair of scalars for all segments.  segment_sums() observes the
    sums.

    ("card_groups", op, 0, k, ("fiber", d) / ("slice", d)) on the identity, D_x, D_y or D_z is group cardinality (csrc/card_groups.h): at
    most k fibers / slices of the array of shape TD_n are non-zero -- "at most k traces change" on D_z per fiber z, "at most k frames are
    active" on the identity per slice z.  The non-convex counterpart of l21_groups (ncvx is set, as for cardinality and rank): the k
    segments of largest l2 norm stay as they are, ties to the lower segment index, the others become zero.  k is an integer >= 1; min is
    ignored.  group_norms() observes the norms it selects on.

    ("l20", "TV" | "TV_xy", 0, k, ("matrix" | "tensor", "")) is the l2,0 set on total variation (csrc/l20.h), L0 gradient smoothing: at most
    k grid points carry a non-zero gradient vector -- a piecewise-constant model with at most k edge points whose edges keep their
    contrast.  ("l20", "TV_xy", 0, k, ("slice", "z")) gives every frame its own budget, k one integer or a vector of n3 (replaceable with
    Solver.set_data as ub); ("l20_joint", "TV_xy", 0, k, ("tensor", "")) lets at most k pixels carry an edge in any frame, one common edge
    set.  The non-convex counterparts of the l21 / l21_joint sets (ncvx is set): the k groups of largest norm stay as they are, ties to
    the lower point index, every member of the others becomes zero.  ("cardinality", "TV") is another set: it counts differences, so a
    diagonal edge costs two.  tv_group_norms() observes the norms it selects on.

    ("l2inf", "TV" | "TV_xy", 0, c, ("matrix" | "tensor", "")) is the l2,inf ball on total variation (csrc/l2inf.h): the gradient magnitude
    ||grad x(p)||_2 <= c_p at every grid point, the rotation-invariant slope constraint (("bounds", "TV") bounds every direction on its
    own).  c is one positive number or a vector with one bound >= 0 per grid point in the order of tv_group_norms() (+inf frees a point,
    0 flattens it; replaceable with Solver.set_data as ub).  ("l2inf_joint", "TV_xy", 0, c, ("tensor", "")) bounds the norm of a pixel's
    in-plane differences across all frames (c: a scalar or n1 n2 numbers); ("l2inf", "Hessian", 0, c, mode) and ("l2inf_stacked", name,
    0, c, mode, custom_TD_OP=(A, False), blocks=B) bound the group norms across the blocks of a stacked operator (c: a scalar or one per
    row of a block).  min must be 0.  l2inf_norm() observes the largest group norm."""
    TF = np.dtype(TF).type
    P_sub, TD_OP, prop = [], [], set_properties()
    for c in constraint:
        seg = segment_norms and c.set_type in ("l1", "l2", "annulus") and c.app_mode[0] in ("slice", "fiber")
        if seg and np.ndim(c.min) != np.ndim(c.max):      # radii per segment: a scalar beside a vector, each converted on its own
            c.min, c.max = [np.asarray(a, TF) if np.ndim(a) else (TF(a) if isinstance(a, (float, np.floating)) else a) for a in (c.min, c.max)]
        elif c.set_type == "l21" and np.ndim(c.max):
            pass                                       # (radii per frame: converted below)
        elif c.set_type in L2INF_KINDS:
            pass                                       # (max: one bound or one per group, converted by Projector)
        elif c.set_type in ("card_groups", "l20", "l20_joint"):
            pass                                       # (max is k, a count: Projector must see it unrounded to refuse one that TF cannot hold)
        elif np.ndim(c.min) == 0:
            if isinstance(c.min, (float, np.floating)):
                c.min, c.max = TF(c.min), TF(c.max)
        else:
            c.min, c.max = np.asarray(c.min, TF), np.asarray(c.max, TF)
        if c.set_type == "l21" and np.ndim(c.max) == 1:      # one radius per frame (TV_xy, ("slice", "z"))
            c.max = np.asarray(c.max, TF)
        if getattr(c, "weights", None) is not None and isinstance(c.weights, np.ndarray) and c.weights.dtype.kind == "f":
            c.weights = np.asarray(c.weights, TF)             # (like min / max: floating-point data takes the working precision)
        if c.set_type in ("l21", "l21_joint", "l21_groups", "tnv", "l1_weighted", "simplex", "card_groups", "l20", "l20_joint", "l21_stacked") + L2INF_KINDS:
            Projector(c, comp_grid, TF)      # a set of the engine's own: its refusals come before the operator is looked at
        if c.set_type in ("nuclear", "rank") and c.app_mode[0] in ("matrix", "tensor") and len(comp_grid.n) == 3:
            raise SipxError("requested rank or nuclear norm constraints on a tensor, use mode=(slice,x) e.t.c. to "
                            "define constraints per slice")
        if c.set_type in ("l1", "l2") and c.app_mode[0] in ("slice", "fiber") and not segment_norms:
            raise SipxError("l1 and l2 constraints only available for matrix or tensor mode, currently")
        if c.set_type in ("l1", "l2", "annulus") and c.app_mode[0] in ("slice", "fiber"):
            if not segment_norms:
                raise SipxError("annulus constraints per fiber or slice need setup_constraints(..., segment_norms=True)")
            cust0 = c.custom_TD_OP[0]
            if c.TD_OP in ("TV", "D2D", "D3D", "D_xz", "TV_xy") or not (isinstance(cust0, (tuple, list)) and len(cust0) == 0):
                raise SipxError("fiber / slice modes need an operator with one block (identity, D_x, D_y, D_z)")
        cust = c.custom_TD_OP[0] if c.set_type != "subspace" else ()
        named = "identity" if c.set_type in ("l21_stacked", "l2inf_stacked") and not (isinstance(cust, (tuple, list)) and len(cust) == 0) else c.TD_OP
        A, AtA_diag, dense, TD_n, banded = get_TD_operator(comp_grid, named, TF)      # (l21_stacked: the name of a caller-supplied operator is free)
        if not (isinstance(cust, (tuple, list)) and len(cust) == 0):          # setup_constraints.jl:70-72
            A = CustomOperator(cust, comp_grid, TF)
            AtA_diag, dense = False, False
        banded = True       # the engine keeps Q in CDS: a DFT set contributes the identity band like any orthogonal op
        P_sub.append(Projector(c, comp_grid, TF))
        if P_sub[-1].seg_radii:
            P_sub[-1].check_rows(A)           # nseg depends on the operator
        TD_OP.append(A)
        prop.AtA_diag.append(AtA_diag); prop.dense.append(dense); prop.TD_n.append(TD_n)
        prop.banded.append(banded); prop.AtA_offsets.append(None)
        prop.tag.append((c.set_type, c.TD_OP, c.app_mode[0], c.app_mode[1]))
        if c.set_type in ("rank", "cardinality", "card_groups", "l20", "l20_joint"):
            ncvx = True
        elif c.set_type in ("bounds", "histogram") and c.TD_OP != "identity" and TF(np.max(c.min)) > TF(0):
            ncvx = True
        else:
            ncvx = False
        prop.ncvx.append(ncvx)
    return P_sub, TD_OP, prop


def PARSDMM_precompute_distribute(TD_OP, set_Prop, comp_grid, options):
    """src/PARSDMM_precompute_distribute.jl:6-77.  AtA[i] = None means "generate the CDS bands of
    A_i'A_i on the device from the descriptor" (bit-identical to mat2CDS(TD_OP'*TD_OP)).
    A custom operator whose set is marked set_Prop.banded[i] = False, or whose A'A has more diagonals than one set hands over
    (MAX_SET_BANDS), gets AtA[i] = None and empty AtA_offsets[i] too: the engine applies it as a matrix-free term of Q,
    the reference's sparse Q of a set that is not banded (PARSDMM_precompute_distribute.jl:51-59, argmin_x.jl:42-51)."""
    TF = np.dtype(options.FL).type
    n, _ = _grid(comp_grid)
    if not options.feasibility_only:
        TD_OP.append(TDOperator("identity", comp_grid, TF))
        set_Prop.TD_n.append(n); set_Prop.AtA_offsets.append(np.array([0], np.int64))
        set_Prop.banded.append(True); set_Prop.AtA_diag.append(True)
        set_Prop.ncvx.append(False); set_Prop.dense.append(False)
        set_Prop.tag.append(("distance squared", "identity", "matrix", ""))
    p = len(TD_OP)
    AtA = [None] * p
    st = {1: 1, 2: n[0], 3: n[0] * n[1] if len(n) > 2 else None}
    for i in range(p):
        kind = TD_OP[i].kind
        if kind == "custom":
            # (more diagonals than one set hands over, as the named "Hessian" has with 13 / 25: the operator enters Q matrix-free)
            if not set_Prop.banded[i] or TD_OP[i].ata_diagonals() > min(MAX_SET_BANDS, MAX_Q_BANDS):
                AtA[i], set_Prop.AtA_offsets[i] = None, np.zeros(0, np.int64)
            else:
                AtA[i], set_Prop.AtA_offsets[i] = TD_OP[i].ata_cds()
            continue
        dirs = {"identity": [], "D_x": [0], "D_y": [1], "D_z": [len(n) - 1], "TV_xy": [0, 1]}.get(kind, list(range(len(n))))
        strides = [int(np.prod(n[:a])) for a in dirs]
        set_Prop.AtA_offsets[i] = np.array(sorted({0} | {s for s in strides} | {-s for s in strides}), np.int64)
    del st
    y = [np.zeros(TD_OP[i].shape[0], TF) for i in range(p)]
    l = [np.zeros(TD_OP[i].shape[0], TF) for i in range(p)]
    return TD_OP, AtA, l, y


def PARSDMM_precompute_distribute_Minkowski(TD_OP_c1, TD_OP_c2, TD_OP_sum, set_Prop_c1, set_Prop_c2, set_Prop_sum,
                                           comp_grid, options):
    """src/PARSDMM_precompute_distribute_Minkowski.jl:6-173 -> (TD_OP, set_Prop, AtA, l, y): the operators become the
    block rows [A 0], [0 A], [A A] acting on x = [u; v], the distance term [I I] is appended; AtA[i] = None (the 2N x 2N
    CDS bands are generated on the device)."""
    import copy
    TF = np.dtype(options.FL).type
    n, _ = _grid(comp_grid)
    groups = ((TD_OP_c1, 1), (TD_OP_c2, 2), (TD_OP_sum, 3))
    if any(A.kind == "TV_xy" for ops, _ in groups for A in ops):
        raise SipxError(TV_XY_NO_MINKOWSKI)
    TD_OP = [TDOperator(A.kind, comp_grid, TF, component=c) for ops, c in groups for A in ops]
    prop = copy.deepcopy(set_Prop_c1)
    for other in (set_Prop_c2, set_Prop_sum):
        for f in ("AtA_diag", "AtA_offsets", "TD_n", "banded", "dense", "ncvx", "tag"):
            getattr(prop, f).extend(copy.deepcopy(getattr(other, f)))
    if not options.feasibility_only:
        TD_OP.append(TDOperator("identity", comp_grid, TF, component=3))
        prop.TD_n.append(n); prop.AtA_offsets.append(np.array([0], np.int64))
        prop.banded.append(True); prop.AtA_diag.append(False); prop.dense.append(False)
        prop.ncvx.append(False); prop.tag.append(("distance squared", "identity", "matrix", ""))
    s = len(TD_OP)
    N = int(np.prod(n))
    for i in range(s):
        kind, comp = TD_OP[i].kind, TD_OP[i].component
        dirs = {"identity": [], "D_x": [0], "D_y": [1], "D_z": [len(n) - 1], "TV_xy": [0, 1]}.get(kind, list(range(len(n))))
        base = sorted({0} | {int(np.prod(n[:a])) for a in dirs} | {-int(np.prod(n[:a])) for a in dirs})
        off = sorted({o + sh for o in base for sh in (-N, 0, N)}) if comp == 3 else base
        prop.AtA_offsets[i] = np.array(off, np.int64)
    y = [np.zeros(TD_OP[i].shape[0], TF) for i in range(s)]
    l = [np.zeros(TD_OP[i].shape[0], TF) for i in range(s)]
    return TD_OP, prop, [None] * s, l, y


# --------------------------------------------------------------------------------------------------
# engine handle (phase-level API, include/sipx.h section A)
# --------------------------------------------------------------------------------------------------
def _warm_start_arrays(lst, TF, rows):
    """l or y of a warm start as contiguous vectors of the working precision, one per term."""
    if len(lst) != len(rows):
        raise SipxError("warm start: l and y need one vector per term (sets plus the distance term)")
    out = []
    for i, a in enumerate(lst):
        a = np.ascontiguousarray(a, TF)
        if a.shape != (rows[i],):
            raise SipxError(f"warm start: vector {i} has {a.shape} entries, operator {i} has {rows[i]} rows")
        out.append(a)
    return out


class Context:
    def __init__(self, comp_grid, TF, device: Optional[int] = None):
        device = _default_device if device is None else device
        self.TF = np.dtype(TF).type
        n, h = _grid(comp_grid)
        self.n, self.N = n, int(np.prod(n))
        self.Nx = self.N                         # unknowns: 2N once a Minkowski component is added
        self.h = C.c_void_p()
        na = (C.c_int64 * len(n))(*n)
        ha = (C.c_double * len(n))(*h)
        _chk(lib().sipx_create(C.byref(self.h), _dtype_code(self.TF), len(n), na, ha, device))
        self.rows: List[int] = []
        self.data_len: List[Optional[int]] = []      # per set: entries of the vectors set_data takes (None: it has none)
        self.p = self.pp = 0
        self._keep = []
        self._keep_proj: List[Projector] = []        # per set: its descriptor

    def close(self):
        if self.h:
            lib().sipx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_set(self, op: TDOperator, proj: Projector, ncvx=False, AtA=None, AtA_offsets=None) -> int:
        proj.check_rows(op)
        d = proj.desc(op.kind, ncvx)
        d.component = int(getattr(op, "component", 0))
        if d.component:
            self.Nx = 2 * self.N
        if op.kind == "custom":         # AtA = None: a matrix-free term of Q (sipx.h, SIPX_OP_CSC)
            cp = np.ascontiguousarray(op.A.indptr, np.int64); ri = np.ascontiguousarray(op.A.indices, np.int64)
            nz = np.ascontiguousarray(op.A.data, self.TF)
            self._keep += [cp, ri, nz]
            d.csc_colptr, d.csc_rowval, d.csc_nzval = cp.ctypes.data, ri.ctypes.data, nz.ctypes.data
            d.csc_rows = int(op.A.shape[0])
        self._keep.append(proj)
        if AtA is not None:
            R = np.asfortranarray(AtA, dtype=self.TF)
            off = np.ascontiguousarray(AtA_offsets, np.int64)
            rc = lib().sipx_add_set(self.h, C.byref(d), _ptr(R), _ptr(off), int(R.shape[1]))
        else:
            rc = lib().sipx_add_set(self.h, C.byref(d), None, None, 0)
        if rc < 0:
            raise SipxError(lib().sipx_last_error().decode())
        r = C.c_int64()
        _chk(lib().sipx_set_rows(self.h, rc, C.byref(r)))
        self.rows.append(int(r.value))
        self.data_len.append(proj.data_len(op))
        self._keep_proj.append(proj)
        return rc

    def set_q_mode(self, mode: str):
        if mode not in Q_MODES:
            raise SipxError(f"unknown Q mode {mode!r} (cds | stencil)")
        _chk(lib().sipx_set_q_mode(self.h, Q_MODES[mode]))

    def apply_Q(self, x):
        x = np.ascontiguousarray(x, self.TF)
        if x.shape != (self.Nx,):
            raise SipxError("length of x does not match the number of unknowns")
        y = np.empty_like(x)
        _chk(lib().sipx_apply_Q(self.h, _ptr(x), _ptr(y)))
        return y

    def q_terms(self):
        """(bands of the CDS part of Q, number of matrix-free terms) of the finalized context (sipx_q_terms)."""
        b, f = C.c_int(), C.c_int()
        _chk(lib().sipx_q_terms(self.h, C.byref(b), C.byref(f)))
        return int(b.value), int(f.value)

    def set_decomp(self, mode: str):
        """"sets": the reference's split by constraint set; "slab": every rank works on its z-slab of every set (sipx.h)."""
        if mode not in ("sets", "slab", "slab_full"):
            raise SipxError(f"unknown decomposition {mode!r} (sets | slab | slab_full)")
        # slab: a rank's arrays hold its planes only (sparse arrays); slab_full: whole arrays on every rank (levels of a multilevel solve)
        _chk(lib().sipx_set_decomp(self.h, {"sets": 0, "slab": 1, "slab_full": 2}[mode]))

    def set_owned(self, owned: Sequence[int]):
        a = np.zeros(len(self.rows) + 1, np.int32)       # constraint sets + the distance term
        a[:len(owned)] = np.asarray(owned, np.int32)[:len(a)]
        _chk(lib().sipx_set_owned(self.h, _ptr(a)))

    def finalize(self, m, rho_ini, gamma_ini, feasibility_only=False, zero_ini_guess=True, x0=None, l0=None, y0=None):
        return self._start(False, False, m, rho_ini, gamma_ini, feasibility_only, zero_ini_guess, x0, l0, y0)

    def reset(self, m, rho_ini, gamma_ini, zero_ini_guess=True, x0=None, l0=None, y0=None):
        """The same sets on the same grid, once more (sipx_reset): a new model m -- and, optionally, a new warm start and rho_ini --
        on this finalised context, without any allocation.  Returns the initial feasibilities.  A solve that follows gives the
        bits a newly built context gives."""
        return self._start(False, True, m, rho_ini, gamma_ini, False, zero_ini_guess, x0, l0, y0)

    def _start(self, on_dev, again, m, rho_ini, gamma_ini, feasibility_only, zero_ini_guess, x0, l0, y0):
        """What finalize, reset and their _dev forms are: m and the warm start checked against the grid and the rows of the terms,
        handed to sipx_finalize / sipx_reset (first call / again) or their _dev forms (on_dev: torch tensors on this context's GPU
        instead of numpy arrays).  Stores and returns the initial feasibilities."""
        TF = self.TF
        rows = self.rows if again else list(self.rows) + ([] if feasibility_only else [self.N])
        npp = self.pp if again else len(self.rows)
        l0, y0 = [None if lst is None or len(lst) == 0 else lst for lst in (l0, y0)]
        if on_dev:
            dev, ptr = m.device, _tensor_ptr
            _check_tensor("m", m, TF, self.N, dev)
            if x0 is not None:
                _check_tensor("x", x0, TF, self.Nx, dev)
            for name, lst in (("l", l0), ("y", y0)):
                if lst is not None:
                    _check_tensor_list(name, lst, TF, rows, dev)
            import torch
            self.set_caller_stream(torch.cuda.current_stream(dev).cuda_stream)
        else:
            ptr = _ptr
            m = np.ascontiguousarray(m, TF)
            if m.shape != (self.N,):
                raise SipxError("length of m does not match the grid")
            if x0 is not None:
                x0 = np.ascontiguousarray(x0, TF)
                if x0.shape != (self.Nx,):
                    raise SipxError("length of x does not match the grid")
            l0, y0 = [None if lst is None else _warm_start_arrays(lst, TF, rows) for lst in (l0, y0)]
        rho = np.ascontiguousarray(rho_ini, np.float64)
        feas = np.zeros(max(npp, 1))
        # (m, x0, l0, y0 -- the converted copies among them -- live until this frame is left: across the call)
        fn = getattr(lib(), ("sipx_reset" if again else "sipx_finalize") + ("_dev" if on_dev else ""))
        _chk(fn(self.h, ptr(m), _ptr(rho), len(rho), C.c_double(gamma_ini), *(() if again else (int(feasibility_only),)),
                int(zero_ini_guess), ptr(x0), _ptr_array(l0, ptr), _ptr_array(y0, ptr), _ptr(feas)))
        if not again:
            p, pp = C.c_int(), C.c_int()
            _chk(lib().sipx_num_terms(self.h, C.byref(p), C.byref(pp)))
            self.p, self.pp = p.value, pp.value
            if self.p > npp:
                self.rows.append(self.N)         # the distance term
        self.feasibility_initial = feas[:npp]
        return self.feasibility_initial

    # ---- device-resident forms (sipx_finalize_dev / sipx_reset_dev / sipx_download_dev): torch tensors on this context's GPU ----
    def set_caller_stream(self, stream):
        """The stream the caller's tensors are produced and consumed on (a hipStream_t as an integer, e.g.
        torch.cuda.current_stream().cuda_stream; 0 / None: the default stream).  The device-resident calls order themselves against it."""
        _chk(lib().sipx_set_caller_stream(self.h, C.c_void_p(int(stream or 0))))

    def _data_want(self, i):
        i = int(i)
        return self.data_len[i] if 0 <= i < len(self.data_len) else None

    def set_data(self, i, lb=None, ub=None):
        """New bound / histogram vectors for set i from numpy arrays (sipx_set_data): lengths and meaning as at add_set, None keeps a
        vector.  Before finalize they replace what add_set was given; on a finalized context they hold from the next reset on.
        A set without such vectors, the distance term and an index out of range are refused by the engine."""
        want, arrs = self._data_want(i), []
        for name, a in (("lb", lb), ("ub", ub)):
            if a is not None:
                a = _check_array(name, a, self.TF, want)
            arrs.append(a)
        P = self._keep_proj[int(i)] if 0 <= int(i) < len(self._keep_proj) else None
        if P is not None and P.kind == "l20" and P.seg_radii and arrs[1] is not None:
            for k in arrs[1].tolist():
                _check_l20_k(k, int(np.prod(_grid(P.comp_grid)[0][:2])), self.TF)
        elif P is not None and P.kind in L2INF_KINDS:
            if arrs[0] is not None:
                raise SipxError("set_data: " + L2INF_NO_WEIGHTS)
            if not P.seg_radii:
                raise SipxError("set_data: " + L2INF_NO_SET_DATA)
            if arrs[1] is not None:
                _check_l2inf_bounds(arrs[1], P.per, P.kind == "l2inf_stacked")
        elif P is not None and P.seg_radii and arrs[1] is not None:
            _check_l1_radii("l1" if P.kind == "l21" else P.kind, arrs[1])
        if P is not None and P.weighted:
            if arrs[1] is not None:
                raise SipxError(L1W_WEIGHTS_ARE_LB if P.kind == "l1_weighted" else L21_WEIGHTS_ARE_LB)
            if arrs[0] is not None:
                _check_l21_weights(P.kind, arrs[0])
        _chk(lib().sipx_set_data(self.h, int(i), _ptr(arrs[0]), _ptr(arrs[1])))

    def set_data_dev(self, i, lb=None, ub=None):
        """set_data with torch tensors on this context's GPU (sipx_set_data_dev), ordered against torch's current stream: what that
        stream has queued before the call is seen, the tensors may be overwritten by work queued on it afterwards; no host wait."""
        import torch
        want, dev = self._data_want(i), None
        for name, t in (("lb", lb), ("ub", ub)):
            if t is not None:
                _check_tensor(name, t, self.TF, t.shape[0] if want is None and t.dim() == 1 else want, dev)
                dev = t.device
        if dev is not None:
            self.set_caller_stream(torch.cuda.current_stream(dev).cuda_stream)
        _chk(lib().sipx_set_data_dev(self.h, int(i), _tensor_ptr(lb), _tensor_ptr(ub)))

    def io_bytes(self, reset=False):
        """(host-to-device, device-to-host) bytes of the N-sized transfers finalize, reset and download have made (sipx_io_bytes)."""
        a, b = C.c_int64(), C.c_int64()
        _chk(lib().sipx_io_bytes(self.h, C.byref(a), C.byref(b), int(bool(reset))))
        return a.value, b.value

    def finalize_dev(self, m, rho_ini, gamma_ini, feasibility_only=False, zero_ini_guess=True, x0=None, l0=None, y0=None):
        """finalize with m and the warm start as torch tensors on this context's GPU, ordered against torch's current stream."""
        return self._start(True, False, m, rho_ini, gamma_ini, feasibility_only, zero_ini_guess, x0, l0, y0)

    def reset_dev(self, m, rho_ini, gamma_ini, zero_ini_guess=True, x0=None, l0=None, y0=None):
        """reset with m and the warm start as torch tensors on this context's GPU, ordered against torch's current stream."""
        return self._start(True, True, m, rho_ini, gamma_ini, False, zero_ini_guess, x0, l0, y0)

    def download_dev(self, device, want_ly=True, out=None):
        """x, l, y as torch tensors on `device` (this context's GPU), written on the engine stream; torch's current stream waits
        for them by an event, the host does not.  out = (x, l, y): preallocated tensors that are filled and returned."""
        import torch
        dt = torch.float32 if self.TF == np.float32 else torch.float64
        ox, ol, oy = (None, None, None) if out is None else out
        if ox is None:
            ox = torch.empty(self.Nx, dtype=dt, device=device)
        else:
            _check_tensor("out x", ox, self.TF, self.Nx, device)
        res = [ox]
        for name, lst in (("out l", ol), ("out y", oy)):
            if not want_ly:
                res.append(None)
            elif lst is None:
                res.append([torch.empty(r, dtype=dt, device=device) for r in self.rows])
            else:
                _check_tensor_list(name, lst, self.TF, self.rows, device)
                res.append(lst)
        x, l, y = res
        self.set_caller_stream(torch.cuda.current_stream(device).cuda_stream)
        _chk(lib().sipx_download_dev(self.h, _tensor_ptr(x), _ptr_array(l, _tensor_ptr), _ptr_array(y, _tensor_ptr)))
        return x, l, y

    # ---- phases ----
    def rhs_compose(self, rho):
        rho = np.ascontiguousarray(rho, np.float64)
        _chk(lib().sipx_rhs_compose(self.h, _ptr(rho)))

    def argmin_x(self, it, tol_ref):
        t, ci, rr, fl = C.c_double(tol_ref), C.c_int64(), C.c_double(), C.c_int()
        _chk(lib().sipx_argmin_x(self.h, int(it), C.byref(t), C.byref(ci), C.byref(rr), C.byref(fl)))
        return t.value, ci.value, rr.value, fl.value

    def update_y_l(self, it, flags, rho, gamma):
        rho = np.ascontiguousarray(rho, np.float64); gamma = np.ascontiguousarray(gamma, np.float64)
        rp, rd, fe = np.zeros(self.p), np.zeros(self.p), np.zeros(max(self.pp, 1))
        _chk(lib().sipx_update_y_l(self.h, int(it), int(flags), _ptr(rho), _ptr(gamma), _ptr(rp), _ptr(rd), _ptr(fe)))
        return rp, rd, fe[:self.pp]

    def log_scalars(self):
        a, b = C.c_double(), C.c_double()
        _chk(lib().sipx_log_scalars(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def adapt_rho_gamma(self, adjust_rho, adjust_gamma, rho, gamma):
        rho = np.array(rho, np.float64); gamma = np.array(gamma, np.float64)
        _chk(lib().sipx_adapt_rho_gamma(self.h, int(adjust_rho), int(adjust_gamma), _ptr(rho), _ptr(gamma)))
        return rho, gamma

    def q_update(self, rho_new, rho_old):
        a = np.ascontiguousarray(rho_new, np.float64); b = np.ascontiguousarray(rho_old, np.float64)
        _chk(lib().sipx_q_update(self.h, _ptr(a), _ptr(b)))

    def download(self, want_ly=True, x_out=None):
        # the reference overwrites the x argument in place (cg.jl:95, PARSDMM.jl:64): a caller's array of the right kind is the
        # destination itself -- its pages exist already, a fresh array pays a page fault per 4 KiB of the copy
        if (x_out is not None and isinstance(x_out, np.ndarray) and x_out.dtype == self.TF and x_out.shape == (self.Nx,)
                and x_out.flags.c_contiguous and x_out.flags.writeable):
            x = x_out
        else:
            x = np.empty(self.Nx, self.TF)
        l = [np.zeros(r, self.TF) for r in self.rows] if want_ly else None
        y = [np.zeros(r, self.TF) for r in self.rows] if want_ly else None
        _chk(lib().sipx_download(self.h, _ptr(x), _ptr_array(l), _ptr_array(y)))
        return x, l, y

    def warm_start_from(self, coarse: "Context"):
        """x, l, y of this (finer) level from a solved coarser context, resampled on the device (sipx_warm_start_from)."""
        _chk(lib().sipx_warm_start_from(self.h, coarse.h))

    def slab(self):
        """(row0, row1, chunk): this rank's rows of the x-step and the elements per rank of the padded exchange buffers."""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        _chk(lib().sipx_slab(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def get_rhs(self):
        """rhs of the last rhs_compose (src/rhs_compose.jl:24-36), copied to the host."""
        rhs = np.empty(self.Nx, self.TF)
        _chk(lib().sipx_get_rhs(self.h, _ptr(rhs)))
        return rhs

    def get_Q(self):
        d = C.c_int()
        offs = np.zeros(32, np.int64)
        _chk(lib().sipx_get_Q(self.h, None, _ptr(offs), C.byref(d)))
        Q = np.empty((self.Nx, d.value), self.TF, order="F")
        _chk(lib().sipx_get_Q(self.h, _ptr(Q), _ptr(offs), C.byref(d)))
        return Q, offs[:d.value].copy()

    def time_spmv(self, reps=20):
        ms = C.c_double()
        _chk(lib().sipx_time_spmv(self.h, int(reps), C.byref(ms)))
        return ms.value

    def debug_proj(self, set_index: int, which: int = 0):
        out = np.zeros(16)
        _chk(lib().sipx_debug_proj(self.h, int(set_index), int(which), _ptr(out)))
        keys = ("need", "theta", "theta_prev", "hw", "spec_lo", "spec_hi", "lo", "hi", "asum", "vmax", "gathered",
                "overflow", "spec_ok", "michelot_its", "refine", "lean")
        d = dict(zip(keys, out))
        d["sampled"] = float(int(d["lean"]) >> 1)      # the probes of the last search were centred by the sampled estimate
        d["lean"] = float(int(d["lean"]) & 1)
        return d

    def kernel_stats(self, enable):
        """(launches, total ms) of the CG product since the last call; then (re)starts the collection: 0 / False = off,
        1 / True = that kernel only, 2 = every kernel (sipx.h, sipx_kernel_stats)."""
        n, ms = C.c_int64(), C.c_double()
        _chk(lib().sipx_kernel_stats(self.h, int(enable), C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def kernel_stats_all(self, enable):
        """Per-kernel statistics gathered since the last call, as a dict (sipx_kernel_stats_json); `enable` as above.
        enable = -1: the engine's counters only (`slab_searches`, `rank_route`, `routes`) -- nothing is synchronised, a
        running collection and its samples stay as they are.  `routes` counts, since finalize, the launches of the Q
        products and of the right-hand side per kernel that served them -- `k_cds_march<MODE=m>/bands` and `/table` (m = 3:
        the fused iteration), `k_cds<MODE=m>`, `k_cds_fused`, `k_rhs_march`, `k_rhs` -- where the entries of `kernels`
        name the marched and the flat kernel alike."""
        import json
        txt = lib().sipx_kernel_stats_json(self.h, int(enable))
        if txt is None:
            raise SipxError(lib().sipx_last_error().decode())
        return json.loads(txt.decode())

    def device_bytes(self):
        """{"context": bytes this context allocated on its GPU, "device_used", "device_total": the runtime's figures} (sipx_device_bytes)."""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        _chk(lib().sipx_device_bytes(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return {"context": a.value, "device_used": b.value, "device_total": c.value}

    def comm_info(self):
        """What the attached communicator reports: {"nranks", "rank", "version", "decomposition"} (sipx_comm_info)."""
        n, r, d = C.c_int(), C.c_int(), C.c_int()
        ver = C.create_string_buffer(64)
        _chk(lib().sipx_comm_info(self.h, C.byref(n), C.byref(r), ver, 64, C.byref(d)))
        return {"nranks": n.value, "rank": r.value, "version": ver.value.decode(), "decomposition": "slab" if d.value == 1 else "sets"}

    def _log_struct(self, options: PARSDMM_options):
        maxit, p, pp = int(options.maxit), self.p, self.pp
        o = _Options(maxit, float(options.evol_rel_tol), float(options.feas_tol), float(options.obj_tol),
                     int(options.rho_update_frequency), int(options.adjust_rho), int(options.adjust_gamma),
                     int(options.adjust_feasibility_rho))
        arrs = dict(set_feasibility=np.zeros((maxit, max(pp, 1))), r_dual=np.zeros((maxit, p)),
                    r_pri=np.zeros((maxit, p)), r_dual_total=np.zeros(maxit), r_pri_total=np.zeros(maxit),
                    obj=np.zeros(maxit), evol_x=np.zeros(maxit), rho=np.zeros((maxit, p)),
                    gamma=np.zeros((maxit, p)), cg_it=np.zeros(maxit, np.int64), cg_relres=np.zeros(maxit))
        lg = _Log()
        for k, a in arrs.items():
            setattr(lg, k, a.ctypes.data)
        return o, lg, arrs

    def _log_result(self, lg, arrs):
        it, nf, pp = lg.n_iter, lg.n_feas_rows, self.pp
        return log_type_PARSDMM(arrs["set_feasibility"][:nf, :pp], arrs["r_dual"][:it], arrs["r_pri"][:it],
                                arrs["r_dual_total"][:it], arrs["r_pri_total"][:it], arrs["obj"][:it],
                                arrs["evol_x"][:it], arrs["rho"][:it], arrs["gamma"][:it], arrs["cg_it"][:it],
                                arrs["cg_relres"][:it],
                                dict(zip(TIMING_SECTIONS, [t * 1e-3 for t in lg.timing_ms])))

    def parsdmm(self, options: PARSDMM_options):
        o, lg, arrs = self._log_struct(options)
        _chk(lib().sipx_parsdmm(self.h, C.byref(o), C.byref(lg)))
        return self._log_result(lg, arrs), bool(lg.stopped_feasible)

    # the same native solve advanced in pieces (sipx_parsdmm_begin / sipx_parsdmm_steps)
    def parsdmm_begin(self, options: PARSDMM_options):
        self._run = self._log_struct(options)            # keeps the log arrays alive
        o, lg, arrs = self._run
        _chk(lib().sipx_parsdmm_begin(self.h, C.byref(o), C.byref(lg)))

    def parsdmm_steps(self, nsteps: int) -> bool:
        done = C.c_int()
        _chk(lib().sipx_parsdmm_steps(self.h, int(nsteps), C.byref(done)))
        return bool(done.value)

    def parsdmm_log(self):
        o, lg, arrs = self._run
        return self._log_result(lg, arrs)


def _check_term_count(TD_OP, P_sub, options):
    if len(TD_OP) != len(P_sub) + (0 if options.feasibility_only else 1):
        raise SipxError("TD_OP must hold one operator per set plus the identity of the distance term "
                        "(output of PARSDMM_precompute_distribute)")


def _populate(ctx, AtA, TD_OP, set_Prop, P_sub, options) -> Context:
    """The sets and the Q mode of a new context, which is closed when one of them is refused.  What is left is finalize."""
    try:
        for i, P in enumerate(P_sub):
            A = AtA[i] if AtA is not None else None
            ctx.add_set(TD_OP[i], P, set_Prop.ncvx[i], A, set_Prop.AtA_offsets[i] if A is not None else None)
        ctx.set_q_mode(getattr(options, "Q_mode", "cds"))
    except Exception:
        ctx.close()
        raise
    return ctx


def _start_values(options, TF, x=None, l=None, y=None):
    """(rho_ini, gamma_ini, zero_ini_guess, warm start) as finalize and reset take them: the options in the working precision
    (convert_options!.jl:6-15); with zero_ini_guess x, l, y are zero-filled (PARSDMM_initialize.jl:304-313) and not passed on."""
    zero = bool(options.zero_ini_guess)
    return [float(TF(r)) for r in options.rho_ini], float(TF(options.gamma_ini)), zero, (None, None, None) if zero else (x, l, y)


def build_context(m, AtA, TD_OP, set_Prop, P_sub, comp_grid, options, x=None, l=None, y=None, device=None,
                  owned=None, attach=None) -> Context:
    """Everything PARSDMM_initialize allocates (src/PARSDMM_initialize.jl:117-230), on the device.  `attach(ctx)` is called
    before sipx_finalize: where a rank of a sharded solve is given its communicator (sharded.attach_comm)."""
    TF = np.dtype(m.dtype).type
    if not (np.isrealobj(m) and (x is None or np.isrealobj(x))):
        raise SipxError("input for PARSDMM is not real")                 # src/PARSDMM.jl:50-52
    _check_term_count(TD_OP, P_sub, options)
    ctx = _populate(Context(comp_grid, TF, device), AtA, TD_OP, set_Prop, P_sub, options)
    try:
        if owned is not None:
            ctx.set_owned(owned)
        if attach is not None:
            attach(ctx)
        rho_ini, gamma_ini, zero, warm = _start_values(options, TF, x, l, y)
        ctx.finalize(m, rho_ini, gamma_ini, options.feasibility_only, zero, *warm)
    except Exception:
        ctx.close()
        raise
    return ctx


def _solve(ctx, again, t0, m, options, x, l, y, outputs, out=None, dev=None):
    """The whole solve on a populated context, for every front end: start (finalize, or reset when the context has been through
    one: `again`), the native loop, the download -> (x, log, l, y).  dev = None: the host form (numpy arrays); a torch.device:
    the device-resident form, tensors on that GPU and `out` the preallocated results.  t0: the clock at entry of the caller."""
    import time
    rho_ini, gamma_ini, zero, warm = _start_values(options, ctx.TF, x, l, y)
    ctx._start(dev is not None, again, m, rho_ini, gamma_ini, options.feasibility_only, zero, *warm)
    t_init = time.perf_counter() - t0
    log, _ = ctx.parsdmm(options)
    log.timing[TIMING_SECTIONS[0]] = t_init          # "initialization": PARSDMM_initialize (src/PARSDMM.jl:40)
    want_ly = outputs == "all"
    # the reference overwrites the x argument in place (PARSDMM.jl:64)
    if dev is not None:
        xo, lo, yo = ctx.download_dev(dev, want_ly, (x, None, None) if out is None and x is not None else out)
    else:
        xo, lo, yo = ctx.download(want_ly, x_out=x)
        if isinstance(x, np.ndarray) and xo is not x and len(x) == len(xo):
            x[:] = xo
            xo = x
    log.context_reused = again
    return xo, log, lo, yo


# Contexts kept between calls of PARSDMM (round 5).  The reference's callers wrap PARSDMM as a projector and call it again and again
# with the same sets on the same grid (examples/constrained_freq_FWI_simple.jl:468, examples/Constraint_examples_2D.jl:222-223,
# examples/Dykstra_parallel_vs_PARSDMM.jl:134); every such call of the reference allocates its 16 work vectors per set again
# (src/PARSDMM_initialize.jl:129-184).  Here a call looks its context up by (device, precision, grid, Q mode, set descriptors): a
# hit costs sipx_reset -- zero-fills, the upload of m, Q assembled again, the initial feasibility -- instead of sipx_create ...
# sipx_finalize.  Only descriptors without array arguments are cached (scalar bounds, radii, ranks ...: what their bytes are is what
# they are); a list with bound vectors, a subspace basis, a caller-supplied operator or explicit A'A bands builds a context per call
# as before.  SIPX_CONTEXT_CACHE=0 switches the cache off, SIPX_CONTEXT_CACHE=k keeps k contexts (default 2: each holds the whole
# device state of its problem); clear_context_cache() frees them.
_ctx_cache: "dict" = {}


_extra_caches: "list" = []           # (multilevel.py keeps the level contexts of its last call: cleared together with these)


def clear_context_cache():
    for ctx in list(_ctx_cache.values()):
        ctx.close()
    _ctx_cache.clear()
    for f in _extra_caches:
        f()


def _cache_limit() -> int:
    e = os.environ.get("SIPX_CONTEXT_CACHE")
    if e is None or e == "":
        return 2
    try:
        return max(0, int(e))
    except ValueError:
        return 2


def _context_key(m, AtA, TD_OP, set_Prop, P_sub, comp_grid, options, device):
    """None when this problem must not be cached (array arguments inside a descriptor, explicit A'A bands, sharded set ownership)."""
    n, h = _grid(comp_grid)
    sig = []
    for i, P in enumerate(P_sub):
        if not isinstance(P, Projector) or P.lb is not None or P.ub is not None or P.basis is not None:
            return None
        op = TD_OP[i]
        if not isinstance(op, TDOperator) or op.kind == "custom" or (AtA is not None and AtA[i] is not None):
            return None
        sig.append((op.kind, int(getattr(op, "component", 0)), P.kind, P.pmin, P.pmax, P.mode, P.dir, P.transform, bool(set_Prop.ncvx[i])))
    dev = _default_device if device is None else device
    # (the engine reads its A/B switches when a context is built: a context built under other switches is another context)
    env = tuple(sorted((k, v) for k, v in os.environ.items() if k.startswith("SIPX_")))
    return (dev, np.dtype(m.dtype).str, tuple(n), tuple(h), bool(options.feasibility_only), getattr(options, "Q_mode", "cds"), tuple(sig), env)


class _CachedContext:
    """The context of one call of a cached front end, `with _CachedContext(m, <the problem>, device) as slot`: slot.ctx is the
    entry of _ctx_cache for this problem, taken out for the call (slot.reused), or a context built and populated now (m gives
    the precision only).  When the body raises, the context is closed and forgotten.  Otherwise it goes (back) into the cache,
    whose oldest entries make room for it; a problem that is not cached (no key) has its context closed."""

    def __init__(self, m, AtA, TD_OP, set_Prop, P_sub, comp_grid, options, device):
        self.limit = _cache_limit()
        self.key = _context_key(m, AtA, TD_OP, set_Prop, P_sub, comp_grid, options, device) if self.limit > 0 else None
        self.ctx = _ctx_cache.pop(self.key, None) if self.key is not None else None
        self.reused = self.ctx is not None
        if not self.reused:
            _check_term_count(TD_OP, P_sub, options)
            self.ctx = _populate(Context(comp_grid, np.dtype(m.dtype).type, device), AtA, TD_OP, set_Prop, P_sub, options)

    def __enter__(self):
        return self

    def __exit__(self, etype, exc, tb):
        if etype is not None:
            if issubclass(etype, Exception):
                self.ctx.close()
        elif self.key is not None:
            while len(_ctx_cache) >= self.limit:                 # the oldest entry goes (dicts keep insertion order)
                _ctx_cache.pop(next(iter(_ctx_cache))).close()
            _ctx_cache[self.key] = self.ctx
        else:
            self.ctx.close()
        return False


def PARSDMM(m, AtA, TD_OP, set_Prop, P_sub, comp_grid, options, x=None, l=None, y=None, device=None, outputs="all"):
    """Drop-in for src/PARSDMM.jl:25-258 (serial path): returns (x, log_PARSDMM, l, y).
    outputs="x": l and y are not copied back (returned as None) -- a caller that uses PARSDMM as a projector reads x only
    (examples/constrained_freq_FWI_simple.jl:468 keeps `[1]` of the result)."""
    import time
    t0 = time.perf_counter()
    if outputs not in ("all", "x"):
        raise SipxError("outputs must be 'all' or 'x'")
    if not (np.isrealobj(m) and (x is None or np.isrealobj(x))):
        raise SipxError("input for PARSDMM is not real")                 # src/PARSDMM.jl:50-52
    with _CachedContext(m, AtA, TD_OP, set_Prop, P_sub, comp_grid, options, device) as slot:
        return _solve(slot.ctx, slot.reused, t0, m, options, x, l, y, outputs)


# --------------------------------------------------------------------------------------------------
# the device-resident form of the whole solve
# --------------------------------------------------------------------------------------------------
def _tensor_TF(name, t):
    """Working precision of a torch tensor (checked without importing torch: by the names of its type and dtype)."""
    if type(t).__module__.split(".")[0] != "torch" or not hasattr(t, "data_ptr"):
        raise SipxError(f"{name} must be a torch tensor on a GPU (PARSDMM takes numpy arrays)")
    TF = {"torch.float32": np.float32, "torch.float64": np.float64}.get(str(t.dtype))
    if TF is None:
        raise SipxError(f"{name} must be Float32 or Float64, not {t.dtype}")
    return TF


def _check_tensor(name, t, TF, length, device):
    if _tensor_TF(name, t) != np.dtype(TF).type:
        raise SipxError(f"{name} has dtype {t.dtype}: not the working precision ({np.dtype(TF).name})")
    if not t.is_cuda:
        raise SipxError(f"{name} must live on a GPU, not on {t.device}")
    if device is not None and t.device != device:
        raise SipxError(f"{name} lives on {t.device}, m on {device}")
    if t.dim() != 1:
        raise SipxError(f"{name} must be 1-D, not of shape {tuple(t.shape)}")
    if not t.is_contiguous():
        raise SipxError(f"{name} must be contiguous (strided tensors are not taken)")
    if t.shape[0] != length:
        raise SipxError(f"{name} has {t.shape[0]} entries, {length} are needed")


def _check_tensor_list(name, lst, TF, rows, device):
    if not isinstance(lst, (list, tuple)) or len(lst) != len(rows):
        raise SipxError(f"{name} needs one vector per term (sets plus the distance term): {len(rows)}, not "
                        f"{len(lst) if isinstance(lst, (list, tuple)) else type(lst).__name__}")
    for i, t in enumerate(lst):
        _check_tensor(f"{name}[{i}]", t, TF, rows[i], device)


def _check_device_args(m, x, l, y, out, TF, N, Nx, rows, outputs):
    """The tensor arguments of a device-form solve: everything that can be wrong with them, before the library is touched or a
    pointer is taken.  m names the device, the others live there."""
    _check_tensor("m", m, TF, N, None)
    dev = m.device
    if x is not None:
        _check_tensor("x", x, TF, Nx, dev)
    for name, lst in (("l", l), ("y", y)):
        if lst is not None:
            _check_tensor_list(name, lst, TF, rows, dev)
    if out is not None:
        if not isinstance(out, (list, tuple)) or len(out) != 3:
            raise SipxError("out must be (x, l, y): the result tensors (l, y may be None with outputs='x')")
        if out[0] is not None:
            _check_tensor("out x", out[0], TF, Nx, dev)
        for name, lst in (("out l", out[1]), ("out y", out[2])):
            if lst is not None and outputs == "all":
                _check_tensor_list(name, lst, TF, rows, dev)


def _check_array(name, a, TF, length):
    """A numpy vector of the working precision; returned contiguous."""
    if not isinstance(a, np.ndarray):
        raise SipxError(f"{name} must be a numpy array (the device form takes torch tensors), not {type(a).__name__}")
    if a.dtype.type != np.dtype(TF).type:
        raise SipxError(f"{name} has dtype {a.dtype}: not the working precision ({np.dtype(TF).name})")
    if a.ndim != 1:
        raise SipxError(f"{name} must be 1-D, not of shape {a.shape}")
    if length is not None and a.shape[0] != length:
        raise SipxError(f"{name} has {a.shape[0]} entries, {length} are needed")
    return np.ascontiguousarray(a)


L21_WEIGHTS_ARE_LB = "set_data: the weights of an l2,1 set are its lb; it has no ub (the radius is fixed when the set is built)"


def _check_l21_weights(kind, w):
    """No host path hands the device a weight of the weighted l2,1 ball that is negative, NaN or infinite (csrc/l21_weighted.h); nor one
    of the weighted l1 ball (kind "l1_weighted", csrc/l1_weighted.h), in words of its own."""
    w = np.asarray(w)
    ok = np.isfinite(w) & (w >= 0)
    if not np.all(ok):
        bad = int(np.flatnonzero(~ok)[0])
        if kind in ("l1_weighted", "l1_weighted_norm"):
            raise SipxError(f"the weighted l1 ball (l1_weighted): weight {bad} is negative, NaN or infinite ({w[bad]!r}) -- every weight must "
                            "be finite and >= 0 (0 leaves its row free)")
        raise SipxError(f"the weighted l2,1 ball ({kind}): weight {bad} is negative, NaN or infinite ({w[bad]!r}) -- every weight must be "
                        "finite and >= 0 (0 leaves its group unconstrained)")


def _check_l20_k(k, ngroups, TF):
    """One budget of an l2,0 set over ngroups groups in precision TF (csrc/l20.h, l20_check_k): an integer >= 1 that TF holds."""
    if isinstance(k, (bool, np.bool_)) or np.ndim(k) != 0:
        raise SipxError(L20_BAD_K)
    k = float(k)
    if not np.isfinite(k) or k != np.floor(k) or k < 1:
        raise SipxError(L20_BAD_K)
    if k < ngroups and float(TF(k)) != k:
        raise SipxError(L20_K_INEXACT)
    return k


def _check_l1_radii(kind, r):
    """project_l1_Duchi!.jl:22 for every segment: no host path hands the device an l1 radius that is not > 0."""
    if kind == "l1" and not np.all(np.asarray(r) > 0):
        bad = int(np.flatnonzero(~(np.asarray(r) > 0))[0])
        raise SipxError(f"Radius of L1 ball is negative (segment {bad}: {np.asarray(r)[bad]!r})")


_one_runtime_checked = False


def _check_one_hip_runtime():
    """torch wheels bring a HIP runtime of their own.  Imported BEFORE libsipx.so is loaded, torch's copy serves both (the
    loader matches the library name); the other way round the process holds two runtimes, and a stream or a buffer of one means
    nothing to the other.  Looked at once per process."""
    global _one_runtime_checked
    if _one_runtime_checked:
        return
    lib()
    try:
        with open("/proc/self/maps") as f:
            paths = {ln.split()[-1] for ln in f if "libamdhip64" in ln}
    except OSError:
        paths = set()
    if len(paths) > 1:
        raise SipxError("two HIP runtimes are loaded in this process (" + ", ".join(sorted(paths)) + "): torch tensors cannot be "
                        "shared with the engine.  Import torch before the first call into sipx")
    _one_runtime_checked = True


def PARSDMM_device(m, AtA, TD_OP, set_Prop, P_sub, comp_grid, options, x=None, l=None, y=None, outputs="all", out=None):
    """PARSDMM for data that lives on the GPU: m, x, l[i], y[i] are 1-D contiguous torch tensors of the working precision on one
    ROCm device (taken from m), in the reference's row order; returns (x, log_PARSDMM, l, y) with tensors on that device
    (l, y = None with outputs="x").  No vector crosses PCIe and the host waits for nothing but the solve: the call orders itself
    against torch.cuda.current_stream(m.device) -- whatever that stream has queued before the call is seen, and work queued on
    it afterwards sees the results.  out = (x, l, y) supplies preallocated result tensors (l, y may be None with outputs="x"),
    which are filled and returned, so that a loop allocates nothing.  Contexts are cached as for PARSDMM (the same keys: a
    host-form and a device-form call of one problem share a context); the solve and its log are those of PARSDMM, bit for bit."""
    import time
    t0 = time.perf_counter()
    if outputs not in ("all", "x"):
        raise SipxError("outputs must be 'all' or 'x'")
    # ---- everything that can be wrong with the arguments, before the library is touched
    TF = _tensor_TF("m", m)
    n, _ = _grid(comp_grid)
    N = int(np.prod(n))
    _check_term_count(TD_OP, P_sub, options)
    Nx = 2 * N if any(int(getattr(A, "component", 0)) for A in TD_OP) else N
    _check_device_args(m, x, l, y, out, TF, N, Nx, [int(A.shape[0]) for A in TD_OP], outputs)
    import torch
    _check_one_hip_runtime()
    device = m.device.index if m.device.index is not None else torch.cuda.current_device()
    # (the key of the host form: m stands in by its precision)
    with _CachedContext(np.empty(0, TF), AtA, TD_OP, set_Prop, P_sub, comp_grid, options, device) as slot:
        return _solve(slot.ctx, slot.reused, t0, m, options, x, l, y, outputs, out, torch.device("cuda", device))


# --------------------------------------------------------------------------------------------------
# one context, many projections, the data of a set replaced in between
# --------------------------------------------------------------------------------------------------
def _is_tensor(a):
    return type(a).__module__.split(".")[0] == "torch"


class Solver:
    """A list of sets kept alive on the GPU: build once, then project model after model through it and replace the vectors of a
    data-bearing set in between -- the loop of the reference's application examples, which learn their constraints once and give
    every image its own data-fit box, P_sub[end] = x -> project_bounds!(x, LBD, UBD)
    (examples/Indonesia_desaturation/image_desaturation_by_constraint_learning.jl:264).

        S = Solver(AtA, TD_OP, set_Prop, P_sub, comp_grid, options, TF, device=None)
        S.set_data(i, lb=None, ub=None)      # numpy arrays or CUDA tensors; holds until changed; None keeps a vector
        x, log, l, y = S(m, x=None, l=None, y=None, outputs="all", out=None)
        S.close()                            # also a context manager

    The arguments are those of PARSDMM.  The first call builds the context (sipx_finalize), every later one is sipx_reset, the
    solve and the download; data set before the first call goes in before finalize.  With a torch tensor m the call is the
    device-resident one (PARSDMM_device): every argument is a tensor on m's device, the results are tensors there, torch's
    current stream is the caller's stream.  set_data takes element-wise or per-fiber bounds (no transform), the relaxed
    histogram and the radii of a per-fiber / per-slice l1, l2 or annulus set that was built with a vector of them (ub: the radii,
    lb: the annulus' inner radii; nseg entries); a numpy vector is uploaded at every set_data (the array may be changed afterwards), a tensor is read on the device.
    Every wrong argument raises SipxError before the library is touched.  log.context_reused tells whether the call found its
    context built.  The Solver owns its context: the caches of PARSDMM / PARSDMM_device and clear_context_cache() do not know it."""

    def __init__(self, AtA, TD_OP, set_Prop, P_sub, comp_grid, options, TF, device=None):
        self.TF = np.dtype(TF).type
        _dtype_code(self.TF)
        _check_term_count(TD_OP, P_sub, options)
        for i, P in enumerate(P_sub):
            if not isinstance(P, Projector):
                raise SipxError(f"P_sub[{i}] must be a Projector (the output of setup_constraints)")
            if P.TF != self.TF:
                raise SipxError(f"P_sub[{i}] was set up in {np.dtype(P.TF).name}, the Solver in {np.dtype(self.TF).name}")
        if any(int(getattr(A, "component", 0)) for A in TD_OP):
            raise SipxError("Solver: Minkowski sets are not taken (use PARSDMM)")
        self.AtA, self.TD_OP, self.set_Prop, self.P_sub = AtA, list(TD_OP), set_Prop, list(P_sub)
        self.comp_grid, self.options = comp_grid, options
        self.feasibility_only = bool(options.feasibility_only)
        n, _ = _grid(comp_grid)
        self.N = int(np.prod(n))
        self.rows = [int(A.shape[0]) for A in TD_OP]
        self.device = None if device is None else int(device)
        self.ctx: Optional[Context] = None
        self.built = self.closed = False

    # ---- argument checks (nothing here touches the library)
    def _device_of(self, t):
        """Index of the GPU a tensor lives on; refused when the Solver is bound to another one."""
        idx = t.device.index
        if idx is None:
            import torch
            idx = torch.cuda.current_device()
        if self.device is not None and idx != self.device:
            raise SipxError(f"the tensors live on cuda:{idx}, the Solver on cuda:{self.device}")
        return idx

    def _check_open(self):
        if self.closed:
            raise SipxError("this Solver has been closed")

    def _context(self, device):
        if self.ctx is None:
            self.device = _default_device if device is None else device
            self.ctx = _populate(Context(self.comp_grid, self.TF, self.device), self.AtA, self.TD_OP, self.set_Prop, self.P_sub,
                                 self.options)
        return self.ctx

    def set_data(self, i, lb=None, ub=None):
        self._check_open()
        if not isinstance(i, (int, np.integer)) or isinstance(i, bool):
            raise SipxError(f"set_data: the set index must be an integer, not {type(i).__name__}")
        i = int(i)
        pp = len(self.P_sub)
        if i == pp and not self.feasibility_only:
            raise SipxError(f"set_data: index {i} is the distance term, which holds no vectors (its data is m)")
        if not 0 <= i < pp:
            raise SipxError(f"set_data: set index {i} out of range ({pp} sets)")
        if self.P_sub[i].kind == "card_groups":
            raise SipxError("set_data: " + CARDG_NO_SET_DATA)
        if self.P_sub[i].kind in ("l20", "l20_joint") and not self.P_sub[i].seg_radii:
            raise SipxError("set_data: " + L20_NO_SET_DATA)
        if self.P_sub[i].kind == "l20" and lb is not None:
            raise SipxError("set_data: " + L20_SET_DATA_UB)
        if self.P_sub[i].kind in L2INF_KINDS and lb is not None:
            raise SipxError("set_data: " + L2INF_NO_WEIGHTS)
        if self.P_sub[i].kind in L2INF_KINDS and not self.P_sub[i].seg_radii:
            raise SipxError("set_data: " + L2INF_NO_SET_DATA)
        want = self.P_sub[i].data_len(self.TD_OP[i])
        if want is None:
            raise SipxError(f"set_data: set {i} ({self.set_Prop.tag[i][0]} on {self.set_Prop.tag[i][1]}) holds no replaceable vectors -- "
                            "element-wise and per-fiber bounds (no transform), the relaxed histogram and per-fiber / per-slice l1, l2 "
                            "and annulus sets built with a vector of radii do, and the l2,1 sets built with weights; build a new "
                            "Solver for other data")
        if self.P_sub[i].weighted and ub is not None:
            raise SipxError(L1W_WEIGHTS_ARE_LB if self.P_sub[i].kind == "l1_weighted" else L21_WEIGHTS_ARE_LB)
        if self.P_sub[i].seg_radii and lb is not None and self.P_sub[i].kind != "annulus":
            raise SipxError(f"set_data: set {i} is an {self.P_sub[i].kind} set: its radii are ub, only the annulus has inner radii (lb)")
        given = [(k, a) for k, a in (("lb", lb), ("ub", ub)) if a is not None]
        if not given:
            return
        on_dev = [_is_tensor(a) for _, a in given]
        if any(on_dev) and not all(on_dev):
            raise SipxError("set_data: lb and ub must both be numpy arrays or both be tensors on the GPU")
        if on_dev[0]:
            for k, t in given:
                _check_tensor(k, t, self.TF, want, None)
            if len(given) == 2 and ub.device != lb.device:
                raise SipxError(f"ub lives on {ub.device}, lb on {lb.device}")
            device = self._device_of(given[0][1])
            _check_one_hip_runtime()
            fn = self._context(device).set_data_dev
        else:
            for k, a in given:
                _check_array(k, a, self.TF, want)
            if self.P_sub[i].kind == "l20" and ub is not None:
                for k in np.asarray(ub).tolist():
                    _check_l20_k(k, int(np.prod(_grid(self.comp_grid)[0][:2])), self.TF)
            elif self.P_sub[i].kind in L2INF_KINDS:
                if ub is not None:
                    _check_l2inf_bounds(ub, self.P_sub[i].per, self.P_sub[i].kind == "l2inf_stacked")
            elif self.P_sub[i].seg_radii and ub is not None:
                _check_l1_radii("l1" if self.P_sub[i].kind == "l21" else self.P_sub[i].kind, ub)
            if self.P_sub[i].weighted and lb is not None:
                _check_l21_weights(self.P_sub[i].kind, lb)
            fn = self._context(self.device).set_data
        try:
            fn(i, lb, ub)
        except BaseException:
            self.close()
            raise

    def __call__(self, m, x=None, l=None, y=None, outputs="all", out=None):
        import time
        t0 = time.perf_counter()
        self._check_open()
        if outputs not in ("all", "x"):
            raise SipxError("outputs must be 'all' or 'x'")
        opt, TF = self.options, self.TF
        on_dev = _is_tensor(m)
        if on_dev:
            _check_device_args(m, x, l, y, out, TF, self.N, self.N, self.rows, outputs)
            device = self._device_of(m)
        else:
            if not isinstance(m, np.ndarray):
                raise SipxError(f"m must be a numpy array or a torch tensor on a GPU, not {type(m).__name__}")
            if out is not None:
                raise SipxError("out takes preallocated tensors: for a numpy m pass x, which is overwritten in place")
            if not (np.isrealobj(m) and (x is None or np.isrealobj(x))):
                raise SipxError("input for PARSDMM is not real")                 # src/PARSDMM.jl:50-52
            _check_array("m", m, TF, self.N)
            for name, a in (("x", x),):
                if a is not None and (_is_tensor(a) or np.shape(a) != (self.N,)):
                    raise SipxError(f"{name} must be a numpy vector of {self.N} entries, like m")
            for name, lst in (("l", l), ("y", y)):
                if lst is not None and len(lst) and (len(lst) != len(self.rows) or any(_is_tensor(a) or np.shape(a) != (r,) for a, r in zip(lst, self.rows))):
                    raise SipxError(f"{name} needs one numpy vector per term (sets plus the distance term) with {self.rows} entries")
            device = self.device
        try:
            dev = None
            if on_dev:
                import torch
                _check_one_hip_runtime()
                dev = torch.device("cuda", device)
            res = _solve(self._context(device), self.built, t0, m, opt, x, l, y, outputs, out, dev)
            self.built = True
        except BaseException:
            self.close()
            raise
        return res

    def close(self):
        self.closed = True
        if self.ctx is not None:
            self.ctx.close()
            self.ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# --------------------------------------------------------------------------------------------------
# kernel-level helpers (parity tests / bench)
# --------------------------------------------------------------------------------------------------
def cds_spmv(R, offsets, x, device=None):
    """y = A x for a CDS matrix (fill! + CDS_MVp_MT, src/argmin_x.jl:72-78)."""
    device = _default_device if device is None else device
    TF = x.dtype.type
    R = np.asfortranarray(R, dtype=TF)
    off = np.ascontiguousarray(offsets, np.int64)
    x = np.ascontiguousarray(x)
    y = np.empty_like(x)
    _chk(lib().sipx_cds_spmv(_dtype_code(TF), C.c_int64(R.shape[0]), int(R.shape[1]), _ptr(R), _ptr(off),
                             _ptr(x), _ptr(y), device))
    return y


def prox_l2s(x, rho, m, device=None):
    """x = (x*rho + m) / (rho + 1.0) in place (src/prox_l2s!.jl:3-6), on the device."""
    device = _default_device if device is None else device
    TF = x.dtype.type
    if not x.flags.c_contiguous or m.dtype != x.dtype or m.shape != x.shape:
        raise SipxError("prox_l2s: x and m must be contiguous vectors of one precision and length")
    m = np.ascontiguousarray(m)
    _chk(lib().sipx_prox_l2s(_dtype_code(TF), C.c_int64(x.size), _ptr(x), C.c_double(float(rho)), _ptr(m), device))
    return x


def resample_nn(a, nc, nf, device=None):
    """Nearest-neighbour grid transfer (Interpolations.BSpline(Constant()) on range(1, stop=nc, length=nf)), on the device."""
    device = _default_device if device is None else device
    a = np.ascontiguousarray(a)
    TF = a.dtype.type
    nc, nf = [int(v) for v in nc], [int(v) for v in nf]
    if a.size != int(np.prod(nc)):
        raise SipxError("resample: array size does not match its shape")
    out = np.empty(int(np.prod(nf)), TF)
    _chk(lib().sipx_resample_nn(_dtype_code(TF), len(nc), (C.c_int64 * len(nc))(*nc), (C.c_int64 * len(nf))(*nf),
                                _ptr(a), _ptr(out), device))
    return out


def segment_norms(x, comp_grid, TD_OP: str, app_mode, norm: str):
    """The l1 or l2 norm of every fiber / slice of A x, A = TD_OP in ("identity", "D_x", "D_y", "D_z"), app_mode = ("fiber" | "slice", d),
    norm in ("l1", "l2"), on a 2-D or 3-D grid: nseg numbers of the working precision (that of x) in the order the per-segment radii of
    setup_constraints(..., segment_norms=True) are read -- a fiber set: the array of shape "TD_n without the fiber's axis", flattened
    in Fortran order; a slice set: the coordinate along d.  Computed by the projector's own first pass (sipx_segment_norms): used as
    radii they leave A x untouched.  x: a numpy vector (a numpy result) or a 1-D torch tensor on a GPU (a tensor there; nothing
    crosses PCIe, the call orders itself against torch's current stream).  Radii for several training arrays: np.maximum / np.minimum
    over the results."""
    if norm not in ("l1", "l2"):
        raise SipxError(f"segment_norms: norm must be 'l1' or 'l2', not {norm!r}")
    if TD_OP not in ("identity", "D_x", "D_y", "D_z"):
        raise SipxError("fiber / slice modes need an operator with one block (identity, D_x, D_y, D_z)")
    am = tuple(app_mode)
    if len(am) != 2 or am[0] not in ("fiber", "slice"):
        raise SipxError(f"segment_norms: app_mode must be ('fiber', d) or ('slice', d), not {app_mode!r}")
    on_dev = _is_tensor(x)
    TF = _tensor_TF("x", x) if on_dev else (x.dtype.type if isinstance(x, np.ndarray) else None)
    if TF not in (np.float32, np.float64):
        raise SipxError("segment_norms: x must be a Float32 or Float64 numpy vector or torch tensor on a GPU")
    return _segment_observe(x, comp_grid, TD_OP, am, TF, on_dev, "l2", "sipx_segment_norms", (0 if norm == "l1" else 1,))


def _segment_observe(x, comp_grid, TD_OP, am, TF, on_dev, set_type, fn_name, extra):
    """What segment_norms and segment_sums share: one number per fiber / slice of A x by the library call fn_name (its _dev form for a
    tensor), in a context of its own; set_type names the set whose mode, direction and refusals apply."""
    n, _ = _grid(comp_grid)
    if TD_OP == "D_y" and len(n) == 2:
        raise SipxError("provided an unknown transform domain operator. check function get_TD_operator(comp_grid,TD_type,TF) for options")
    P = Projector(set_definitions(set_type, TD_OP, 0.0, 1.0, am), comp_grid, TF)      # mode, direction and their refusals
    nseg = P.nseg(TDOperator(TD_OP, comp_grid, TF))
    N = int(np.prod(n))
    if on_dev:
        import torch
        _check_tensor("x", x, TF, N, None)
        _check_one_hip_runtime()
        device = x.device.index if x.device.index is not None else torch.cuda.current_device()
        out = torch.empty(nseg, dtype=x.dtype, device=torch.device("cuda", device))
        xp, op_ = C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr())
        fn = getattr(lib(), fn_name + "_dev")
    else:
        x = _check_array("x", x, TF, N)
        device = None
        out = np.empty(nseg, TF)
        xp, op_ = _ptr(x), _ptr(out)
        fn = getattr(lib(), fn_name)
    ctx = Context(comp_grid, TF, device)
    try:
        if on_dev:
            ctx.set_caller_stream(torch.cuda.current_stream(x.device).cuda_stream)
        cnt = C.c_int64()
        _chk(fn(ctx.h, OPS[TD_OP], P.mode, P.dir, *extra, None, None, C.byref(cnt)))      # the count only
        if cnt.value != nseg:
            raise SipxError(f"internal: the engine counts {cnt.value} segments, the host {nseg}")
        _chk(fn(ctx.h, OPS[TD_OP], P.mode, P.dir, *extra, xp, op_, C.byref(cnt)))
    finally:
        ctx.close()
    return out


def segment_sums(x, comp_grid, TD_OP: str, app_mode):
    """The sum of the positive parts of every fiber / slice of A x, sum_i max((A x)_i, 0): nseg numbers of the working precision (that of
    x) in the order of segment_norms(), arguments as there.  Computed by pass 1 of the ("simplex", TD_OP, app_mode) projector
    (sipx_segment_sums, csrc/seg_simplex.h): the very numbers it compares with min and max, so a nonnegative A x is not written by a
    simplex set built with min = the smallest and max = the largest of them.  x: a numpy vector or a 1-D torch tensor on a GPU."""
    if TD_OP in SPECIAL_OPERATORS:
        raise SipxError(SIMPLEX_NO_TRANSFORM)
    if TD_OP not in ONE_BLOCK_OPERATORS:
        raise SipxError(SIMPLEX_ONE_BLOCK)
    am = tuple(app_mode)
    if len(am) != 2 or am[0] not in ("fiber", "slice"):
        raise SipxError(SIMPLEX_NEEDS_MODE)
    on_dev = _is_tensor(x)
    TF = _tensor_TF("x", x) if on_dev else (x.dtype.type if isinstance(x, np.ndarray) else None)
    if TF not in (np.float32, np.float64):
        raise SipxError("segment_sums: x must be a Float32 or Float64 numpy vector or torch tensor on a GPU")
    return _segment_observe(x, comp_grid, TD_OP, am, TF, on_dev, "simplex", "sipx_segment_sums", ())


def group_norms(x, comp_grid, TD_OP: str, app_mode):
    """The l2 norm of every fiber / slice of A x: nseg numbers g of the working precision (that of x) in the order of segment_norms(),
    arguments as there.  Computed by the norms launch of the ("card_groups", TD_OP, app_mode) projector (sipx_group_norms,
    csrc/card_groups.h): the very array it selects on -- it keeps the first k segments of the stable descending order of g (ties to the
    lower index), so k can be picked from the sorted values.  The count the projector compares with k is count_nonzero(group_norms):
    at most k non-zero norms and it writes nothing.  Fibers: the bits of segment_norms(..., "l2"); slices: chunked compensated sums,
    within one unit in the last place of the exactly summed norm.  x: a numpy vector or a 1-D torch tensor on a GPU."""
    if TD_OP in SPECIAL_OPERATORS:
        raise SipxError(CARDG_NO_TRANSFORM)
    if TD_OP not in ONE_BLOCK_OPERATORS:
        raise SipxError(CARDG_ONE_BLOCK)
    am = tuple(app_mode)
    if len(am) != 2 or am[0] not in ("fiber", "slice"):
        raise SipxError(CARDG_NEEDS_MODE)
    on_dev = _is_tensor(x)
    TF = _tensor_TF("x", x) if on_dev else (x.dtype.type if isinstance(x, np.ndarray) else None)
    if TF not in (np.float32, np.float64):
        raise SipxError("group_norms: x must be a Float32 or Float64 numpy vector or torch tensor on a GPU")
    return _segment_observe(x, comp_grid, TD_OP, am, TF, on_dev, "card_groups", "sipx_group_norms", ())


def tv_group_norms(x, comp_grid, TD_OP: str = "TV", joint: bool = False):
    """The norms of the gradient groups of TV x (TD_OP "TV", "D2D", "D3D" or "TV_xy"): N numbers g of the working precision (that of x) in
    grid-point order (column-major), or with joint=True the n1 n2 numbers of the pixels of TV_xy across all frames.  Computed by the norms
    launch of the ("l20", TD_OP) / ("l20_joint", "TV_xy") projector (sipx_tv_group_norms, csrc/l20.h), which is the one of the l21 /
    l21_joint sets: the very array the set selects on -- it keeps the first k groups of the stable descending order of g (ties to the
    lower index), so k can be picked from the sorted values; per frame it selects on g[frame] of g.reshape(n3, n1 n2).  The count the
    projector compares with k is count_nonzero(g).  x: a numpy vector or a 1-D torch tensor on a GPU."""
    if TD_OP in SPECIAL_OPERATORS:
        raise SipxError(L20_NO_TRANSFORM)
    if joint and TD_OP != "TV_xy":
        raise SipxError(L20_JOINT_ROUTE)
    if TD_OP not in TV_OPERATORS + ("TV_xy",):
        raise SipxError(L20_NEEDS_TV)
    on_dev = _is_tensor(x)
    TF = _tensor_TF("x", x) if on_dev else (x.dtype.type if isinstance(x, np.ndarray) else None)
    if TF not in (np.float32, np.float64):
        raise SipxError("tv_group_norms: x must be a Float32 or Float64 numpy vector or torch tensor on a GPU")
    n, _ = _grid(comp_grid)
    if TD_OP == "TV_xy" and len(n) != 3:
        raise SipxError(TV_XY_NEEDS_3D)
    N = int(np.prod(n))
    ng = int(n[0]) * int(n[1]) if joint else N
    if on_dev:
        import torch
        _check_tensor("x", x, TF, N, None)
        _check_one_hip_runtime()
        device = x.device.index if x.device.index is not None else torch.cuda.current_device()
        out = torch.empty(ng, dtype=x.dtype, device=torch.device("cuda", device))
        xp, op_ = C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr())
        fn = lib().sipx_tv_group_norms_dev
    else:
        x = _check_array("x", x, TF, N)
        device = None
        out = np.empty(ng, TF)
        xp, op_ = _ptr(x), _ptr(out)
        fn = lib().sipx_tv_group_norms
    ctx = Context(comp_grid, TF, device)
    try:
        if on_dev:
            ctx.set_caller_stream(torch.cuda.current_stream(x.device).cuda_stream)
        cnt = C.c_int64()
        _chk(fn(ctx.h, OPS[TD_OP], int(bool(joint)), None, None, C.byref(cnt)))      # the count only
        if cnt.value != ng:
            raise SipxError(f"internal: the engine counts {cnt.value} groups, the host {ng}")
        _chk(fn(ctx.h, OPS[TD_OP], int(bool(joint)), xp, op_, C.byref(cnt)))
    finally:
        ctx.close()
    return out


def _l21_observe(name, x, comp_grid, needs_3d, per_frame, fn, before, after, weights=None, groups=0, no_weights=()):
    """What l21_norm and l21_joint_norm share: x, a numpy vector or a 1-D torch tensor on a GPU, goes through the library call
    fn(ctx, *before, x, out, *after) -- its _dev form for a tensor, ordered against torch's current stream -- in a context of its
    own.  out: n3 entries (per_frame) or one, of the kind and precision of x.  weights (`groups` entries, of the kind and precision of
    x) go between x and out: fn(ctx, *before, x, weights, out); no_weights: what takes their place when there are none (a call whose
    weights argument may be NULL passes (None,)).  Returns (out, x is a tensor)."""
    on_dev = _is_tensor(x)
    TF = _tensor_TF("x", x) if on_dev else (x.dtype.type if isinstance(x, np.ndarray) else None)
    if TF not in (np.float32, np.float64):
        raise SipxError(f"{name}: x must be a Float32 or Float64 numpy vector or torch tensor on a GPU")
    n, _ = _grid(comp_grid)
    N = int(np.prod(n))
    if needs_3d and len(n) != 3:
        raise SipxError(TV_XY_NEEDS_3D)
    nout = int(n[2]) if per_frame else 1
    if on_dev:
        import torch
        _check_tensor("x", x, TF, N, None)
        _check_one_hip_runtime()
        device = x.device.index if x.device.index is not None else torch.cuda.current_device()
        out = torch.empty(nout, dtype=x.dtype, device=torch.device("cuda", device))
        xp, op_ = C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr())
        if weights is not None:
            if not _is_tensor(weights):
                raise SipxError(f"{name}: x is a tensor on the GPU, the weights must be one too")
            _check_tensor("weights", weights, TF, groups, x.device)
            mid = (C.c_void_p(weights.data_ptr()),)
    else:
        x = _check_array("x", x, TF, N)
        device = None
        out = np.empty(nout, TF)
        xp, op_ = _ptr(x), _ptr(out)
        if weights is not None:
            weights = _check_array("weights", weights, TF, groups)
            _check_l21_weights(name, weights)
            mid = (_ptr(weights),)
    if weights is None:
        mid = tuple(no_weights)
    ctx = Context(comp_grid, TF, device)
    try:
        if on_dev:
            ctx.set_caller_stream(torch.cuda.current_stream(x.device).cuda_stream)
        _chk(getattr(lib(), fn + ("_dev" if on_dev else ""))(ctx.h, *before, xp, *mid, op_, *after))
    finally:
        ctx.close()
    return out, on_dev


def l21_stacked_norm(x, comp_grid, TD_OP, blocks=None):
    """sum_p ||(A x)_p||_2 over the groups of the stacked l2,1 ball (csrc/l21_stacked.h), one number of the working precision (that of
    x): TD_OP = "Hessian" gives sum_p ||H x(p)||_F, the second-order total variation of x (blocks: None); TD_OP a sparse matrix with
    N columns and M rows gives the norm of the ("l21_stacked", ...) set on it, blocks = B its equal-sized blocks.  Computed by the
    engine's sparse product, the norms kernel and the first-pass sum of the projector (sipx_l21_stacked_norm): used as the radius it
    leaves A x untouched.  x: a numpy vector (a numpy scalar comes back) or a 1-D torch tensor on a GPU (a tensor of one entry there;
    nothing of x crosses PCIe, the call orders itself against torch's current stream)."""
    TF = _tensor_TF("x", x) if _is_tensor(x) else (x.dtype.type if isinstance(x, np.ndarray) else None)
    if TF not in (np.float32, np.float64):
        raise SipxError("l21_stacked_norm: x must be a Float32 or Float64 numpy vector or torch tensor on a GPU")
    named = isinstance(TD_OP, str)
    if named and TD_OP != "Hessian":
        raise SipxError(L21S_NEEDS_CSC)
    c = set_definitions("l21_stacked", "Hessian" if named else "custom", 0.0, 1.0, ("matrix", ""),
                        custom_TD_OP=((), False) if named else (TD_OP, False), blocks=blocks)
    P = Projector(c, comp_grid, TF)
    op = hessian_operator(comp_grid, TF) if named else CustomOperator(TD_OP, comp_grid, TF)
    P.check_rows(op)
    d = P.desc("custom", False)
    cp = np.ascontiguousarray(op.A.indptr, np.int64); ri = np.ascontiguousarray(op.A.indices, np.int64)
    nz = np.ascontiguousarray(op.A.data, TF)
    d.csc_colptr, d.csc_rowval, d.csc_nzval, d.csc_rows = cp.ctypes.data, ri.ctypes.data, nz.ctypes.data, int(op.A.shape[0])
    out, on_dev = _l21_observe("l21_stacked_norm", x, comp_grid, False, False, "sipx_l21_stacked_norm", (C.byref(d),), ())
    return out if on_dev else out[0]


def l2inf_norm(x, comp_grid, TD_OP="TV", joint=False, blocks=None):
    """max_p ||(A x)_p||_2 over the groups of the l2,inf sets (csrc/l2inf.h), one number of the working precision (that of x): the
    steepest gradient magnitude of x for TD_OP "TV" ("D2D", "D3D") or "TV_xy", with joint=True the largest norm over the pixels of TV_xy
    across all frames, for TD_OP = "Hessian" the largest Frobenius norm of the Hessian, for TD_OP a sparse matrix with N columns the
    largest group norm across its `blocks` equal-sized blocks.  Computed by the projector's own norms launch and a two-stage maximum
    (sipx_l2inf_norm): a set built with the value as its bound leaves A x untouched.  x: a numpy vector (a numpy scalar comes back) or a
    1-D torch tensor on a GPU (a tensor of one entry there)."""
    TF = _tensor_TF("x", x) if _is_tensor(x) else (x.dtype.type if isinstance(x, np.ndarray) else None)
    if TF not in (np.float32, np.float64):
        raise SipxError("l2inf_norm: x must be a Float32 or Float64 numpy vector or torch tensor on a GPU")
    named = isinstance(TD_OP, str)
    if named and TD_OP != "Hessian":
        c = set_definitions("l2inf_joint" if joint else "l2inf", TD_OP, 0.0, 1.0, ("matrix", ""))
        P = Projector(c, comp_grid, TF)
        d = P.desc(P.op, False)
        keep = ()
    else:
        if joint:
            raise SipxError(L2INF_JOINT_ROUTE)
        c = set_definitions("l2inf_stacked", "Hessian" if named else "custom", 0.0, 1.0, ("matrix", ""),
                            custom_TD_OP=((), False) if named else (TD_OP, False), blocks=blocks)
        P = Projector(c, comp_grid, TF)
        op = hessian_operator(comp_grid, TF) if named else CustomOperator(TD_OP, comp_grid, TF)
        P.check_rows(op)
        d = P.desc("custom", False)
        keep = (np.ascontiguousarray(op.A.indptr, np.int64), np.ascontiguousarray(op.A.indices, np.int64), np.ascontiguousarray(op.A.data, TF))
        d.csc_colptr, d.csc_rowval, d.csc_nzval, d.csc_rows = keep[0].ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data, int(op.A.shape[0])
    out, on_dev = _l21_observe("l2inf_norm", x, comp_grid, False, False, "sipx_l2inf_norm", (C.byref(d),), ())
    del keep
    return out if on_dev else out[0]


def l21_norm(x, comp_grid, TD_OP: str = "TV", app_mode=None, weights=None):
    """||TV x||_2,1, the isotropic total variation of x on a 2-D or 3-D grid: sum over the grid points of the l2 norm of the forward
    differences that start there, one number of the working precision (that of x).  Computed by the kernel and the first-pass sum of
    the ("l21", "TV") projector (sipx_l21_norm): used as the radius it leaves TV x untouched.  x: a numpy vector (a numpy scalar
    comes back) or a 1-D torch tensor on a GPU (a tensor of one entry there; nothing crosses PCIe, the call orders itself against
    torch's current stream).

    TD_OP = "TV_xy" (3-D grids) observes the in-plane gradient vcat(D_y, D_x) instead.  With app_mode = ("slice", "z") the n3 per-frame
    norms come back (an array / a tensor of n3 entries): the sums of the group norms of every z-slice as the per-frame projector
    ("l21", "TV_xy", ("slice", "z")) compares them with its radii (sipx_l21_norms), so radii observed on x leave TV_xy x unwritten.

    weights (whole array only): one weight >= 0 per grid point in column-major order, of the kind and precision of x -- the weighted
    norm sum_p w_p g_p as the first pass of the weighted projector sums it (sipx_l21_weighted_norm, csrc/l21_weighted.h)."""
    if TD_OP not in TV_OPERATORS + ("TV_xy",):
        raise SipxError(L21_NEEDS_TV)
    mode, dirn = 0, 0
    if app_mode is not None and tuple(app_mode)[0] not in ("matrix", "tensor"):
        if TD_OP != "TV_xy":
            raise SipxError(L21_WHOLE_ONLY)
        if tuple(app_mode) != ("slice", "z"):
            raise SipxError(L21_FRAMES_Z)
        mode, dirn = MODES["slice"], 2
    if weights is not None:
        if mode:
            raise SipxError(L21_WEIGHTS_NO_FRAMES)
        out, on_dev = _l21_observe("l21_norm", x, comp_grid, TD_OP == "TV_xy", False, "sipx_l21_weighted_norm", (OPS[TD_OP], 0), (),
                                   weights, int(np.prod(_grid(comp_grid)[0])))
        return out if on_dev else out[0]
    out, on_dev = _l21_observe("l21_norm", x, comp_grid, TD_OP == "TV_xy", bool(mode), "sipx_l21_norms", (OPS[TD_OP], mode, dirn), (None,))
    return out if (on_dev or mode) else out[0]


def l21_groups_norm(x, comp_grid, TD_OP: str, app_mode, weights=None):
    """sum_s w_s ||(A x)[segment s]||_2 over the fibers / slices of A x, A = TD_OP one of identity, D_x, D_y, D_z: one number of the
    working precision (that of x), (T)asum as the norms launch and the first pass of the ("l21_groups", TD_OP, app_mode) projector sum
    and compare it (sipx_l21_groups_norm, csrc/l21_groups.h) -- used as the radius it leaves A x unwritten.  x: a numpy vector (a numpy
    scalar comes back) or a 1-D torch tensor on a GPU (a tensor of one entry there; nothing crosses PCIe, the call orders itself
    against torch's current stream).  weights: one finite weight >= 0 per segment in the order of segment_norms(), of the kind and
    precision of x; None: every weight 1."""
    TF = _tensor_TF("x", x) if _is_tensor(x) else (x.dtype.type if isinstance(x, np.ndarray) else None)
    if TF not in (np.float32, np.float64):
        raise SipxError("l21_groups_norm: x must be a Float32 or Float64 numpy vector or torch tensor on a GPU")
    P = Projector(set_definitions("l21_groups", TD_OP, 0.0, 1.0, tuple(app_mode)), comp_grid, TF)      # mode, direction and the refusals
    nseg = P.nseg(TDOperator(TD_OP, comp_grid, TF))
    fn = "sipx_l21_groups_norm"
    if weights is None:
        out, on_dev = _l21_observe("l21_groups_norm", x, comp_grid, False, False, fn, (OPS[TD_OP], P.mode, P.dir), (), None, 0, (None,))
    else:
        out, on_dev = _l21_observe("l21_groups_norm", x, comp_grid, False, False, fn, (OPS[TD_OP], P.mode, P.dir), (), weights, nseg)
    return out if on_dev else out[0]


def l1_weighted_norm(x, comp_grid, TD_OP: str, weights):
    """sum_i w_i |(A x)_i| over the rows of A = TD_OP, one of identity, D_x, D_y, D_z, TV (D2D, D3D), TV_xy: one number of the working
    precision (that of x), (T)asum as the first pass of the ("l1_weighted", TD_OP) projector sums and compares it
    (sipx_l1_weighted_norm, csrc/l1_weighted.h) -- used as the radius it leaves A x unwritten.  x: a numpy vector (a numpy scalar comes
    back) or a 1-D torch tensor on a GPU (a tensor of one entry there; nothing crosses PCIe, the call orders itself against torch's
    current stream).  weights: one finite weight >= 0 per row of A in the order of A @ x, of the kind and precision of x."""
    TF = _tensor_TF("x", x) if _is_tensor(x) else (x.dtype.type if isinstance(x, np.ndarray) else None)
    if TF not in (np.float32, np.float64):
        raise SipxError("l1_weighted_norm: x must be a Float32 or Float64 numpy vector or torch tensor on a GPU")
    if weights is None:
        raise SipxError(L1W_NEEDS_WEIGHTS)
    if TD_OP in SPECIAL_OPERATORS:
        raise SipxError(L1W_NO_TRANSFORM)
    if TD_OP not in L1W_OPERATORS:
        raise SipxError(L1W_NO_CUSTOM if TD_OP == "D_xz" else UNKNOWN_OPERATOR)
    rows = TDOperator(TD_OP, comp_grid, TF).shape[0]           # (TV_xy, D_y on a 2-D grid: refused here)
    out, on_dev = _l21_observe("l1_weighted_norm", x, comp_grid, TD_OP == "TV_xy", False, "sipx_l1_weighted_norm", (OPS[TD_OP],), (),
                               weights, rows)
    return out if on_dev else out[0]


def l21_joint_norm(x, comp_grid, weights=None):
    """The joint (vectorial) total variation of the frames of x on a 3-D grid: the sum over the pixels (i, j) of the l2 norm of all
    in-plane differences that start at that pixel in any frame, one number of the working precision (that of x).  Computed by the
    z-march and the first-pass sum of the ("l21_joint", "TV_xy") projector (sipx_l21_joint_norm): used as the radius it leaves TV_xy x
    unwritten.  x: a numpy vector (a numpy scalar comes back) or a 1-D torch tensor on a GPU (a tensor of one entry there; nothing
    crosses PCIe, the call orders itself against torch's current stream).  weights: one weight >= 0 per pixel (n1 n2 entries, pixel
    order), of the kind and precision of x -- the weighted norm as the weighted projector sums it (sipx_l21_weighted_norm)."""
    if weights is not None:
        n, _ = _grid(comp_grid)
        if len(n) != 3:
            raise SipxError(TV_XY_NEEDS_3D)
        out, on_dev = _l21_observe("l21_joint_norm", x, comp_grid, True, False, "sipx_l21_weighted_norm", (OPS["TV_xy"], 1), (),
                                   weights, int(n[0]) * int(n[1]))
        return out if on_dev else out[0]
    out, on_dev = _l21_observe("l21_joint_norm", x, comp_grid, True, False, "sipx_l21_joint_norm", (), ())
    return out if on_dev else out[0]


def tnv_norm(x, comp_grid):
    """The total nuclear variation of the frames of x on a 3-D grid: the sum over the pixels (i, j) of the nuclear norm of the 2 x n3
    matrix whose column k is (D_y x, D_x x) at that pixel in frame k, one number of the working precision (that of x).  Computed by
    the Gram march, the decomposition and the first-pass sum of the ("tnv", "TV_xy") projector (sipx_tnv_norm): used as the radius it
    leaves TV_xy x unwritten.  x: a numpy vector (a numpy scalar comes back) or a 1-D torch tensor on a GPU (a tensor of one entry
    there; nothing crosses PCIe, the call orders itself against torch's current stream)."""
    out, on_dev = _l21_observe("tnv_norm", x, comp_grid, True, False, "sipx_tnv_norm", (), ())
    return out if on_dev else out[0]


def _dwt_check_grid(n):
    """The grids the wavelet transform takes: 2-D or 3-D, every dimension divisible by 2^L, L = maxtransformlevels(min(n))."""
    n = tuple(int(v) for v in n)
    if len(n) not in (2, 3):
        raise SipxError("wavelet transform: 2-D and 3-D grids only")
    m, L = min(n), 0
    while m > 0 and m % 2 == 0:
        m //= 2
        L += 1
    for a, v in enumerate(n):
        if v % (1 << L):
            raise SipxError(f"wavelet transform: the grid {' x '.join(map(str, n))} has {L} levels (2^L divides the smallest "
                            f"dimension) but dimension {a + 1} is not divisible by 2^{L}")
    return L


def dwt(x, n, inverse=False, device=None):
    """W x (or W' x with inverse=True): the orthonormal periodic multilevel db4 transform behind TD_OP = "wavelet"
    (sipx.h, SIPX_TRANSFORM_WAVELET) of the column-major grid n, on the device.  ||W x||_1 sets the radius of an l1 ball
    behind it (src/constraint_learning_by_observation.jl:68,114)."""
    device = _default_device if device is None else device
    x = np.ascontiguousarray(x)
    TF = x.dtype.type
    n = [int(v) for v in n]
    if len(n) == 3 and n[2] == 1:
        n = n[:2]
    _dwt_check_grid(n)
    if x.size != int(np.prod(n)):
        raise SipxError("dwt: array size does not match the grid")
    x = x.reshape(-1)
    out = np.empty(x.size, TF)
    _chk(lib().sipx_dwt(_dtype_code(TF), len(n), (C.c_int64 * len(n))(*n), int(bool(inverse)), _ptr(x), _ptr(out), device))
    return out


# keys of the reference's dictionary (src/constraint_learning_by_observation.jl:27-58), in its order and in sipx_observations'
LEARN_KEYS = ("nuclear_norm", "nuclear_Dx", "nuclear_Dz", "rank_095", "TV", "wavelet_l1", "Dx_l1", "Dz_l1", "DFT_l1", "DFT_card_095",
              "TV_card_095", "annulus", "TV_annulus", "D_l2", "D_x_min", "D_x_max", "D_z_min", "D_z_max", "DCT_x_LB", "DCT_x_UB",
              "DCT_y_LB", "DCT_y_UB", "hist_min", "hist_max", "hist_TV_min", "hist_TV_max")


class _Observations(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in LEARN_KEYS]


def _learn_layout(n, TF, n_train):
    """Length and dtype of every key (sipx.h, sipx_observations)."""
    n1, n2 = n
    N, M = n1 * n2, (n1 - 1) * n2 + n1 * (n2 - 1)
    TI = np.int32 if TF == np.float32 else np.int64
    lay = {k: (n_train, TF) for k in LEARN_KEYS}
    lay.update({k: (n_train, TI) for k in ("rank_095", "DFT_card_095", "TV_card_095")})
    lay.update({"hist_min": (N, np.float64), "hist_max": (N, TF), "hist_TV_min": (M, np.float64), "hist_TV_max": (M, TF),
                "DCT_x_LB": (n1, np.float64), "DCT_x_UB": (n1, TF), "DCT_y_LB": (n2, np.float64), "DCT_y_UB": (n2, TF)})
    return lay


def constraint_learning_by_obseration(comp_grid, m_train, keys=None, max_batch=0, device=None):
    """src/constraint_learning_by_observation.jl:8-163 (the reference's spelling; constraint_learning_by_observation is an
    alias): a dict of statistics of the training images m_train[i, :, :] on the 2-D grid, computed on the device.

    m_train is (n_train, n1, n2) in C or Fortran order (numpy strides are passed through), or one (n1, n2) image.  keys selects
    what is computed (default: every key of the reference); a key not asked for costs nothing.  max_batch bounds the images per
    device chunk (0: from free memory); every chunking gives the same bits.  Dtypes and lengths: include/sipx.h.  As in the
    reference, the *_min / *_LB arrays start at 1e8 and are float64 (Julia promotes zeros(TF, n) .+ 1e8), the *_max / *_UB
    arrays start at 0 in TF.  Unlike the reference, a count whose magnitudes are all zero is 0 (Julia throws), the cumulative
    sums run in float64, and wavelet_l1 is 0 unless n1 == n2."""
    n = tuple(int(v) for v in comp_grid.n)
    if len(n) == 3 and n[2] == 1:
        n = n[:2]
    if len(n) != 2:
        raise SipxError("constraint learning: 2-D grids only")
    if n[0] < 2 or n[1] < 2:
        raise SipxError("constraint learning: the grid needs n1 >= 2 and n2 >= 2")
    h = tuple(float(v) for v in comp_grid.d[:2])
    m = np.asarray(m_train)
    if np.iscomplexobj(m) or m.dtype.type not in (np.float32, np.float64):
        raise SipxError("constraint learning: m_train must be real Float32 or Float64")
    if m.ndim == 2:
        m = m[None]
    if m.ndim != 3 or m.shape[1:] != n or m.shape[0] < 1:
        raise SipxError(f"constraint learning: m_train of shape {np.shape(m_train)} does not match the grid {n}")
    wanted = LEARN_KEYS if keys is None else tuple(keys)
    for k in wanted:
        if k not in LEARN_KEYS:
            raise SipxError(f"constraint learning: unknown key {k!r}")
    if not (m.flags.c_contiguous or m.flags.f_contiguous):
        m = np.ascontiguousarray(m)
    TF = m.dtype.type
    device = _default_device if device is None else device
    lay = _learn_layout(n, TF, m.shape[0])
    out = {k: np.empty(lay[k][0], lay[k][1]) for k in LEARN_KEYS if k in wanted}
    obs = _Observations(**{k: v.ctypes.data for k, v in out.items()})
    strides = (C.c_int64 * 3)(*[s // m.itemsize for s in m.strides])
    _chk(lib().sipx_learn_observations(_dtype_code(TF), (C.c_int64 * 2)(*n), (C.c_double * 2)(*h), C.c_int64(m.shape[0]),
                                       _ptr(m), strides, C.c_int64(int(max_batch)), C.byref(obs), int(device)))
    return out


constraint_learning_by_observation = constraint_learning_by_obseration


def CDS_MVp(N, ndiags, R, offset, x, y):
    """Reference signature (src/CDS_MVp.jl:9-28): y += A x."""
    y += cds_spmv(R, offset, x)
    return y
