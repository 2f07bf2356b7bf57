# SipxPARSDMM.jl -- PARSDMM on one MI355X through libsipx.so (include/sipx.h), with the EXACT positional signature of the
# reference's entry point (src/PARSDMM.jl:25-35):
#
#     PARSDMM(m, AtA, TD_OP, set_Prop, P_sub, comp_grid, options[, x, l, y]) -> (x, log_PARSDMM, l, y)
#
# so that `(x, log) = PARSDMM(m, AtA, TD_OP, set_Prop, P_sub, comp_grid, options)` in a caller's script
# (examples/projection_intersection_2D.jl:81) needs no edit: `include("SipxPARSDMM.jl"); using .SipxPARSDMM: PARSDMM` in place of
# `using SetIntersectionProjection: PARSDMM`.
#
# NOT EXECUTED anywhere in this repository's pipeline: neither the build container nor the GPU box has a Julia toolchain
# (SURVEY 8c).  The C side of every call below IS exercised -- tests/c_abi/phases.c drives the same sequence of entry points
# from plain C and tests/test_gpu_parity.py drives it through ctypes.
#
# How the opaque inputs are recovered:
#   * P_sub[i] is a closure built by get_projector (src/get_projector.jl:3-103); EVERY branch captures the `constraint`
#     it was built from, so `getfield(P_sub[i], :constraint)` returns the set_definitions (set_type, TD_OP, min, max,
#     app_mode, custom_TD_OP) -- the projector descriptor;
#   * TD_OP[i] is described by set_Prop.tag[i] = (set_type, TD_OP name, app_mode[1], app_mode[2]) (src/setup_constraints.jl:86)
#     and comp_grid.n / .d; a constraint.custom_TD_OP[1] sparse matrix travels as its CSC arrays;
#   * AtA[i] (CDS, N x d_i) and set_Prop.AtA_offsets[i] are passed as they are (src/PARSDMM_precompute_distribute.jl:52-59).
module SipxPARSDMM

using SparseArrays
using TimerOutputs
import SetIntersectionProjection: log_type_PARSDMM, convert_options!

export PARSDMM, release_contexts, constraint_learning_by_obseration, setup_constraints

const libsipx = get(ENV, "SIPX_LIBRARY", "libsipx.so")

# ---- mirrors of the C structs (include/sipx.h) ---------------------------------------------------------------------
struct SipxSetDesc                     # sipx_set_desc
    op::Int32; proj::Int32
    pmin::Float64; pmax::Float64
    lb::Ptr{Cvoid}; ub::Ptr{Cvoid}
    ncvx::Int32; reserved::Int32
    mode::Int32; dir::Int32
    basis::Ptr{Cvoid}; basis_rows::Int64; basis_cols::Int32; basis_orth::Int32
    component::Int32
    csc_colptr::Ptr{Int64}; csc_rowval::Ptr{Int64}; csc_nzval::Ptr{Cvoid}; csc_rows::Int64
    transform::Int32; pad_::Int32
    blocks::Int32; pad2_::Int32          # SIPX_PROJ_L21_STACKED: the equal-sized blocks of the stacked operator; 0 otherwise
end

struct SipxOptions                     # sipx_options
    maxit::Int32
    evol_rel_tol::Float64; feas_tol::Float64; obj_tol::Float64
    rho_update_frequency::Int32
    adjust_rho::Int32; adjust_gamma::Int32; adjust_feasibility_rho::Int32
end

mutable struct SipxLog                 # sipx_log: flat row-major arrays the caller allocates for maxit rows
    set_feasibility::Ptr{Float64}; r_dual::Ptr{Float64}; r_pri::Ptr{Float64}
    r_dual_total::Ptr{Float64}; r_pri_total::Ptr{Float64}; obj::Ptr{Float64}; evol_x::Ptr{Float64}
    rho::Ptr{Float64}; gamma::Ptr{Float64}; cg_it::Ptr{Int64}; cg_relres::Ptr{Float64}
    timing_ms::NTuple{7,Float64}
    n_iter::Int32; n_feas_rows::Int32; stopped_feasible::Int32
end

const OPS  = Dict("identity" => 0, "D_x" => 1, "D_y" => 2, "D_z" => 3, "TV" => 4, "D2D" => 4, "D3D" => 4,
                 "TV_xy" => 6)      # (libsipx's own in-plane gradient of a 3-D grid: SIPX_OP_TV_XY)
# SIPX_OP_TV_XY (include/sipx.h): the in-plane gradient [D_y; D_x] of a 3-D grid, libsipx's own.  The reference's get_TD_operator has no
# such name, so setup_constraints of this shim cannot build the set; the code is mirrored for callers of the C ABI.
const SIPX_OP_TV_XY = 6
const SIPX_PROJ_TNV = 17     # total nuclear variation on the range of TV_xy (include/sipx.h), set_type = "tnv"
# the weighted l1 ball { sum_i w_i |(A x)_i| <= max } with one weight per row of identity, D_x, D_y, D_z, TV or TV_xy in lb, reserved = the
# rows (include/sipx.h, csrc/l1_weighted.h), set_type = "l1_weighted".  The reference's set_definitions has no field for weights and this
# binding does not carry them: the constant is mirrored for callers of the C ABI, projector_fields refuses the tag and names ("l1", op).
const SIPX_PROJ_L1_WEIGHTED = 18
# simplex sets: every fiber / slice of the range of identity, D_x, D_y or D_z has entries >= 0 and a sum in [min, max] (include/sipx.h,
# csrc/seg_simplex.h), set_type = "simplex".  The reference's setup_constraints cannot set such a set up and this binding does not build it
# yet: the constant is mirrored for callers of the C ABI, projector_fields refuses the tag and names the stand-in.
const SIPX_PROJ_SIMPLEX = 19
# group cardinality: at most k non-zero fibers / slices of the range of identity, D_x, D_y or D_z (include/sipx.h, csrc/card_groups.h),
# set_type = "card_groups", max = k, min ignored.  Not a set of the reference; its setup_constraints leaves ncvx false for an unknown
# tag, so set set_Prop.ncvx[i] = true for such a set, as for cardinality and rank.
const SIPX_PROJ_CARD_GROUPS = 20
# the l2,0 sets on the gradient groups of TV / TV_xy (include/sipx.h, csrc/l20.h), set_type = "l20" and "l20_joint", max = k
const SIPX_PROJ_L20 = 21
const SIPX_PROJ_L20_JOINT = 22
# the l2,1 ball across the equal-sized blocks of a caller-supplied stacked operator (include/sipx.h, csrc/l21_stacked.h), set_type =
# "l21_stacked", custom_TD_OP = (A, false) with A = [A_0; ...; A_{B-1}] a SparseMatrixCSC of M = B G rows, max = the radius.  The
# reference's set_definitions has no field for B: it travels in min (an integer 1 .. 8), which the set does not use otherwise.
# With A the Hessian of the grid (D_11, D_22[, D_33], sqrt(2) D_12[, sqrt(2) D_13, sqrt(2) D_23], each zero-padded to N rows) this is
# second-order isotropic TV; the Python front end assembles that operator under the name "Hessian".
const SIPX_PROJ_L21_STACKED = 23
# the l2,inf ball: every group norm of TV / TV_xy (l2inf), of the pixels of TV_xy across the frames (l2inf_joint) or across the blocks of
# a stacked operator (l2inf_stacked) at most max (include/sipx.h, csrc/l2inf.h), set_type = "l2inf" / "l2inf_joint"; min must be 0, max is
# one positive number or a vector with one bound >= 0 per group (it travels in ub, its length in the descriptor's `reserved`)
const SIPX_PROJ_L2INF = 24
const SIPX_PROJ_L2INF_JOINT = 25
const SIPX_PROJ_L2INF_STACKED = 26
const MODE = Dict("matrix" => 0, "tensor" => 0, "fiber" => 1, "slice" => 2)
const SPECIAL = ("DFT", "DCT", "wavelet", "curvelet")          # src/setup_constraints.jl:54
# the seven @timeit sections of src/PARSDMM.jl:40,100,105,113,152,163,229
const SECTIONS = ("initialization", "form rhs for linear system", "argmin x", "argmin y and l update",
                  "stopping conditions check", "adjust rho and gamma", "Q-update")

check(rc) = rc == 0 || error(unsafe_string(ccall((:sipx_last_error, libsipx), Cstring, ())))

"0-based array dimension of an application direction: x = 0, y = 1, z = last"
dir_of(d::AbstractString, ndim::Int) = d == "x" ? 0 : d == "y" ? 1 : d == "z" ? ndim - 1 : 0

"(proj kind, pmin, pmax, lb, ub, transform) of one constraint -- the branches of get_projector (src/get_projector.jl:3-103)"
function projector_fields(c, TF)
    st, op = c.set_type, c.TD_OP
    vecb = (c.min isa AbstractVector) && length(c.min) > 1
    nothing_ = (0.0, 0.0, nothing, nothing, Int32(0))
    if op == "DCT"                                   # x -> C' P(C x), orthonormal DCT-II folded into the projector
        st in ("l2", "annulus") && return (st == "l2" ? 3 : 4, st == "annulus" ? Float64(c.min) : 0.0, Float64(c.max), nothing, nothing, Int32(0))
        st == "l1" && return (2, 0.0, Float64(c.max), nothing, nothing, Int32(1))
        st == "cardinality" && return (5, 0.0, Float64(c.max), nothing, nothing, Int32(1))
        st == "bounds" && !vecb && return (0, Float64(c.min), Float64(c.max), nothing, nothing, Int32(1))
        st == "bounds" && return (1, 0.0, 0.0, convert(Vector{TF}, c.min), convert(Vector{TF}, c.max), Int32(1))
        error("set type $st behind the DCT is not built in libsipx")
    elseif op == "DFT"
        st == "l1" && return (7, 0.0, Float64(c.max), nothing, nothing, Int32(0))                 # SIPX_PROJ_L1_DFT
        st == "bounds" && vecb && return (12, 0.0, 0.0, nothing, convert(Vector{TF}, c.max), Int32(0))   # SIPX_PROJ_BOUNDS_DFT (mask)
        st in ("l2", "annulus") && return (st == "l2" ? 3 : 4, st == "annulus" ? Float64(c.min) : 0.0, Float64(c.max), nothing, nothing, Int32(0))
        st == "cardinality" && c.app_mode[1] in ("matrix", "tensor") &&
            return (13, 0.0, Float64(convert(Integer, c.max)), nothing, nothing, Int32(0))          # SIPX_PROJ_CARD_DFT
        error("of the DFT-domain sets libsipx builds the l1 ball, cardinality (matrix / tensor mode), masking bounds, the l2 ball and the annulus")
    elseif op == "wavelet"                           # x -> W' P(W x), periodic db4 (SIPX_TRANSFORM_WAVELET = 2)
        st in ("l2", "annulus") && return (st == "l2" ? 3 : 4, st == "annulus" ? Float64(c.min) : 0.0, Float64(c.max), nothing, nothing, Int32(0))
        st == "l1" && return (2, 0.0, Float64(c.max), nothing, nothing, Int32(2))
        st == "cardinality" && return (5, 0.0, Float64(c.max), nothing, nothing, Int32(2))
        st == "bounds" && !vecb && return (0, Float64(c.min), Float64(c.max), nothing, nothing, Int32(2))
        error("set type $st behind the wavelet transform is not built in libsipx")
    elseif op in SPECIAL
        error("operator $op is outside libsipx (JOLI curvelet transform)")
    end
    st == "bounds"      && !vecb && return (0, Float64(c.min), Float64(c.max), nothing, nothing, Int32(0))
    st == "bounds"      && return (1, 0.0, 0.0, convert(Vector{TF}, c.min), convert(Vector{TF}, c.max), Int32(0))
    # l1 / l2 / annulus per fiber or slice with one radius per segment (setup_constraints(...; segment_norms=true)): the vectors travel
    # in lb / ub like per-fiber bounds (include/sipx.h, SIPX_PROJ_L1); a scalar beside a vector is repeated
    if st in ("l1", "l2", "annulus") && c.app_mode[1] in ("fiber", "slice") && (c.max isa AbstractVector || (st == "annulus" && c.min isa AbstractVector))
        nseg = c.max isa AbstractVector ? length(c.max) : length(c.min)
        ub = c.max isa AbstractVector ? convert(Vector{TF}, c.max) : fill(TF(c.max), nseg)
        lb = st != "annulus" ? nothing : (c.min isa AbstractVector ? convert(Vector{TF}, c.min) : fill(TF(c.min), nseg))
        st == "l1" && !all(ub .> 0) && error("Radius of L1 ball is negative")
        return (st == "l1" ? 2 : st == "l2" ? 3 : 4, lb === nothing ? 0.0 : Float64(minimum(lb)), Float64(maximum(ub)), lb, ub, Int32(0))
    end
    # isotropic total variation: the l2,1 ball on the range of the TV operator (include/sipx.h, SIPX_PROJ_L21; not a set of the reference)
    if st == "l21"
        op in ("TV", "D2D", "D3D") && c.custom_TD_OP[1] == [] || error("the l2,1 ball acts on the range of the TV operator: TD_OP must be TV (D2D, D3D)")
        c.app_mode[1] in ("matrix", "tensor") || error("the l2,1 ball applies to the whole array (mode matrix/tensor)")
        c.max > 0 || error("Radius of L1 ball is negative")
        return (14, 0.0, Float64(c.max), nothing_[3:5]...)
    end
    # joint (vectorial) total variation across frames: one group per pixel on the range of TV_xy (include/sipx.h, SIPX_PROJ_L21_JOINT;
    # neither the set nor the operator is the reference's: its setup_constraints cannot build TD_OP = "TV_xy", so this tag reaches
    # libsipx only from a caller that assembles the descriptor list itself, with OPS["TV_xy"])
    if st == "l21_joint"
        op == "TV_xy" && c.custom_TD_OP[1] == [] && c.app_mode[1] in ("matrix", "tensor") ||
            error("the joint l2,1 ball groups the frames of TV_xy: TD_OP must be TV_xy, mode tensor")
        c.max > 0 || error("Radius of L1 ball is negative")
        return (15, 0.0, Float64(c.max), nothing_[3:5]...)
    end
    # total nuclear variation: the nuclear-norm ball on the 2 x n3 Jacobians of the pixels of TV_xy (include/sipx.h, SIPX_PROJ_TNV; as for
    # "l21_joint", the tag reaches libsipx only from a caller that assembles the descriptor list itself, with OPS["TV_xy"]); no weights
    if st == "tnv"
        op == "TV_xy" && c.custom_TD_OP[1] == [] && c.app_mode[1] in ("matrix", "tensor") ||
            error("total nuclear variation couples the frames of TV_xy: TD_OP must be TV_xy, mode tensor, no transform")
        c.max > 0 || error("Radius of L1 ball is negative")
        return (SIPX_PROJ_TNV, 0.0, Float64(c.max), nothing_[3:5]...)
    end
    # group sparsity: the l2,1 ball whose groups are the fibers / slices of the range of a one-block operator (include/sipx.h,
    # SIPX_PROJ_L21_GROUPS; not a set of the reference).  Without weights: the binding does not carry them yet.
    if st == "l21_groups"
        op in ("identity", "D_x", "D_y", "D_z") && c.custom_TD_OP[1] == [] ||
            error("the l2,1 ball over fibers or slices (l21_groups) groups the range of a one-block operator: TD_OP must be the identity, D_x, D_y or D_z (on TV use the l21 sets, whose groups are the grid points)")
        c.app_mode[1] in ("fiber", "slice") ||
            error("the l2,1 ball over fibers or slices (l21_groups) needs a fiber or slice mode: on the whole array it has one group and is the l2 ball -- use the l2 set")
        c.max > 0 || error("Radius of L1 ball is negative")
        return (16, 0.0, Float64(c.max), nothing_[3:5]...)
    end
    st == "l1_weighted" && error("the weighted l1 ball (l1_weighted, SIPX_PROJ_L1_WEIGHTED) needs one weight per row of the operator, which this binding does not carry: use the plain (\"l1\", op), or the C ABI")
    if st == "card_groups"
        op in ("identity", "D_x", "D_y", "D_z") && c.custom_TD_OP[1] == [] ||
            error("group cardinality (card_groups) counts the fibers or slices of the range of a one-block operator: TD_OP must be the identity, D_x, D_y or D_z (on TV or a custom operator use the cardinality set, which counts entries)")
        c.app_mode[1] in ("fiber", "slice") ||
            error("group cardinality (card_groups) needs a fiber or slice mode: on the whole array it has one group, which every k >= 1 keeps -- drop the set, or count entries with the cardinality set")
        (c.max isa Real && isfinite(c.max) && c.max >= 1 && c.max == floor(c.max)) ||
            error("group cardinality (card_groups) needs an integer k >= 1, the number of fibers or slices kept (k = 0 is the zero array: use bounds)")
        return (SIPX_PROJ_CARD_GROUPS, 0.0, Float64(c.max), nothing_[3:5]...)
    end
    # the l2,0 sets on total variation, L0 gradient smoothing: at most k grid points (l20) or pixels in any frame (l20_joint) carry a
    # gradient vector (include/sipx.h, SIPX_PROJ_L20 / SIPX_PROJ_L20_JOINT, csrc/l20.h; not sets of the reference).  max = k, min ignored;
    # per frame -- ("slice", "z") on TV_xy -- max may be a vector of n3 budgets, which travels in ub.  As for "l21_joint", TV_xy reaches
    # libsipx only from a caller that assembles the descriptor list itself.  Set set_Prop.ncvx[i] = true, as for cardinality and rank.
    if st == "l20"
        op in ("TV", "D2D", "D3D", "TV_xy") && c.custom_TD_OP[1] == [] ||
            error("the l2,0 set (l20) counts the gradient vectors of the TV operator: TD_OP must be TV (D2D, D3D) or TV_xy, not a one-block or custom operator (there use the cardinality set, which counts entries, or card_groups)")
        c.app_mode[1] in ("matrix", "tensor") || (op == "TV_xy" && c.app_mode == ("slice", "z")) ||
            error("the l2,0 set (l20) applies to the whole array (matrix / tensor mode), or per frame as (\"slice\", \"z\") on TV_xy: fiber modes and other slices have no gradient groups -- use card_groups on D_x, D_y or D_z there")
        ks = c.max isa AbstractVector ? c.max : [c.max]
        (c.max isa AbstractVector ? c.app_mode[1] == "slice" : true) && all(k -> k isa Real && isfinite(k) && k >= 1 && k == floor(k), ks) ||
            error("the l2,0 set (l20, l20_joint) needs an integer k >= 1, the number of grid points that may carry a gradient (k = 0 is the constant array: use bounds on TV)")
        c.max isa AbstractVector && return (SIPX_PROJ_L20, 0.0, Float64(maximum(ks)), nothing, convert(Vector{TF}, c.max), Int32(0))
        return (SIPX_PROJ_L20, 0.0, Float64(c.max), nothing_[3:5]...)
    end
    if st == "l20_joint"
        op == "TV_xy" && c.custom_TD_OP[1] == [] && c.app_mode[1] in ("matrix", "tensor") ||
            error("the joint l2,0 set (l20_joint) needs the TV_xy operator of a 3-D grid in tensor mode: its groups span the frames -- for one budget over all grid points use (\"l20\", \"TV_xy\"), per frame (\"l20\", \"TV_xy\", (\"slice\", \"z\"))")
        (c.max isa Real && isfinite(c.max) && c.max >= 1 && c.max == floor(c.max)) ||
            error("the l2,0 set (l20, l20_joint) needs an integer k >= 1, the number of grid points that may carry a gradient (k = 0 is the constant array: use bounds on TV)")
        return (SIPX_PROJ_L20_JOINT, 0.0, Float64(c.max), nothing_[3:5]...)
    end
    if st == "l21_stacked"
        c.custom_TD_OP[1] == [] && error("the stacked l2,1 ball (l21_stacked) groups the rows of a caller-supplied sparse operator across its blocks: the operator must be SIPX_OP_CSC (custom_TD_OP, or the named \"Hessian\") -- on the built-in TV operator the set is (\"l21\", \"TV\")")
        c.app_mode[1] in ("matrix", "tensor") ||
            error("the stacked l2,1 ball (l21_stacked) applies to the whole array (matrix / tensor mode): its groups are the rows p, G + p, 2 G + p, ... of the operator, fibers and slices have no meaning there")
        (c.min isa Real && c.min == floor(c.min) && 1 <= c.min <= 8) ||
            error("the stacked l2,1 ball (l21_stacked): blocks = $(c.min), the number of equal-sized blocks of the operator must be 1 .. 8")
        size(c.custom_TD_OP[1], 1) % Int(c.min) == 0 ||
            error("the stacked l2,1 ball (l21_stacked): the operator has M = $(size(c.custom_TD_OP[1], 1)) rows, not a multiple of blocks = $(Int(c.min)) -- every block needs the same number of rows (pad a shorter block with zero rows)")
        c.max > 0 || error("Radius of L1 ball is negative")
        return (SIPX_PROJ_L21_STACKED, 0.0, Float64(c.max), nothing_[3:5]...)
    end
    if st == "l2inf" || st == "l2inf_joint"
        joint = st == "l2inf_joint"
        c.custom_TD_OP[1] == [] && (joint ? op == "TV_xy" : op in ("TV", "D2D", "D3D", "TV_xy")) ||
            error(joint ? "the joint l2,inf ball (l2inf_joint) groups the frames of TV_xy: TD_OP must be TV_xy, mode tensor -- per frame bounds are (\"l2inf\", \"TV_xy\")" :
                          "the l2,inf ball (l2inf) bounds the gradient magnitude at every grid point: TD_OP must be TV (D2D, D3D), TV_xy or the named \"Hessian\" -- a bound on one difference direction is (\"bounds\", \"D_z\"), a caller-supplied stacked operator takes (\"l2inf_stacked\", name, 0, c, mode, custom_TD_OP=(A, False), blocks=B)")
        c.app_mode[1] in ("matrix", "tensor") ||
            error("the l2,inf ball (l2inf, l2inf_joint, l2inf_stacked) applies to the whole array (matrix / tensor mode), fibers and slices are not built: (\"slice\", \"z\") on TV_xy is the vector form with c constant within every frame -- pass max = np.repeat(c_frames, n1 * n2)")
        (c.min isa Real && c.min == 0) ||
            error("the l2,inf ball (l2inf, l2inf_joint, l2inf_stacked) bounds the group norms from above only: min must be 0 -- a lower bound on the gradient magnitude is not convex and not built")
        kind = joint ? SIPX_PROJ_L2INF_JOINT : SIPX_PROJ_L2INF
        c.max isa AbstractVector && return (kind, 0.0, 1.0, nothing, convert(Vector{TF}, c.max), Int32(0))      # (checked by libsipx: length, entries >= 0)
        c.max > 0 || error("the l2,inf ball (l2inf, l2inf_joint, l2inf_stacked) needs a bound c > 0 as a scalar (c = 0 is the constant array: use bounds on TV, or a vector of zeros to flatten chosen points)")
        return (kind, 0.0, Float64(c.max), nothing_[3:5]...)
    end
    st == "l2inf_stacked" && error("the stacked l2,inf ball (l2inf_stacked, SIPX_PROJ_L2INF_STACKED) is not built in this binding: the reference's set_definitions has no field for the number of blocks and min must stay 0 -- use the C ABI or the Python front end")
    st == "simplex" && error("simplex sets (simplex, SIPX_PROJ_SIMPLEX) are not built in this binding yet: use (\"bounds\") together with (\"l1\", op, mode) and segment_norms=true, or the C ABI")
    st == "l1"          && return (2, 0.0, Float64(c.max), nothing_[3:5]...)
    st == "l2"          && return (3, 0.0, Float64(c.max), nothing_[3:5]...)
    st == "annulus"     && return (4, Float64(c.min), Float64(c.max), nothing_[3:5]...)
    st == "cardinality" && return (5, 0.0, Float64(convert(Integer, c.max)), nothing_[3:5]...)
    st == "prox_l1"     && return (6, 0.0, Float64(c.max), nothing_[3:5]...)
    st == "rank"        && return (8, 0.0, Float64(convert(Integer, c.max)), nothing_[3:5]...)
    st == "nuclear"     && return (9, 0.0, Float64(c.max), nothing_[3:5]...)
    st == "histogram"   && return (10, 0.0, 0.0, convert(Vector{TF}, c.min), convert(Vector{TF}, c.max), Int32(0))
    st == "subspace"    && return (11, 0.0, 0.0, nothing, nothing, Int32(0))
    error("set type $st is not part of libsipx")
end

"""
    setup_constraints(constraint, comp_grid, TF; segment_norms=false) -> (P_sub, TD_OP, set_Prop)

The reference's `setup_constraints` (src/setup_constraints.jl:17-102).  With `segment_norms=true` it also takes l1, l2 and annulus
sets with `app_mode = ("fiber", d)` or `("slice", d)` on the identity, D_x, D_y or D_z: libsipx projects every fiber / slice of the
array of shape TD_n on its own, all with the scalar min / max, or each with its own: `max` (for the annulus `min` and / or `max`) a
vector of nseg entries in the segment order of include/sipx.h (SIPX_PROJ_L1), a scalar beside a vector repeated.  The reference has no such
projector ("l1 and l2 constraints only available for matrix or tensor mode, currently"): without the keyword its error stays.
The reference sets the operators and properties up for the whole-array form of such a set; the application mode is put back
into the constraint its P_sub[i] captured -- where `PARSDMM` above reads it -- and into set_Prop.tag[i].  Such a P_sub[i] must
not be called as a Julia function: it would project the whole array.

`("l21", "TV")` in matrix / tensor mode -- isotropic total variation, the l2,1 ball of radius `max` on the TV range (include/sipx.h,
SIPX_PROJ_L21) -- is libsipx's own as well and needs no keyword.  The reference sets such a set up as the anisotropic `("l1", "TV")`
(same operator, same properties); the set type is put back into the captured constraint and the tag.  Its P_sub[i] must not be
called as a Julia function either: it would project onto the l1 ball.
"""
function setup_constraints(constraint, comp_grid, TF; segment_norms::Bool=false)
    iso = [i for (i, c) in enumerate(constraint) if c.set_type == "l21"]
    for i in iso
        projector_fields(constraint[i], TF)                 # the refusals
        constraint[i].set_type = "l1"
    end
    out = try
        setup_constraints_segments(constraint, comp_grid, TF, segment_norms)
    finally
        for i in iso
            constraint[i].set_type = "l21"
        end
    end
    for i in iso
        t = out[3].tag[i]
        out[3].tag[i] = ("l21", t[2], t[3], t[4])
    end
    return out
end

function setup_constraints_segments(constraint, comp_grid, TF, segment_norms::Bool)
    ref = getfield(parentmodule(log_type_PARSDMM), :setup_constraints)
    segment_norms || return ref(constraint, comp_grid, TF)
    ndim = (length(comp_grid.n) == 3 && comp_grid.n[3] > 1) ? 3 : 2
    modes = Dict{Int,Any}()
    for (i, c) in enumerate(constraint)
        (c.set_type in ("l1", "l2", "annulus") && c.app_mode[1] in ("fiber", "slice")) || continue
        c.TD_OP in ("identity", "D_x", "D_y", "D_z") && c.custom_TD_OP[1] == [] ||
            error("fiber / slice modes need an operator with one block (identity, D_x, D_y, D_z)")
        ndim == 2 && c.app_mode[1] == "slice" &&
            error("for 2D models, the mode of application for $(c.set_type) sets needs to be (fiber,x) or (fiber,z), or matrix for the whole array")
        modes[i] = (c.app_mode, c.min, c.max)
        c.app_mode = (ndim == 3 ? "tensor" : "matrix", "")
        c.max isa AbstractVector && (c.max = maximum(c.max))      # the reference sets the whole-array form up with scalars
        c.min isa AbstractVector && (c.min = minimum(c.min))
    end
    (P_sub, TD_OP, set_Prop) = ref(constraint, comp_grid, TF)
    for (i, (am, mn, mx)) in modes
        constraint[i].app_mode = am
        constraint[i].min = mn isa AbstractVector ? convert(Vector{TF}, mn) : constraint[i].min
        constraint[i].max = mx isa AbstractVector ? convert(Vector{TF}, mx) : constraint[i].max
        set_Prop.tag[i] = (set_Prop.tag[i][1], set_Prop.tag[i][2], am[1], am[2])
    end
    return P_sub, TD_OP, set_Prop
end

"log.timing with the reference's seven section names, filled from the engine's accumulators (milliseconds)"
function timer_from_sections(ms::NTuple{7,Float64}, ncalls::NTuple{7,Int})
    to = TimerOutput()
    for (k, name) in enumerate(SECTIONS)
        # TimerOutputs 0.5.x (the reference's compat bound): a section is a child TimerOutput whose accumulated_data holds
        # (ncalls, time in ns, allocated bytes)
        @timeit to name nothing
        td = to.inner_timers[name].accumulated_data
        td.ncalls = ncalls[k]
        td.time   = round(Int64, ms[k] * 1e6)
        td.allocs = 0
    end
    return to
end

# ---- options.parallel = true: one process per GPU, RCCL inside the engine (include/sipx.h, "sharded solve") ----------------
# Launch (one node, 8 GPUs), every process running the SAME script:
#     for r in 0:7:  SIPX_RANK=r SIPX_WORLD=8 SIPX_DEVICE=r SIPX_ID_FILE=/dev/shm/sipx.$JOB SIPX_NONCE=$JOB julia --project script.jl &
# (or under mpiexec with SIPX_RANK / SIPX_WORLD taken from the MPI environment).  Rank 0 obtains the 128-byte ncclUniqueId
# from the engine and publishes it through SIPX_ID_FILE; the others wait for the file.  SIPX_DECOMP=slab (default where the
# set list allows it: bounds / l1 / l2 / annulus on the identity or D_x / D_y / D_z / TV) divides the WHOLE iteration by
# z-slab; SIPX_DECOMP=sets is the reference's own split by constraint set.  SIPX_DECOMP=slab may also be ASKED for with the
# other set lists (round 5: slice-wise rank / nuclear norm on z-slices, cardinality, the l1 ball behind the DFT run inside the slab
# iteration, any other projector through an owner rank; sipx.h, sipx_set_decomp).  Every rank returns the same x and log;
# with the set decomposition l[i], y[i] are filled on the rank that owns set i only.
localize(v) = (isdefined(Main, :DistributedArrays) && v isa Main.DistributedArrays.DArray) ? convert(Vector, v) : v

function slab_decomposable(set_Prop)
    for t in set_Prop.tag                       # (set_type, TD_OP, app_mode[1], app_mode[2])
        (t[1] in ("bounds", "l1", "l2", "annulus", "prox_l1") && t[2] in ("identity", "D_x", "D_y", "D_z", "TV", "D2D", "D3D") &&
         t[3] in ("matrix", "tensor")) || return false
    end
    return true
end

function attach_comm!(ctx, set_Prop)
    world = parse(Int, ENV["SIPX_WORLD"]); rank = parse(Int, ENV["SIPX_RANK"])
    idfile = ENV["SIPX_ID_FILE"]
    id = zeros(UInt8, 128)
    # The id file must belong to THIS launch: a rerun with the same path would otherwise hand the previous job's ncclUniqueId to
    # ranks that find the stale file before rank 0 has replaced it (ncclCommInitRank then hangs).  Every record starts with a
    # nonce the launcher gives all ranks (SIPX_NONCE; without one, a record older than two minutes is taken to be stale).
    nonce = rpad(get(ENV, "SIPX_NONCE", ""), 32)[1:32]
    if rank == 0
        rm(idfile; force=true)
        check(ccall((:sipx_rccl_unique_id, libsipx), Cint, (Ptr{UInt8},), id))
        write(idfile * ".tmp", vcat(Vector{UInt8}(nonce), id)); mv(idfile * ".tmp", idfile; force=true)   # published atomically
    else
        t_start = time()
        while true
            if isfile(idfile) && filesize(idfile) == 160
                rec = read(idfile)
                fresh = haskey(ENV, "SIPX_NONCE") ? true : (mtime(idfile) >= t_start - 120.0)
                if String(rec[1:32]) == nonce && fresh
                    id = rec[33:160]
                    break
                end
            end
            time() - t_start > 600.0 && error("sipx: no ncclUniqueId for this launch appeared in $idfile within 10 minutes")
            sleep(0.01)
        end
    end
    check(ccall((:sipx_set_comm_rccl, libsipx), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Cint, Cint), ctx[], id, world, rank))
    rank == 0 && rm(idfile; force=true)       # ncclCommInitRank is collective: every rank has read the record by now
    decomp = get(ENV, "SIPX_DECOMP", slab_decomposable(set_Prop) ? "slab" : "sets")
    decomp == "slab" && check(ccall((:sipx_set_decomp, libsipx), Cint, (Ptr{Cvoid}, Cint), ctx[], 1))
    # what RCCL itself reports (ncclCommCount / ncclCommUserRank / ncclGetVersion): worth one line in the job log
    nr = Ref{Cint}(0); rk = Ref{Cint}(0); dc = Ref{Cint}(0); ver = zeros(UInt8, 64)
    check(ccall((:sipx_comm_info, libsipx), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Cint}, Ptr{UInt8}, Cint, Ref{Cint}), ctx[], nr, rk, ver, 64, dc))
    rank == 0 && @info "sipx: sharded solve" ranks=nr[] version=unsafe_string(pointer(ver)) decomposition=(dc[] == 1 ? "slab" : "sets")
    nr[] == world || error("RCCL sees $(nr[]) ranks, SIPX_WORLD says $world")
    return nothing
end

# ---- contexts kept between calls (round 5) ----
# The reference's callers wrap PARSDMM as a projector and call it again and again with the SAME AtA / TD_OP / set_Prop / P_sub
# objects (examples/constrained_freq_FWI_simple.jl:468, examples/Constraint_examples_2D.jl:222-223): a call whose arguments are
# those very objects (objectid), on the same grid and precision, finds the device context of the previous call and resets it
# (sipx_reset: no allocation, no plan, no handle) instead of building one.  SIPX_CONTEXT_CACHE=0 switches this off; at most
# SIPX_CONTEXT_CACHE (default 2) contexts are kept, the oldest goes first; release_contexts() frees them (also at exit).
# A caller that mutates AtA / P_sub IN PLACE between calls must call release_contexts() itself -- the arrays were copied to the
# device when the context was built.  Sharded solves (options.parallel) are not cached.
const CONTEXTS = Vector{Pair{Any,Ptr{Cvoid}}}()

function release_contexts()
    for (_, c) in CONTEXTS
        ccall((:sipx_destroy, libsipx), Cvoid, (Ptr{Cvoid},), c)
    end
    empty!(CONTEXTS)
    return nothing
end
atexit(release_contexts)

cache_limit() = something(tryparse(Int, get(ENV, "SIPX_CONTEXT_CACHE", "2")), 2)

function PARSDMM(m         ::Vector{TF},
                 AtA,
                 TD_OP,
                 set_Prop,
                 P_sub,
                 comp_grid,
                 options,
                 x=zeros(TF,length(m)) ::Vector{TF},
                 l=[],
                 y=[]
                 ) where {TF<:Real}
    t_init = time_ns()
    TF in (Float32, Float64) || error("libsipx computes in Float32 or Float64")
    convert_options!(options, TF)                                           # src/PARSDMM.jl:43
    if isreal(m) == false || isreal(x) == false || isreal(l) == false || isreal(y) == false
        error("input for PARSDMM is not real")                              # src/PARSDMM.jl:50-52
    end
    # options.parallel = true (src/PARSDMM.jl:114-131: DArray TD_OP / P_sub, one Julia worker per set): here the solve is
    # sharded over PROCESSES, one per GPU -- every process calls this same method with the same arguments (see
    # attach_comm! below and INTEGRATION.md, section 5); distributed inputs are gathered, every rank builds every set.
    if options.parallel
        TD_OP = localize(TD_OP); P_sub = localize(P_sub); AtA = localize(AtA)
        isempty(l) || (l = localize(l)); isempty(y) || (y = localize(y))
    end
    p  = length(TD_OP)
    pp = options.feasibility_only ? p : p - 1                               # src/PARSDMM.jl:55-56
    length(P_sub) == pp || error("P_sub must hold one projector per constraint set")
    n    = collect(Int64, comp_grid.n)
    h    = collect(Float64, comp_grid.d)
    ndim = length(n)
    N    = prod(n)

    device = parse(Int, get(ENV, "SIPX_DEVICE", get(ENV, "SIPX_RANK", "0")))
    key    = (TF, Tuple(n), Tuple(h), device, Bool(options.feasibility_only), objectid(AtA), objectid(TD_OP), objectid(set_Prop), objectid(P_sub),
              Tuple(sort!([k => v for (k, v) in ENV if startswith(k, "SIPX_")])))
    cached = (!options.parallel && cache_limit() > 0) ? findfirst(e -> isequal(first(e), key), CONTEXTS) : nothing
    ctx = Ref{Ptr{Cvoid}}(C_NULL)
    reused = cached !== nothing
    if reused
        ctx[] = last(CONTEXTS[cached])
        deleteat!(CONTEXTS, cached)                                         # (back in at the end of a call that succeeded)
    else
        check(ccall((:sipx_create, libsipx), Cint, (Ref{Ptr{Cvoid}}, Cint, Cint, Ptr{Int64}, Ptr{Float64}, Cint),
                    ctx, TF == Float32 ? 0 : 1, ndim, n, h, device))
    end
    keep = Any[]                                                            # arrays the descriptors point at, until finalize
    done = false
    try
        for i in (reused ? (1:0) : (1:pp))
            c   = getfield(P_sub[i], :constraint)                            # captured by every branch of get_projector
            tag = set_Prop.tag[i]                                            # (set_type, TD_OP, app_mode[1], app_mode[2])
            (tag[1] == c.set_type && tag[2] == c.TD_OP) || error("set_Prop.tag[$i] does not describe P_sub[$i]")
            (kind, pmin, pmax, lb, ub, transform) = projector_fields(c, TF)
            custom = c.set_type != "subspace" && !(c.custom_TD_OP[1] == [])   # src/setup_constraints.jl:70-72
            opcode = custom ? 5 : (c.TD_OP in SPECIAL ? 0 : OPS[c.TD_OP])    # orthogonal transforms: TD_OP[i] = I (:76-80)
            basis  = c.set_type == "subspace" ? convert(Matrix{TF}, c.custom_TD_OP[1]) : nothing
            colptr = rowval = nzval = nothing
            rows   = 0
            if custom
                A      = c.custom_TD_OP[1]::SparseMatrixCSC
                colptr = convert(Vector{Int64}, A.colptr) .- 1               # 0-based copies
                rowval = convert(Vector{Int64}, A.rowval) .- 1
                nzval  = convert(Vector{TF}, A.nzval)
                rows   = size(A, 1)
            end
            push!(keep, (lb, ub, basis, colptr, rowval, nzval))
            d = SipxSetDesc(opcode, kind, pmin, pmax,
                            lb === nothing ? C_NULL : pointer(lb), ub === nothing ? C_NULL : pointer(ub),
                            set_Prop.ncvx[i] ? 1 : 0,
                            (kind in (SIPX_PROJ_L2INF, SIPX_PROJ_L2INF_JOINT) && ub !== nothing) ? Int32(length(ub)) : Int32(0),   # reserved: the entries of an l2inf ub
                            MODE[c.app_mode[1]], dir_of(c.app_mode[2], ndim),
                            basis === nothing ? C_NULL : pointer(basis), basis === nothing ? 0 : size(basis, 1),
                            basis === nothing ? 0 : size(basis, 2), basis === nothing ? 0 : Int32(c.custom_TD_OP[2]),
                            0,                                                # Minkowski component (see INTEGRATION.md)
                            colptr === nothing ? C_NULL : pointer(colptr), rowval === nothing ? C_NULL : pointer(rowval),
                            nzval === nothing ? C_NULL : pointer(nzval), rows,
                            transform, 0,
                            kind == SIPX_PROJ_L21_STACKED ? Int32(c.min) : Int32(0), 0)
            # AtA[i] in CDS (N x d_i) with its offsets.  A custom sparse TD_OP of a set that is not banded
            # (set_Prop.banded[i] == false: the reference keeps its AtA sparse, PARSDMM_precompute_distribute.jl:51-59) goes
            # without AtA: libsipx applies it as a matrix-free term of Q.  JOLI / dense AtA stay outside libsipx.
            if custom && !set_Prop.banded[i]
                rc = GC.@preserve keep ccall((:sipx_add_set, libsipx), Cint,
                            (Ptr{Cvoid}, Ref{SipxSetDesc}, Ptr{Cvoid}, Ptr{Int64}, Cint),
                            ctx[], d, C_NULL, C_NULL, 0)
            else
                AtA[i] isa Matrix{TF} || error("libsipx needs the AtA of a banded set in CDS storage")
                off = convert(Vector{Int64}, set_Prop.AtA_offsets[i])
                rc = GC.@preserve keep off ccall((:sipx_add_set, libsipx), Cint,
                            (Ptr{Cvoid}, Ref{SipxSetDesc}, Ptr{Cvoid}, Ptr{Int64}, Cint),
                            ctx[], d, AtA[i], off, size(AtA[i], 2))
            end
            rc < 0 && check(1)                                               # sipx_add_set returns the set index, -1 on error
        end

        options.parallel && !reused && attach_comm!(ctx, set_Prop)           # before sipx_finalize: this context is one RANK

        # l, y as PARSDMM_initialize allocates them (src/PARSDMM_initialize.jl:120-127)
        if isempty(l); l = Vector{Vector{TF}}(undef, p); for i in 1:p; l[i] = zeros(TF, size(TD_OP[i], 1)); end; end
        if isempty(y); y = Vector{Vector{TF}}(undef, p); for i in 1:p; y[i] = zeros(TF, size(TD_OP[i], 1)); end; end
        rho_ini = convert(Vector{Float64}, options.rho_ini)
        feas0   = zeros(Float64, max(pp, 1))
        lp = Ptr{Cvoid}[pointer(v) for v in l]; yp = Ptr{Cvoid}[pointer(v) for v in y]
        if reused                                                            # the same sets once more: src/PARSDMM.jl:58-61 without its allocations
            GC.@preserve l y check(ccall((:sipx_reset, libsipx), Cint,
                  (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Cint, Float64, Cint, Ptr{Cvoid}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Float64}),
                  ctx[], m, rho_ini, length(rho_ini), Float64(options.gamma_ini), options.zero_ini_guess, x, lp, yp, feas0))
        else
            GC.@preserve keep l y check(ccall((:sipx_finalize, libsipx), Cint,
                  (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float64}, Cint, Float64, Cint, Cint, Ptr{Cvoid}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Float64}),
                  ctx[], m, rho_ini, length(rho_ini), Float64(options.gamma_ini), options.feasibility_only, options.zero_ini_guess,
                  x, lp, yp, feas0))
        end
        empty!(keep)
        ms_init = (time_ns() - t_init) * 1e-6

        # ---- the main loop, natively (src/PARSDMM.jl:97-257) ----
        maxit = Int(options.maxit)
        sf = zeros(Float64, pp, maxit); rd = zeros(Float64, p, maxit); rpm = zeros(Float64, p, maxit)     # row-major [maxit][.]
        rdt = zeros(Float64, maxit); rpt = zeros(Float64, maxit); obj = zeros(Float64, maxit); evo = zeros(Float64, maxit)
        rho = zeros(Float64, p, maxit); gam = zeros(Float64, p, maxit); cgi = zeros(Int64, maxit); cgr = zeros(Float64, maxit)
        o   = SipxOptions(maxit, Float64(options.evol_rel_tol), Float64(options.feas_tol), Float64(options.obj_tol),
                          Int32(options.rho_update_frequency), options.adjust_rho, options.adjust_gamma,
                          options.adjust_feasibility_rho)
        lg  = SipxLog(pointer(sf), pointer(rd), pointer(rpm), pointer(rdt), pointer(rpt), pointer(obj), pointer(evo),
                      pointer(rho), pointer(gam), pointer(cgi), pointer(cgr), ntuple(_ -> 0.0, 7), 0, 0, 0)
        GC.@preserve sf rd rpm rdt rpt obj evo rho gam cgi cgr check(ccall((:sipx_parsdmm, libsipx), Cint,
              (Ptr{Cvoid}, Ref{SipxOptions}, Ref{SipxLog}), ctx[], o, lg))

        it, nf = Int(lg.n_iter), Int(lg.n_feas_rows)
        if lg.stopped_feasible != 0                                          # feasible input: x = m, one log row (src/PARSDMM.jl:63-82)
            copy!(x, m)
        else
            GC.@preserve l y check(ccall((:sipx_download, libsipx), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}),
                                        ctx[], x, lp, yp))
        end
        # log_type_PARSDMM (src/SetIntersectionProjection.jl:95-108), truncated like output_check_PARSDMM (src/PARSDMM.jl:261-278);
        # the C arrays are row-major [row][column] = column-major (column, row) here, hence the transposes
        ms = ntuple(k -> k == 1 ? ms_init : lg.timing_ms[k], 7)
        nc = ntuple(k -> k == 1 ? 1 : it, 7)
        log_PARSDMM = log_type_PARSDMM(permutedims(sf[:, 1:nf]), permutedims(rd[:, 1:it]), permutedims(rpm[:, 1:it]),
                                       rdt[1:it], rpt[1:it], obj[1:it], evo[1:it],
                                       permutedims(rho[:, 1:it]), permutedims(gam[:, 1:it]), cgi[1:it], cgr[1:it],
                                       timer_from_sections(ms, nc))
        done = true
        return x, log_PARSDMM, l, y
    finally
        if done && !options.parallel && cache_limit() > 0                    # keep the context for the next call with these objects
            while length(CONTEXTS) >= cache_limit()
                ccall((:sipx_destroy, libsipx), Cvoid, (Ptr{Cvoid},), last(popfirst!(CONTEXTS)))
            end
            push!(CONTEXTS, key => ctx[])
        else
            ccall((:sipx_destroy, libsipx), Cvoid, (Ptr{Cvoid},), ctx[])
        end
    end
end

# ---- alternative: keep the reference's own loop (its @timeit sections, stop_PARSDMM, logging) and replace each phase ----
# Inside `for i=1:maxit` of src/PARSDMM.jl, with ctx from sipx_create / sipx_add_set / sipx_finalize as above:
#   :101  rhs_compose(...)            ->  ccall((:sipx_rhs_compose, libsipx), Cint, (Ptr{Cvoid}, Ptr{Float64}), ctx[], rho64)
#   :106-107 copy!(x_old,x); argmin_x ->  ccall((:sipx_argmin_x, libsipx), Cint, (Ptr{Cvoid}, Cint, Ref{Float64}, Ref{Int64}, Ref{Float64}, Ref{Cint}),
#                                               ctx[], i, tol_ref, cg_it, relres, flag)
#   :133  update_y_l(...)             ->  ccall((:sipx_update_y_l, libsipx), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
#                                               ctx[], i, flags, rho64, gamma64, r_pri, r_dual, feas)
#         flags = (mod(i,10)==0 ? 1 : 0) | (((adjust_rho || adjust_gamma) && mod(i,rho_update_frequency)==0) ? 2 : 0) | (i==1 ? 4 : 0)
#   :140,145 obj, evol_x              ->  ccall((:sipx_log_scalars, libsipx), Cint, (Ptr{Cvoid}, Ref{Float64}, Ref{Float64}), ctx[], obj_i, evol_i)
#   :153  stop_PARSDMM(...)               unchanged Julia
#   :164-206 l_hat, snapshots, adapt  ->  (fused into sipx_update_y_l by flags 2 / 4) then
#                                         ccall((:sipx_adapt_rho_gamma, libsipx), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{Float64}, Ptr{Float64}), ctx[], adjust_rho, adjust_gamma, rho64, gamma64)
#   :213-226 feasibility doubling, clamp  unchanged Julia
#   :230-243 Q_update! + prox rebind  ->  ccall((:sipx_q_update, libsipx), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), ctx[], rho64, Float64.(log_PARSDMM.rho[i,:]))
# tests/c_abi/phases.c runs exactly this sequence from C and checks it against sipx_parsdmm bit for bit.

# ---- constraint learning (src/constraint_learning_by_observation.jl:8-163) on the device ---------------------------------
const LEARN_KEYS = ("nuclear_norm", "nuclear_Dx", "nuclear_Dz", "rank_095", "TV", "wavelet_l1", "Dx_l1", "Dz_l1", "DFT_l1",
                    "DFT_card_095", "TV_card_095", "annulus", "TV_annulus", "D_l2", "D_x_min", "D_x_max", "D_z_min", "D_z_max",
                    "DCT_x_LB", "DCT_x_UB", "DCT_y_LB", "DCT_y_UB", "hist_min", "hist_max", "hist_TV_min", "hist_TV_max")

"""The reference's dictionary for m_train[i,:,:] on a 2-D grid (sipx_learn_observations): Julia's own strides are passed, the
*_min / *_LB arrays are Float64 (as the reference's `zeros(TF,n) .+ 1e8` makes them), counts are Int32 (Float32) or Int64."""
function constraint_learning_by_obseration(comp_grid, m_train::Array{TF}; max_batch::Integer=0, device::Integer=0) where {TF<:Union{Float32,Float64}}
    m = ndims(m_train) == 2 ? reshape(m_train, 1, size(m_train)...) : m_train
    ndims(m) == 3 || error("constraint learning: m_train must be n_train x n1 x n2")
    (nt, n1, n2) = size(m)
    TI = TF == Float64 ? Int64 : Int32
    N, M = n1 * n2, (n1 - 1) * n2 + n1 * (n2 - 1)
    len = Dict("DCT_x_LB" => n1, "DCT_x_UB" => n1, "DCT_y_LB" => n2, "DCT_y_UB" => n2, "hist_min" => N, "hist_max" => N,
               "hist_TV_min" => M, "hist_TV_max" => M)
    typ(k) = k in ("rank_095", "DFT_card_095", "TV_card_095") ? TI : (k in ("DCT_x_LB", "DCT_y_LB", "hist_min", "hist_TV_min") ? Float64 : TF)
    out = Dict{String,Any}(k => zeros(typ(k), get(len, k, nt)) for k in LEARN_KEYS)
    ptrs = Ptr{Cvoid}[pointer(out[k]) for k in LEARN_KEYS]
    n = Int64[n1, n2]
    h = Float64[comp_grid.d[1], comp_grid.d[2]]
    st = Int64[strides(m)...]
    GC.@preserve out ptrs m check(ccall((:sipx_learn_observations, libsipx), Cint,
        (Cint, Ptr{Int64}, Ptr{Float64}, Int64, Ptr{Cvoid}, Ptr{Int64}, Int64, Ptr{Ptr{Cvoid}}, Cint),
        TF == Float64 ? 1 : 0, n, h, nt, m, st, max_batch, ptrs, device))
    return out
end

end # module
