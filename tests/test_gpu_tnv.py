"""Total nuclear variation on the GPU: the ("tnv", "TV_xy") set (csrc/tnv.h, csrc/ext_group.hip, TnvProj) against tests/tnv_ref.py: the
projector at three radii, inputs it must not write, exact integer cases, rank-1 stacks against the joint l2,1 ball, observed radii
(sipx.tnv_norm), whole solves against the oracle on the same operator given as custom_TD_OP with its projector swapped for the reference,
and the refusals through the C ABI and host.py.

GRIDS and the path each takes (l21_joint_plan cuts the n3 frames into min(ceil(131072 / (L sizeof(T) / 16)), n3 / 8) chunks, L = n1 n2;
the Gram / apply kernels take 16 bytes per thread when n1 % 4 == 0 and launch min(ceil(items / 256), 2048) workgroups):
  (4, 3, 2), (5, 4, 3)   every boundary class; 16 bytes on (4, 3, 2), one pixel per thread on (5, 4, 3); one chunk
  (33, 20, 3)            odd n1, one pixel per thread, 660 pixels: more than one workgroup; one chunk
  (32, 12, 8)            16-byte path; n3 = 8 < 16: one chunk, two full batches of 4 frames
  (8, 4, 67)             8 chunks of 9 frames, the last one ragged with 4 frames; 16 bytes; k_tnv_finish runs
  (4, 3, 15), (4, 3, 16) the two sides of the chunk boundary: one chunk of 15 frames, two chunks of 8
  (1021, 515, 2)         odd n1, 525 815 pixels > 2048 * 256: a second sweep of the Gram kernel, one pixel per thread
  (1024, 1028, 2)        2 105 344 points > 2048 * 256 * 4: a second, partial sweep of the apply kernel on the 16-byte path
tests/test_tnv_cpu.py asserts these claims from the plan.
(4, 3, 1) is not a grid the set can be built on: a grid with n3 = 1 is a 2-D grid, which the TV_xy operator refuses with its own text
(include/sipx.h, SIPX_OP_TV_XY); test_refusals holds the set to that text, and a search of 2 n1 n2 entries never outgrows the N entries of
scratch.  The rank-1 case "n3 = 1" is run as a stack with one non-zero frame.

INPUT.  make_input of tests/test_gpu_l21_frames.py, then planted: every 7th pixel's D_x row = 0.7 x its D_y row + 1e-4 (Float64: 1e-9) x
itself, every 11th pixel exact rank 1 (D_x row = -0.5 x D_y row), every 13th pixel all zero.
BOUND.  tnv_ref.BOUND, in eps ||J_p||_F over the members of pixel p.  Worst observed on an MI355X: see DESIGN.md section 7i."""
import ctypes as C

import numpy as np
import pytest
import torch      # (before libsipx.so is loaded: one HIP runtime in the process)

from oracle import parsdmm_oracle as O
from tests import l1_exact, l21_frames_ref as RF, l21_joint_ref as RJ, tnv_ref as R
from tests.test_gpu_l21_frames import _in_place, _julia_max, _model, _stacked, make_input

pytestmark = pytest.mark.gpu

GRIDS = [(4, 3, 2), (5, 4, 3), (33, 20, 3), (32, 12, 8), (8, 4, 67), (4, 3, 15), (4, 3, 16), (1021, 515, 2), (1024, 1028, 2)]
CHUNKED = [(8, 4, 67), (4, 3, 16)]
OBSERVE_GRIDS = [(33, 20, 3), (4, 3, 15)] + CHUNKED
FRACS = [0.9, 0.5, 0.05]
PRECISIONS = [np.float32, np.float64]
_inputs, _refs = {}, {}


def _grid(sipx, n):
    return sipx.compgrid(tuple(1.0 for _ in n), n)


def _P(sipx, n, TF, tau, st="tnv"):
    return sipx.Projector(sipx.set_definitions(st, "TV_xy", 0.0, float(tau), ("tensor", "")), _grid(sipx, n), TF)


def planted_input(n, TF):
    """The input of the docstring, as a new array."""
    v, _ = make_input(n, TF)
    G = RJ._members(n)
    both = (G >= 0).all(axis=(1, 2))
    p = np.arange(G.shape[0])
    near = both & (p % 7 == 0)
    v[G[near, :, 1]] = (TF(0.7) * v[G[near, :, 0]] + TF(1e-4 if TF == np.float32 else 1e-9) * v[G[near, :, 1]]).astype(TF)
    one = both & (p % 11 == 0)
    v[G[one, :, 1]] = TF(-0.5) * v[G[one, :, 0]]
    zero = G[p % 13 == 0]
    v[zero[zero >= 0]] = 0
    return v


def _input(n, TF):
    """(v, its nuclear variation, tnv_ref.prepare(v)): computed once, v handed out as a copy."""
    key = (n, np.dtype(TF).name)
    if key not in _inputs:
        v = planted_input(n, TF)
        pre = R.prepare(v, n)
        _inputs[key] = (v, float(np.sum(pre[1][0]) + np.sum(pre[1][1])), pre)
    v, nrm, pre = _inputs[key]
    return v.copy(), nrm, pre


def _reference(n, TF, frac):
    key = (n, np.dtype(TF).name, frac)
    if key not in _refs:
        v, nrm, pre = _input(n, TF)
        tau = TF(frac * nrm)
        ref = R.project(v, n, tau, pre)
        ref.setflags(write=False)
        _refs[key] = (tau, ref, R.inside(v, n, tau, pre))
    return _refs[key]


def _check(v, y, ref, n, TF, tag):
    eps = float(np.finfo(TF).eps)
    worst = float(R.error(y, ref, v, n).max()) / eps
    print(f"tnv {tag} {n} {np.dtype(TF).name}: worst error {worst:.3f} eps |J_p|_F (bound {R.BOUND[TF]})")
    assert worst <= R.BOUND[TF], f"worst error {worst:.3f} eps |J_p|_F"
    return worst


# ---- 1. the projector against the reference; two calls give the same bits ---------------------------------------------------------------------
@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("frac", FRACS)
@pytest.mark.parametrize("n", GRIDS)
def test_projector_matches_the_reference(sipx, TF, frac, n):
    v, nrm, _ = _input(n, TF)
    tau, ref, inside = _reference(n, TF, frac)
    assert inside == -1, "the input is too close to the ball to call"
    P = _P(sipx, n, TF, tau)
    y = P(v.copy())
    _check(v, y, ref, n, TF, f"frac {frac}")
    assert l1_exact.same_bits(P(v.copy()), y), "two calls differ"
    assert not l1_exact.same_bits(y, v)


# ---- 2. radius 2.0: the input's bits, a planted -0.0 included ------------------------------------------------------------------------------------
@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("n", GRIDS)
def test_an_input_inside_the_ball_comes_back_bit_for_bit(sipx, TF, n):
    v, nrm, _ = _input(n, TF)
    v[::7] = -0.0
    v[3::11] = 0.0
    tau = TF(2.0 * nrm)                      # (zeroing entries does not raise the norm past twice the input's ...)
    assert R.inside(v, n, tau) == 1 and np.any(np.signbit(v) & (v == 0))      # (... and the reference says so)
    P = _P(sipx, n, TF, tau)
    assert l1_exact.same_bits(P(v.copy()), v)
    assert l1_exact.same_bits(P(v.copy()), v), "two calls differ"
    if n == GRIDS[3]:
        z = np.zeros_like(v)
        z[::2] = -0.0
        assert l1_exact.same_bits(_P(sipx, n, TF, 1.0)(z.copy()), z)


# ---- 3. exact cases: small integers, frame 0 carries only D_y members and frame 1 only D_x members -------------------------------------------
EXACT_N = (3, 2, 2)      # pixels (0,0), (1,0) have both members, (2,0) D_y alone, (0,1), (1,1) D_x alone, (2,1) none
# per case: {(i, j): (vy in frame 0, vx in frame 1)}, the radius, {(i, j): (expected vy, expected vx)}; every J_p is diagonal, so its
# singular values are |vy| and |vx|, theta = 1 and every non-zero entry comes back one closer to zero
EXACT = [
    ({(0, 0): (4, 2), (1, 0): (5, 0)}, 8.0, {(0, 0): (3, 1), (1, 0): (4, 0)}),                       # sigma 4, 2, 5: (11 - 8) / 3
    ({(0, 0): (-2, 4), (1, 0): (0, -5), (2, 0): (3, None), (0, 1): (None, 6)}, 15.0,                 # sigma 4, 2, 5, 3, 6: (20 - 15) / 5
     {(0, 0): (-1, 3), (1, 0): (0, -4), (2, 0): (2, None), (0, 1): (None, 5)}),
    ({(0, 0): (4, 3), (1, 0): (5, 0), (1, 1): (None, 1)}, 9.0, {(0, 0): (3, 2), (1, 0): (4, 0), (1, 1): (None, 0)}),   # 4, 3, 5 (, 1): theta 1
]


def _exact_vector(n, TF, entries):
    G = RJ._members(n)
    v = np.zeros(R.rows(n), TF)
    for (i, j), (vy, vx) in entries.items():
        p = i + n[0] * j
        if vy is not None:
            v[G[p, 0, 0]] = vy
        if vx is not None:
            v[G[p, 1, 1]] = vx
    return v


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("case", range(len(EXACT)))
def test_exact_integer_cases(sipx, TF, case):
    entries, tau, expect = EXACT[case]
    v, want = _exact_vector(EXACT_N, TF, entries), _exact_vector(EXACT_N, TF, expect)
    s = R.svals(v, EXACT_N, TF)
    assert np.array_equal(s, np.round(s)) and l1_exact.exact_theta(s.astype(np.float64), tau)[0] == 1.0
    y = _P(sipx, EXACT_N, TF, tau)(v.copy())
    assert np.array_equal(y, want), (y, want)


# ---- 4. rank-1 stacks: the joint l2,1 ball at the same radius; the two norms -----------------------------------------------------------------------
RANK1_GRIDS = [(33, 20, 3), (32, 12, 8), (8, 4, 67)]


def _rank1(n, TF, kind):
    """kind "multiples": every frame a power of two times frame 0 (exactly rank 1 in TF); "one frame": one non-zero frame."""
    full, _ = make_input(n, TF)
    v = np.zeros_like(full)
    if kind == "one frame":
        mem = RF.frame_rows(n, n[2] // 2)
        v[mem] = full[mem]
        return v
    base = full[RF.frame_rows(n, 0)]
    for k in range(n[2]):
        v[RF.frame_rows(n, k)] = base * TF((-1.0) ** k * 2.0 ** (k % 3 - 1))
    return v


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("kind", ["multiples", "one frame"])
@pytest.mark.parametrize("n", RANK1_GRIDS)
def test_rank_one_stacks_give_the_joint_ball(sipx, TF, kind, n):
    v = _rank1(n, TF, kind)
    eps = float(np.finfo(TF).eps)
    s2 = R.exact_svd(v, n)[1]
    assert float(np.max(s2)) <= 64 * float(np.finfo(l1_exact._WIDE).eps) * float(np.max(R.frob(v, n))), "the stack is not rank 1"
    tau = TF(0.5 * RJ.norm21(v, n))
    assert RJ.inside(v, n, tau) == -1 and R.inside(v, n, tau) == -1
    y = _P(sipx, n, TF, tau)(v.copy())
    want = _P(sipx, n, TF, tau, "l21_joint")(v.copy())
    worst = float(R.error(y, want, v, n).max()) / eps
    print(f"tnv rank 1 ({kind}) {n} {np.dtype(TF).name}: worst difference to l21_joint {worst:.3f} eps |J_p|_F (bound {R.BOUND[TF]})")
    assert not l1_exact.same_bits(y, v) and worst <= R.BOUND[TF]


def _stack(n, TF, kind):
    """A model x (not a gradient field) on grid n: "general", or a rank-1 stack of frames as _rank1 builds them."""
    rng = np.random.default_rng(7 + sum(n))
    if kind == "general":
        x = rng.standard_normal(n) * (1.0 + np.arange(n[2]))[None, None, :]
    else:
        base = rng.standard_normal(n[:2])
        x = np.zeros(n)
        for k in range(n[2]):
            if kind == "multiples":
                x[:, :, k] = base * ((-1.0) ** k * 2.0 ** (k % 3 - 1))
            elif k == n[2] // 2:
                x[:, :, k] = base
    return x.reshape(-1, order="F").astype(TF)


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("n", RANK1_GRIDS)
def test_the_nuclear_norm_bounds_the_joint_norm_and_meets_it_at_rank_one(sipx, TF, n):
    g = sipx.compgrid((1.0, 1.0, 1.0), n)      # (unit spacing: the differences of a power-of-two multiple are that multiple exactly)
    eps = float(np.finfo(TF).eps)
    x = _stack(n, TF, "general")
    assert sipx.tnv_norm(x, g) >= sipx.l21_joint_norm(x, g) > 0
    for kind in ("multiples", "one frame"):
        x = _stack(n, TF, kind)
        a, b = float(sipx.tnv_norm(x, g)), float(sipx.l21_joint_norm(x, g))
        assert b > 0 and abs(a - b) <= 4 * eps * b, (kind, a, b)


# ---- 5. an observed radius leaves the point unwritten; half of it is met ---------------------------------------------------------------------------
@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("n", OBSERVE_GRIDS)
def test_an_observed_radius_leaves_the_point_unwritten(sipx, TF, n):
    g = sipx.compgrid((3.0, 4.0, 5.0), n)
    x = _stack(n, TF, "general")
    v = sipx.TDOperator("TV_xy", g, TF) @ x
    eps = float(np.finfo(TF).eps)
    tau = sipx.tnv_norm(x, g)
    assert isinstance(tau, TF)
    ref = R.norm(v, n)
    assert abs(float(tau) - ref) <= 2 * eps * ref
    mk = lambda t: sipx.Projector(sipx.set_definitions("tnv", "TV_xy", 0.0, float(t), ("tensor", "")), g, TF)
    assert l1_exact.same_bits(mk(tau)(v.copy()), v), "TV_xy x was written although its radius was observed on x"
    td = sipx.tnv_norm(torch.from_numpy(x).cuda(), g)
    assert td.is_cuda and td.shape == (1,) and l1_exact.same_bits(td.cpu().numpy(), np.array([tau], TF))
    t0 = sipx.tnv_norm(np.zeros(int(np.prod(n)), TF), g)
    assert isinstance(t0, TF) and t0 == 0
    # half the radius: the output lies on the boundary.  Every member is within BOUND eps |J_p|_F of a point whose norm is the radius,
    # L pixels: BOUND eps L in units of the largest |J_p|_F
    half = TF(0.5 * float(tau))
    y = mk(half)(v.copy())
    assert not l1_exact.same_bits(y, v)
    L = n[0] * n[1]
    miss = abs(R.norm(y, n) - float(half))
    print(f"tnv boundary {n} {np.dtype(TF).name}: |norm(y) - tau| = {miss / (eps * L * float(R.frob(v, n).max())):.3f} eps L max|J_p|_F")
    assert miss <= R.BOUND[TF] * eps * L * float(R.frob(v, n).max())


# ---- 6. whole solves against the oracle (rules and tolerances of tests/test_gpu_l21_joint.py, test_solve_matches_oracle) -------------------------
SOLVE_GRIDS, SOLVE_H = [(33, 20, 3), (8, 4, 67)], (25.0, 25.0, 25.0)


def _solve_problem(mod, n, TF, m, opt_kw):
    """{bounds, tnv on TV_xy} for module `mod`; radius: half the norm of A m from the reference.  The oracle is given TV_xy as a custom
    operator -- its own D_y and D_x stacked -- with the l1 ball, whose projector is replaced by the reference."""
    h = SOLVE_H
    g = mod.compgrid(h, n)
    opt = mod.PARSDMM_options(FL=TF, **opt_kw)
    c = [mod.set_definitions("bounds", "identity", 1600.0, 3900.0, ("tensor", ""))]
    A = _stacked(n, h, TF)
    r = TF(0.5 * R.norm(np.asarray(A @ m, TF), n))
    if mod is O:
        c.append(mod.set_definitions("l1", "identity", 0.0, float(r), ("tensor", ""), (A, False)))
    else:
        c.append(mod.set_definitions("tnv", "TV_xy", 0.0, float(r), ("tensor", "")))
    P, A, prop = mod.setup_constraints(c, g, TF)
    if mod is O:
        P[1] = lambda x: _in_place(R.project, x, n, r)
    A, AtA, l, y = mod.PARSDMM_precompute_distribute(A, prop, g, opt)
    return g, opt, P, A, prop, AtA


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("n", SOLVE_GRIDS)
def test_solve_matches_oracle(sipx, TF, n):
    m = _model(n, TF, seed=2)
    kw = dict(maxit=60)
    go, oo, Po, Ao, propo, AtAo = _solve_problem(O, n, TF, m, kw)
    gs, os_, Ps, As, props, AtAs = _solve_problem(sipx, n, TF, m, kw)
    assert props.ncvx == propo.ncvx
    xo, lo, l_o, y_o = O.PARSDMM(m.copy(), AtAo, Ao, propo, Po, go, oo)
    xs, ls, l_s, y_s = sipx.PARSDMM(m.copy(), AtAs, As, props, Ps, gs, os_)
    K = min(6, len(lo.obj), len(ls.obj))
    rt = 5e-4 if TF == np.float32 else 1e-8
    assert np.array_equal(ls.cg_it[:K], lo.cg_it[:K])
    for f in ("obj", "r_pri_total", "r_dual_total", "rho", "gamma"):
        a, b = np.asarray(getattr(ls, f))[:K], np.asarray(getattr(lo, f))[:K]
        assert np.allclose(a, b, rtol=rt, atol=1e-12), (f, a, b)
    assert len(ls.obj) == len(lo.obj) or min(len(ls.obj), len(lo.obj)) > 6
    assert np.array_equal(ls.set_feasibility[0], lo.set_feasibility[0]) or \
        np.allclose(ls.set_feasibility[0], lo.set_feasibility[0], rtol=rt)
    err = np.linalg.norm(xs.astype(np.float64) - xo) / np.linalg.norm(xo)
    Kc = min(len(ls.obj), len(lo.obj))
    sep_rt = 1e-5 if TF == np.float32 else 1e-6
    sep = next((k for k in range(Kc) if ls.cg_it[k] != lo.cg_it[k] or not np.allclose(ls.rho[k], lo.rho[k], rtol=sep_rt)), None)
    upto = Kc if sep is None else sep
    for f in ("obj", "r_pri_total", "rho", "gamma"):
        a, b = np.asarray(getattr(ls, f))[:upto], np.asarray(getattr(lo, f))[:upto]
        assert np.allclose(a, b, rtol=(5e-4 if TF == np.float32 else 1e-6), atol=1e-12), (f, upto)
    tol = 5e-4 if TF == np.float32 else 1e-6
    print(f"tnv solve {n} {np.dtype(TF).name}: iterations {len(ls.obj)} / {len(lo.obj)}, separation {sep}, rel diff {err:.3e}")
    if sep is not None or len(ls.obj) != len(lo.obj):
        # after a separation: the oracle again with the engine's rho / gamma history forced on it
        gr, orr, Pr, Ar, propr, AtAr = _solve_problem(O, n, TF, m, dict(kw, maxit=len(ls.obj)))
        xr, lr, _, _ = O.PARSDMM(m.copy(), AtAr, Ar, propr, Pr, gr, orr, replay=(ls.rho, ls.gamma))
        err_replay = np.linalg.norm(xs.astype(np.float64) - xr) / np.linalg.norm(xr)
        assert err_replay < tol, (n, "replayed", sep, err_replay)
        tol = max(tol, 5e-4)
        assert _julia_max(ls.set_feasibility[-1]) <= max(_julia_max(lo.set_feasibility[-1]), float(os_.feas_tol))
    assert err < tol, (n, sep, err)
    assert ls.r_pri.shape == (len(ls.obj), 3) and ls.set_feasibility.shape[1] == 2
    assert len(y_s) == 3 and [len(q) for q in y_s] == [len(q) for q in y_o]
    assert len(ls.obj) > 6, "the solve stopped before anything was compared"


# ---- 7. refusals through the C ABI and through host.py, each with its exact text --------------------------------------------------------------------
ROUTE = "total nuclear variation couples the frames of TV_xy: TD_OP must be TV_xy, mode tensor, no transform"
NO_WEIGHTS = ("total nuclear variation (tnv) takes no weights or vectors (lb, ub): the weighted set across the frames is "
              "(\"l21_joint\", \"TV_xy\")")
RADIUS = "Radius of L1 ball is negative"
SHARDED = ("the TV_xy operator takes single-process contexts only, this one has a communicator, a slab decomposition or set ownership: "
           "use D_x and D_y sets, or a single process")
NEEDS_3D = ("provided an unknown transform domain operator. check function get_TD_operator(comp_grid,TD_type,TF) for options "
            "(TV_xy is the in-plane gradient of a 3-D grid; on a 2-D grid TV is in-plane already)")
PROJ_TNV = 17


def _desc(sipx, op, proj=PROJ_TNV, mode=0, pmax=1.0, transform=0, dir=0, component=0):
    d = sipx.host._SetDesc()
    d.op, d.proj, d.pmin, d.pmax, d.mode, d.dir, d.transform, d.component = op, proj, 0.0, pmax, mode, dir, transform, component
    return d


def _refused(sipx, ctx, d):
    rc = sipx.lib().sipx_add_set(ctx.h, C.byref(d), None, None, 0)
    assert rc < 0, "the engine took the set"
    return sipx.lib().sipx_last_error().decode()


def test_refusals(sipx):
    TF = np.float32
    XY = sipx.host.OPS["TV_xy"]
    assert sipx.host.PROJ["tnv"] == PROJ_TNV
    L = sipx.lib()
    n = (16, 12, 8)
    g = _grid(sipx, n)
    N = int(np.prod(n))
    ctx = sipx.Context(g, TF)
    try:
        for op in ("identity", "D_x", "D_y", "D_z", "TV"):
            assert _refused(sipx, ctx, _desc(sipx, sipx.host.OPS[op])) == ROUTE
        for mode, dr in ((2, 2), (2, 0), (1, 0), (1, 2)):
            assert _refused(sipx, ctx, _desc(sipx, XY, mode=mode, dir=dr)) == ROUTE
        for tr in (1, 2):
            assert _refused(sipx, ctx, _desc(sipx, XY, transform=tr)) == ROUTE
        w = np.ones(n[0] * n[1], TF)
        for field in ("lb", "ub"):
            d = _desc(sipx, XY)
            setattr(d, field, w.ctypes.data_as(C.c_void_p))
            d.reserved = len(w)
            assert _refused(sipx, ctx, d) == NO_WEIGHTS
        for r in (0.0, -2.0, float("nan")):
            assert _refused(sipx, ctx, _desc(sipx, XY, pmax=r)) == RADIUS
        assert _refused(sipx, ctx, _desc(sipx, XY, component=1)) == "the TV_xy operator takes no Minkowski component"
        # after the refusals the context takes the set; it holds no replaceable vectors; sipx_project refuses any other length or operator
        assert L.sipx_add_set(ctx.h, C.byref(_desc(sipx, XY)), None, None, 0) == 0
        assert L.sipx_set_data(ctx.h, 0, None, w.ctypes.data_as(C.c_void_p)) != 0
        assert "holds no replaceable vectors" in L.sipx_last_error().decode()
        v = np.zeros(N, TF)
        assert L.sipx_project(ctx.h, C.byref(_desc(sipx, XY)), v.ctypes.data_as(C.c_void_p), C.c_int64(len(v))) != 0
        assert f"TV_xy range: {R.rows(n)} entries on this grid, {len(v)} given" in L.sipx_last_error().decode()
        assert L.sipx_project(ctx.h, C.byref(_desc(sipx, sipx.host.OPS["TV"])), v.ctypes.data_as(C.c_void_p), C.c_int64(len(v))) != 0
        assert L.sipx_last_error().decode() == ROUTE
        out = np.zeros(1, TF)
        assert L.sipx_tnv_norm(ctx.h, None, out.ctypes.data_as(C.c_void_p)) != 0 and "x and out are needed" in L.sipx_last_error().decode()
        # ... and is still usable
        u = np.arange(R.rows(n), dtype=TF)
        assert L.sipx_project(ctx.h, C.byref(_desc(sipx, XY, pmax=3.0)), u.ctypes.data_as(C.c_void_p), C.c_int64(len(u))) == 0
        assert abs(R.norm(u, n) - 3.0) <= 1e-5 * 3.0
        x = np.random.default_rng(1).standard_normal(N).astype(TF)
        assert L.sipx_tnv_norm(ctx.h, x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == 0
        assert out[0] == sipx.tnv_norm(x, g) > 0
    finally:
        ctx.close()
    # a 2-D grid, and a grid with one frame, which is one: the operator's own refusal
    for n2 in ((16, 12), (4, 3, 1)):
        ctx = sipx.Context(_grid(sipx, n2), TF)
        try:
            assert _refused(sipx, ctx, _desc(sipx, XY)) == NEEDS_3D
            out = np.zeros(1, TF)
            assert L.sipx_tnv_norm(ctx.h, np.zeros(int(np.prod(n2)), TF).ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) != 0
            assert L.sipx_last_error().decode() == NEEDS_3D
        finally:
            ctx.close()
    # a sharded context -- a slab decomposition or set ownership: at sipx_add_set, or at sipx_finalize when it came later
    ctx = sipx.Context(g, TF)
    try:
        ctx.set_decomp("slab")
        assert _refused(sipx, ctx, _desc(sipx, XY)) == SHARDED
    finally:
        ctx.close()
    for late in ("slab", "owned"):
        ctx = sipx.Context(g, TF)
        try:
            assert L.sipx_add_set(ctx.h, C.byref(_desc(sipx, XY)), None, None, 0) == 0
            if late == "slab":
                ctx.set_decomp("slab")
            else:
                ctx.set_owned([1, 1])
            with pytest.raises(sipx.SipxError) as e:
                ctx.finalize(np.ones(N, TF), [10.0], 1.0)
            assert SHARDED in str(e.value)
        finally:
            ctx.close()


def test_host_refusals_word_for_word(sipx):
    TF = np.float32
    g3 = _grid(sipx, (16, 12, 8))

    def setup(op, mx, mode, g=g3, cust=((), False), **kw):
        return sipx.setup_constraints([sipx.set_definitions("tnv", op, 0.0, mx, mode, cust, **kw)], g, TF)

    def text(f):
        with pytest.raises(sipx.SipxError) as e:
            f()
        return str(e.value)
    for op in ("identity", "D_x", "D_z", "TV", "DFT", "wavelet"):                       # wrong operator, a transform
        assert text(lambda: setup(op, 1.0, ("tensor", ""))) == ROUTE
    for mode in (("slice", "z"), ("fiber", "x")):                                        # wrong mode
        assert text(lambda: setup("TV_xy", 1.0, mode)) == ROUTE
    assert text(lambda: setup("TV_xy", 1.0, ("tensor", ""), weights=np.ones(16 * 12, TF))) == NO_WEIGHTS
    assert text(lambda: setup("TV_xy", np.ones(8, TF), ("tensor", ""))) == NO_WEIGHTS
    assert text(lambda: setup("TV_xy", -1.0, ("tensor", ""))) == RADIUS
    for n2 in ((16, 12), (4, 3, 1)):
        assert text(lambda: setup("TV_xy", 1.0, ("tensor", ""), _grid(sipx, n2))) == NEEDS_3D
    P, A, prop = setup("TV_xy", 2.0, ("tensor", ""))
    assert prop.tag[0] == ("tnv", "TV_xy", "tensor", "") and P[0].kind == "tnv" and P[0].data_len(A[0]) is None
    assert text(lambda: P[0].check_rows(sipx.TDOperator("TV", g3, TF))) == ROUTE
