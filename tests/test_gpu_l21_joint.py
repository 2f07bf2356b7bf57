"""Joint (vectorial) isotropic total variation across frames on the GPU: the ("l21_joint", "TV_xy") set (csrc/l21_joint.h,
csrc/ext_group.hip, BallProj) against tests/l21_joint_ref.py: the projector at four radii, inputs it must not write, exact ties, the
whole-array set on an input with one non-zero frame, observed radii (sipx.l21_joint_norm), whole solves against the oracle on the same
operator given as custom_TD_OP with its projector swapped for the reference, and the engine's refusals through the C ABI.

GRIDS and the path each takes (l21_joint_plan cuts the n3 frames into min(ceil(131072 / (L sizeof(T) / 16)), n3 / 8) chunks, L = n1 n2;
the norms / scale kernels take 16 bytes per thread when n1 % 4 == 0 and launch min(ceil(items / 256), 2048) workgroups):
  (4, 3, 2), (5, 4, 3)   every boundary class; 16 bytes (one vector per grid line) on (4, 3, 2), one pixel per thread on (5, 4, 3);
                         n3 below the unroll batch of 4 frames; one chunk
  (33, 20, 3)            odd n1, one pixel per thread, 660 pixels: more than one workgroup; one chunk
  (32, 12, 8)            16-byte path; n3 = 8 < 16: one chunk, two full batches
  (8, 4, 67)             n3 prime: 8 chunks of 9 frames (two batches and a single frame), the last one ragged with 4 frames; 16 bytes
  (4, 3, 15), (4, 3, 16) the two sides of the chunk boundary, n3 / 8 = 1 and 2: one chunk of 15 frames, two chunks of 8
  (1024, 1028, 2)        2 105 344 points > 2048 * 256 * 4: a second, partial grid-stride sweep of the scale kernel in both precisions
  (1021, 515, 2)         odd n1, 525 815 pixels > 2048 * 256: a second sweep of the norms kernel, one pixel per thread
tests/test_l21_joint_cpu.py asserts these claims from the plan.
Worst |y - ref| / (eps |v|) observed on an MI355X: see DESIGN.md section 7f."""
import ctypes as C

import numpy as np
import pytest
import torch      # (before libsipx.so is loaded: one HIP runtime in the process)

from oracle import parsdmm_oracle as O
from tests import l1_exact, l21_frames_ref as RF, l21_joint_ref as R
from tests.test_gpu_l21_frames import LOG_FIELDS, _in_place, _julia_max, _model, _stacked, make_input

pytestmark = pytest.mark.gpu

GRIDS = [(4, 3, 2), (5, 4, 3), (33, 20, 3), (32, 12, 8), (8, 4, 67), (4, 3, 15), (4, 3, 16), (1024, 1028, 2), (1021, 515, 2)]
CHUNKED = [(8, 4, 67), (4, 3, 16)]
OBSERVE_GRIDS = [(33, 20, 3), (4, 3, 15)] + CHUNKED
FRACS = [0.9, 0.5, 0.05]
PRECISIONS = [np.float32, np.float64]
_norms, _refs = {}, {}


def _grid(sipx, n):
    return sipx.compgrid(tuple(1.0 for _ in n), n)


def _P(sipx, n, TF, tau, st="l21_joint"):
    return sipx.Projector(sipx.set_definitions(st, "TV_xy", 0.0, float(tau), ("tensor", "")), _grid(sipx, n), TF)


def _input(n, TF):
    """(v, its joint norm): make_input of tests/test_gpu_l21_frames.py -- heavy-tailed, the frames scaled apart."""
    v, _ = make_input(n, TF)
    key = (n, np.dtype(TF).name)
    if key not in _norms:
        _norms[key] = R.norm21(v, n)
    return v, _norms[key]


def _reference(n, TF, frac):
    key = (n, np.dtype(TF).name, frac)
    if key not in _refs:
        v, nrm = _input(n, TF)
        tau = TF(frac * nrm)
        ref = R.project(v, n, tau)
        ref.setflags(write=False)
        _refs[key] = (tau, ref, R.inside(v, n, tau))
    return _refs[key]


def bound(n, TF):
    """|y - ref| <= bound eps |v|: one rounding each of g, theta, g - theta, the quotient and the product; in Float64 the float64 sum of
    squares itself can be off by (n3 / 2 + 1 / 4) eps relative in g."""
    return 4.0 if TF == np.float32 else max(4.0, 3.0 + n[2] / 2.0)


def _check(v, y, ref, n, TF, tag):
    eps = float(np.finfo(TF).eps)
    a = np.abs(v.astype(np.float64))
    err = np.abs(y.astype(np.float64) - ref)
    worst = float(np.max(err / np.maximum(a, np.finfo(np.float64).tiny)) / eps)
    print(f"l21 joint {tag} {n} {np.dtype(TF).name}: worst error {worst:.3f} eps |v| (bound {bound(n, TF)})")
    assert np.all(err <= bound(n, TF) * eps * a), f"worst error {worst:.3f} eps |v|"
    return worst


# ---- 1. the projector against the reference; two calls give the same bits ---------------------------------------------------------------------
@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("frac", FRACS)
@pytest.mark.parametrize("n", GRIDS)
def test_projector_matches_the_reference(sipx, TF, frac, n):
    v, nrm = _input(n, TF)
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
    v, _ = _input(n, TF)
    v[::7] = -0.0
    v[3::11] = 0.0
    tau = TF(2.0 * R.norm21(v, n))
    assert R.inside(v, n, tau) == 1 and np.any(np.signbit(v) & (v == 0))
    P = _P(sipx, n, TF, tau)
    assert l1_exact.same_bits(P(v.copy()), v)
    assert l1_exact.same_bits(P(v.copy()), v), "two calls differ"
    if n == GRIDS[3]:
        z = np.zeros_like(v)
        z[::2] = -0.0
        assert l1_exact.same_bits(_P(sipx, n, TF, 1.0)(z.copy()), z)


# ---- 3. ties: integer components, exact norms, an exact threshold ---------------------------------------------------------------------------------
SEVENS = [{(0, 0): 7}, {(0, 0): 2, (1, 1): 3, (2, 0): 6}, {(2, 1): -7}, {(0, 1): 6, (1, 0): -3, (2, 1): 2}]
FIVES = [{(0, 0): 3, (1, 1): 4}, {(1, 0): 5}, {(0, 1): 4, (2, 0): -3}, {(2, 1): 5}, {(0, 0): -3, (0, 1): 4}, {(1, 1): -5},
         {(1, 0): 4, (2, 0): 3}, {(0, 1): 5}, {(2, 0): 3, (2, 1): -4}]


def _tie_input(n, TF):
    """4 pixels of norm 7 and 9 of norm 5, their members spread over the frames and the two blocks (2-3-6, 3-4-5, axis-aligned), every
    other pixel norm 1 or none: radius 8 puts theta = 5 exactly."""
    G = R._members(n)
    v = np.zeros(R.rows(n), TF)
    kind = np.zeros(G.shape[0], int)
    for p in range(G.shape[0]):
        k = p % n[2]
        mem = G[p, k][G[p, k] >= 0]
        if len(mem):
            v[mem[p % len(mem)]] = -1 if p % 3 == 0 else 1
            kind[p] = 1
    full = np.nonzero((G >= 0).all(axis=(1, 2)))[0]
    pick = np.random.default_rng(41).permutation(full)
    for p, comp in zip(pick, SEVENS + FIVES):
        v[G[p][G[p] >= 0]] = 0
        for (k, q), val in comp.items():
            v[G[p, k, q]] = val
        kind[p] = 7 if sum(c * c for c in comp.values()) == 49 else 5
    return v, G, kind


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("n", [(8, 6, 3), (9, 7, 16)])
def test_pixels_on_the_threshold_are_zeroed_in_every_frame(sipx, TF, n):
    v, G, kind = _tie_input(n, TF)
    g = R.norms(v, n, TF)
    assert np.array_equal(g, kind.astype(TF)) and (kind == 7).sum() == 4 and (kind == 5).sum() == 9 and (kind == 1).sum() > 9
    assert l1_exact.exact_theta(g.astype(np.float64), TF(8.0))[0] == 5.0
    y = _P(sipx, n, TF, 8.0)(v.copy())
    for kk in (5, 1):
        mem = G[kind == kk]
        assert np.all(y[mem[mem >= 0]] == 0), f"a pixel of norm {kk} survived in some frame"
    mem = G[kind == 7]
    mem = mem[mem >= 0]
    want = v[mem].astype(np.float64) * (2.0 / 7.0)
    assert np.all(np.abs(y[mem] - want) <= 4 * float(np.finfo(TF).eps) * np.abs(v[mem]))
    assert np.count_nonzero(y) == np.count_nonzero(v[mem]) == 1 + 3 + 1 + 3


# ---- 4. one non-zero frame: the whole-array set on TV_xy, bit for bit -----------------------------------------------------------------------------
@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("frac", [0.5, 0.05])
@pytest.mark.parametrize("n", [(33, 20, 3), (32, 12, 8), (8, 4, 67)])
def test_a_single_frame_gives_the_bits_of_the_whole_array_set(sipx, TF, frac, n):
    full, _ = _input(n, TF)
    k = n[2] // 2
    v = np.zeros_like(full)
    mem = RF.frame_rows(n, k)
    v[mem] = full[mem]
    tau = TF(frac * R.norm21(v, n))
    assert R.inside(v, n, tau) == -1
    y = _P(sipx, n, TF, tau)(v.copy())
    want = _P(sipx, n, TF, tau, "l21")(v.copy())
    assert not l1_exact.same_bits(y, v) and l1_exact.same_bits(y, want)
    rest = np.setdiff1d(np.arange(len(v)), mem)
    assert l1_exact.same_bits(y[rest], v[rest])


# ---- 5. an observed radius leaves the point unwritten -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("n", OBSERVE_GRIDS)
def test_an_observed_radius_leaves_the_point_unwritten(sipx, TF, n):
    g = sipx.compgrid((3.0, 4.0, 5.0), n)
    x = np.random.default_rng(5 + sum(n)).standard_normal(n)
    x *= (1.0 + np.arange(n[2]))[None, None, :]
    x = x.reshape(-1, order="F").astype(TF)
    v = sipx.TDOperator("TV_xy", g, TF) @ x
    eps = float(np.finfo(TF).eps)
    tau = sipx.l21_joint_norm(x, g)
    assert isinstance(tau, TF)
    ref = float(np.sum(R.norms(v, n, TF).astype(l1_exact._WIDE)))
    assert abs(float(tau) - ref) <= 2 * eps * ref
    mk = lambda t: sipx.Projector(sipx.set_definitions("l21_joint", "TV_xy", 0.0, float(t), ("tensor", "")), g, TF)
    assert l1_exact.same_bits(mk(tau)(v.copy()), v), "TV_xy x was written although its radius was observed on x"
    assert not l1_exact.same_bits(mk(float(tau) * 0.999)(v.copy()), v)
    td = sipx.l21_joint_norm(torch.from_numpy(x).cuda(), g)
    assert td.is_cuda and td.shape == (1,) and l1_exact.same_bits(td.cpu().numpy(), np.array([tau], TF))
    t0 = sipx.l21_joint_norm(np.zeros(int(np.prod(n)), TF), g)
    assert isinstance(t0, TF) and t0 == 0


# ---- 6. whole solves against the oracle (rules and tolerances of tests/test_gpu_l21_frames.py, test_solve_matches_oracle) ------------------------
SOLVE_SETS = {"l21-joint": [("l21_joint", "TV_xy", ("tensor", ""))],
              "l21-joint+l1-Dz": [("l21_joint", "TV_xy", ("tensor", "")), ("l1", "D_z", ("tensor", ""))]}
SOLVE_N, SOLVE_H = (16, 12, 8), (25.0, 25.0, 25.0)


def _solve_problem(mod, name, TF, m, opt_kw):
    """{bounds, the sets of SOLVE_SETS[name]} for module `mod`; radii: half the norm of A m from the reference.  The oracle is given
    TV_xy as a custom operator -- its own D_y and D_x stacked -- with the l1 ball, whose projector is replaced by the reference."""
    n, h = SOLVE_N, SOLVE_H
    g = mod.compgrid(h, n)
    opt = mod.PARSDMM_options(FL=TF, **opt_kw)
    c = [mod.set_definitions("bounds", "identity", 1600.0, 3900.0, ("tensor", ""))]
    swaps = []
    for st, opn, mode in SOLVE_SETS[name]:
        A = _stacked(n, h, TF) if opn == "TV_xy" else O.get_TD_operator(O.compgrid(h, n), opn, TF)[0]
        s = np.asarray(A @ m, TF)
        if st == "l21_joint":
            r = TF(0.5 * R.norm21(s, n))
            swaps.append((len(c), lambda x, r=r: _in_place(R.project, x, n, r)))
        else:
            r = TF(0.5 * np.abs(s.astype(np.float64)).sum())
        if mod is O:
            c.append(mod.set_definitions("l1", "identity" if opn == "TV_xy" else opn, 0.0, float(r), ("tensor", ""),
                                         (A, False) if opn == "TV_xy" else ((), False)))
        else:
            c.append(mod.set_definitions(st, opn, 0.0, float(r), mode))
    P, A, prop = mod.setup_constraints(c, g, TF)
    if mod is O:
        for i, f in swaps:
            P[i] = f
    A, AtA, l, y = mod.PARSDMM_precompute_distribute(A, prop, g, opt)
    return g, opt, P, A, prop, AtA


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("name", list(SOLVE_SETS))
def test_solve_matches_oracle(sipx, TF, name):
    m = _model(SOLVE_N, TF, seed=1 + len(SOLVE_SETS[name]))
    kw = dict(maxit=60)
    go, oo, Po, Ao, propo, AtAo = _solve_problem(O, name, TF, m, kw)
    gs, os_, Ps, As, props, AtAs = _solve_problem(sipx, name, TF, m, kw)
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
    print(f"{name} {SOLVE_N} {np.dtype(TF).name}: iterations {len(ls.obj)} / {len(lo.obj)}, separation {sep}, rel diff {err:.3e}")
    if sep is not None or len(ls.obj) != len(lo.obj):
        # after a separation: the oracle again with the engine's rho / gamma history forced on it
        gr, orr, Pr, Ar, propr, AtAr = _solve_problem(O, name, TF, m, dict(kw, maxit=len(ls.obj)))
        xr, lr, _, _ = O.PARSDMM(m.copy(), AtAr, Ar, propr, Pr, gr, orr, replay=(ls.rho, ls.gamma))
        err_replay = np.linalg.norm(xs.astype(np.float64) - xr) / np.linalg.norm(xr)
        assert err_replay < tol, (name, "replayed", sep, err_replay)
        tol = max(tol, 5e-4)
        assert _julia_max(ls.set_feasibility[-1]) <= max(_julia_max(lo.set_feasibility[-1]), float(os_.feas_tol))
    assert err < tol, (name, sep, err)
    p = len(SOLVE_SETS[name]) + 2
    assert ls.r_pri.shape == (len(ls.obj), p) and ls.set_feasibility.shape[1] == p - 1
    assert len(y_s) == p and [len(q) for q in y_s] == [len(q) for q in y_o]
    assert len(ls.obj) > 6, "the solve stopped before anything was compared"


def test_device_form_and_solver_give_the_bits_of_the_host_form(sipx):
    TF = np.float32
    m = _model(SOLVE_N, TF, seed=3)
    g, opt, P, A, prop, AtA = _solve_problem(sipx, "l21-joint+l1-Dz", TF, m, dict(maxit=30))
    args = (AtA, A, prop, P, g, opt)
    sipx.clear_context_cache()
    try:
        xh, logh, lh, yh = sipx.PARSDMM(m.copy(), *args)
        sipx.clear_context_cache()
        xd, logd, ld, yd = sipx.PARSDMM_device(torch.from_numpy(m.copy()).cuda(), *args)
        assert not logd.context_reused
        assert xd.is_cuda and np.array_equal(xd.cpu().numpy(), xh)
        assert len(ld) == len(lh) and len(yd) == len(yh)
        for a, b in zip(list(ld) + list(yd), list(lh) + list(yh)):
            assert a.is_cuda and np.array_equal(a.cpu().numpy(), b)
        for f in LOG_FIELDS:
            a, b = np.asarray(getattr(logd, f)), np.asarray(getattr(logh, f))
            assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), f
        assert len(logh.obj) > 1, "the solve stopped before it began: nothing was compared"
    finally:
        sipx.clear_context_cache()
    with sipx.Solver(*args, TF) as S:
        x, log, l, y = S(m.copy())
        assert np.array_equal(x, xh) and np.array_equal(np.asarray(log.obj), np.asarray(logh.obj))
        with pytest.raises(sipx.SipxError, match=r"holds no replaceable vectors"):
            S.set_data(1, ub=np.ones(SOLVE_N[2], TF))


# ---- 7. the engine's refusals through the C ABI ----------------------------------------------------------------------------------------------------
JOINT = "the joint l2,1 ball groups the frames of TV_xy: TD_OP must be TV_xy, mode tensor"


def _desc(sipx, op, proj=15, mode=0, pmax=1.0, transform=0, dir=0, component=0):
    d = sipx.host._SetDesc()
    d.op, d.proj, d.pmin, d.pmax, d.mode, d.dir, d.transform, d.component = op, proj, 0.0, pmax, mode, dir, transform, component
    return d


def _refused(sipx, ctx, d):
    rc = sipx.lib().sipx_add_set(ctx.h, C.byref(d), None, None, 0)
    assert rc < 0, "the engine took the set"
    return sipx.lib().sipx_last_error().decode()


def test_engine_refusals(sipx):
    TF = np.float32
    XY = sipx.host.OPS["TV_xy"]
    assert sipx.host.PROJ["l21_joint"] == 15
    L = sipx.lib()
    n = (16, 12, 8)
    g = _grid(sipx, n)
    N = int(np.prod(n))
    ctx = sipx.Context(g, TF)
    try:
        for op in ("identity", "D_x", "D_y", "D_z", "TV"):
            assert _refused(sipx, ctx, _desc(sipx, sipx.host.OPS[op])) == JOINT
        for mode, dr in ((2, 2), (2, 0), (1, 0), (1, 2)):
            assert _refused(sipx, ctx, _desc(sipx, XY, mode=mode, dir=dr)) == JOINT
        for tr in (1, 2):
            assert _refused(sipx, ctx, _desc(sipx, XY, transform=tr)) == JOINT
        for r in (0.0, -2.0, float("nan")):
            assert _refused(sipx, ctx, _desc(sipx, XY, pmax=r)) == "Radius of L1 ball is negative"
        assert "the TV_xy operator takes no Minkowski component" in _refused(sipx, ctx, _desc(sipx, XY, component=1))
        # the texts ("l21", ...) answers with stay
        assert "frames run along z" in _refused(sipx, ctx, _desc(sipx, XY, 14, mode=2, dir=0))
        assert "TD_OP must be TV (D2D, D3D)" in _refused(sipx, ctx, _desc(sipx, 1, 14))
        # after the refusals the context takes the set; it holds no replaceable vectors; sipx_project refuses any other length
        assert L.sipx_add_set(ctx.h, C.byref(_desc(sipx, XY)), None, None, 0) == 0
        ub = np.ones(n[2], TF)
        assert L.sipx_set_data(ctx.h, 0, None, ub.ctypes.data_as(C.c_void_p)) != 0
        assert "holds no replaceable vectors" in L.sipx_last_error().decode()
        v = np.zeros(N, TF)
        assert L.sipx_project(ctx.h, C.byref(_desc(sipx, XY)), v.ctypes.data_as(C.c_void_p), C.c_int64(len(v))) != 0
        assert f"TV_xy range: {R.rows(n)} entries on this grid, {len(v)} given" in L.sipx_last_error().decode()
        assert L.sipx_project(ctx.h, C.byref(_desc(sipx, sipx.host.OPS["TV"])), v.ctypes.data_as(C.c_void_p), C.c_int64(len(v))) != 0
        assert L.sipx_last_error().decode() == JOINT
        out = np.zeros(1, TF)
        assert L.sipx_l21_joint_norm(ctx.h, None, out.ctypes.data_as(C.c_void_p)) != 0 and "x and out are needed" in L.sipx_last_error().decode()
        # ... and is still usable
        w = np.arange(R.rows(n), dtype=TF)
        assert L.sipx_project(ctx.h, C.byref(_desc(sipx, XY, pmax=3.0)), w.ctypes.data_as(C.c_void_p), C.c_int64(len(w))) == 0
        assert abs(R.norm21(w, n) - 3.0) <= 1e-5 * 3.0
        x = np.random.default_rng(1).standard_normal(N).astype(TF)
        assert L.sipx_l21_joint_norm(ctx.h, x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == 0
        assert out[0] == sipx.l21_joint_norm(x, g) > 0
    finally:
        ctx.close()
    # a 2-D grid: the operator's own refusal
    ctx = sipx.Context(_grid(sipx, (16, 12)), TF)
    try:
        msg = _refused(sipx, ctx, _desc(sipx, XY))
        assert "provided an unknown transform domain operator" in msg and "TV_xy" in msg
        out = np.zeros(1, TF)
        assert L.sipx_l21_joint_norm(ctx.h, np.zeros(16 * 12, TF).ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) != 0
        assert "TV_xy" in L.sipx_last_error().decode()
    finally:
        ctx.close()
    # a context with a slab decomposition or set ownership: at sipx_add_set, or at sipx_finalize when it came later
    msg = "the TV_xy operator takes single-process contexts only"
    ctx = sipx.Context(g, TF)
    try:
        ctx.set_decomp("slab")
        assert msg in _refused(sipx, ctx, _desc(sipx, XY))
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
            with pytest.raises(sipx.SipxError, match=msg):
                ctx.finalize(np.ones(N, TF), [10.0], 1.0)
        finally:
            ctx.close()
