"""Simplex sets on the GPU (csrc/seg_simplex.h, csrc/ext_segments.hip: SimplexSegProj, k_simplex_lane, k_simplex_tile) through
sipx.Projector against the exact reference of tests/simplex_ref.py: accuracy at every seam of the two routes, inputs it must not write,
entries on the threshold, the observed sums, the bit identities, whole solves against the oracle with its projector swapped for the
reference, the reset of a live context, the engine's refusals through raw descriptors and the route in the kernel statistics.

BOUND.  |y_i - y*_i| <= 2 eps max(|v_i|, |theta*|): the rounding of theta gives eps/2 |theta|, the subtraction eps/2 (|v_i| + |theta|), an
entry the two sides classify differently lies within eps |theta| of the threshold.  Worst ratio seen on an MI355X over all cases below:
1.45 (Float32), 1.91 (Float64, where the one rounding of the reference to float64 is half an eps of it); the serial rule on the CPU
(tests/test_simplex_cpu.py) reaches 1.11 / 1.86 on its own draws of the same families.

CASES.  Every segment of an input takes one of six families in turn (mixed signs at scales 1e-2 .. 1e2, fractions a little above and a
little below the target, strongly negative, quarter integers, zeros with -0.0), for each of the bounds (1, 1), (0.5, 2), (0, 1).
Lane route (fibers with contiguous neighbours, L <= SIMPLEX_REG_MAX = 16): fiber z (33,3,4) a ragged wave, (65,2,8) two tiles a row, (64,3,16)
the largest bucket, (1,1,2); fiber y (33,7,3); 2-D fiber z (33,20); the bucket edges L = 4|5, 8|9, 16|17 as fiber z of (5,3,L), the
last one on the tile route.  Tile route: fiber x (20,9,6) and 2-D (33,20): contiguous segments; slices x, y, z of (12,10,5); streaming:
slice z of (96,96,2) Float32 / (72,64,2) Float64 (a segment over 32 KiB), fiber z of (32,2,300) (a tile over 32 KiB).  Operators with a
pad row or plane: D_x, fiber z on (8,3,2); D_z, fiber z on (20,9,6) -- the segments leave the pads out, sipx_project hands the engine the
rows alone, so what a pad holds cannot be set from here: tests/test_simplex_cpu.py runs the rule on strided segments between NaN.
Grid-stride: fiber x of (3,8200), 8200 tiles against the plan's cap of 8192; the lane route's cap of 8192 workgroups (4 waves of 64
segments each) with fiber z of (2097216,1,2), Float32 against a vectorised float64 threshold."""
import ctypes as C

import numpy as np
import pytest
import torch      # (before libsipx.so is loaded: one HIP runtime in the process)

from oracle import parsdmm_oracle as O
from tests import l1_exact
from tests import simplex_ref as R
from tests.test_gpu_l21_frames import LOG_FIELDS, _in_place, _julia_max, _model
from tests.test_gpu_set_data import _assert_same
from tests.test_simplex_cpu import BOUNDS, FAMILIES, segment

pytestmark = pytest.mark.gpu

REG_MAX = 16
FZ, FY, FX = ("fiber", "z"), ("fiber", "y"), ("fiber", "x")
LANE_CASES = [("identity", (33, 3, 4), FZ), ("identity", (65, 2, 8), FZ), ("identity", (64, 3, REG_MAX), FZ), ("identity", (1, 1, 2), FZ),
              ("identity", (33, 7, 3), FY), ("identity", (33, 20), FZ)] + \
             [("identity", (5, 3, L), FZ) for L in (4, 5, 8, 9, 16)] + \
             [("D_x", (8, 3, 2), FZ), ("D_z", (20, 9, 6), FZ)]
TILE_CASES = [("identity", (5, 3, REG_MAX + 1), FZ), ("identity", (20, 9, 6), FX), ("identity", (33, 20), FX),
              ("identity", (12, 10, 5), ("slice", "x")), ("identity", (12, 10, 5), ("slice", "y")), ("identity", (12, 10, 5), ("slice", "z")),
              ("identity", (32, 2, 300), FZ), ("identity", (3, 8200), FX)]
STREAM = {np.float32: ("identity", (96, 96, 2), ("slice", "z")), np.float64: ("identity", (72, 64, 2), ("slice", "z"))}
PRECISIONS = [np.float32, np.float64]
_cache = {}
_worst = {}


def _grid(sipx, n, h=None):
    return sipx.compgrid(tuple(1.0 for _ in n) if h is None else h, n)


def _P(sipx, op, n, mode, TF, smin, smax, g=None):
    return sipx.Projector(sipx.set_definitions("simplex", op, float(smin), float(smax), mode), g or _grid(sipx, n), TF)


def _segs(op, n, mode):
    key = ("s", op, n, mode)
    if key not in _cache:
        _cache[key] = R.segments(n, op, mode)
    return _cache[key]


def _input(op, n, mode, TF, smax):
    """Segment s takes family s % 6, the fractions around smax; computed once, handed out as a copy."""
    key = ("v", op, n, mode, np.dtype(TF).name, smax)
    if key not in _cache:
        rng = np.random.default_rng(20261021 + sum(n) + len(op))
        v = np.zeros(R.rows(n, op), TF)
        for s, idx in enumerate(_segs(op, n, mode)):
            v[idx] = segment(FAMILIES[s % len(FAMILIES)], rng, len(idx), TF, smax)
        _cache[key] = v
    return _cache[key].copy()


def _reference(op, n, mode, TF, smin, smax):
    key = ("r", op, n, mode, np.dtype(TF).name, smin, smax)
    if key not in _cache:
        _cache[key] = R.project(_input(op, n, mode, TF, smax), n, op, mode, TF(smin), TF(smax))
    return _cache[key]


def _check(y, ref, theta, v, TF, what):
    eps = float(np.finfo(TF).eps)
    scale = np.maximum(np.abs(v.astype(np.float64)), theta)
    err = np.abs(y.astype(np.float64) - ref)
    worst = float(np.max(err / np.maximum(scale, np.finfo(np.float64).tiny)) / eps)
    _worst[np.dtype(TF).name] = max(_worst.get(np.dtype(TF).name, 0.0), worst)
    print(f"simplex {what} {np.dtype(TF).name}: worst error {worst:.3f} eps max(|v|, |theta*|); so far {_worst}")
    assert np.all(err <= 2 * eps * scale), f"{what}: worst error {worst:.3f} eps max(|v|, |theta*|)"


def _accuracy(sipx, TF, op, n, mode):
    for smin, smax in BOUNDS:
        v = _input(op, n, mode, TF, smax)
        ref, theta = _reference(op, n, mode, TF, smin, smax)
        P = _P(sipx, op, n, mode, TF, smin, smax)
        y = P(v.copy())
        _check(y, ref, theta, v, TF, f"{op} {n} {mode} [{smin}, {smax}]")
        assert l1_exact.same_bits(P(v.copy()), y), "two calls differ"
        assert np.any(y != v)


# ---- 1. the projector against the exact reference --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("op,n,mode", LANE_CASES)
def test_lane_route_matches_the_reference(sipx, TF, op, n, mode):
    _accuracy(sipx, TF, op, n, mode)


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("op,n,mode", TILE_CASES)
def test_tile_route_matches_the_reference(sipx, TF, op, n, mode):
    _accuracy(sipx, TF, op, n, mode)


@pytest.mark.parametrize("TF", PRECISIONS)
def test_a_segment_over_the_lds_budget_streams(sipx, TF):
    op, n, mode = STREAM[TF]
    assert n[0] * n[1] * np.dtype(TF).itemsize > 32 * 1024
    _accuracy(sipx, TF, op, n, mode)


def test_lane_route_past_its_launch_cap(sipx):
    """8192 workgroups of four waves of 64 segments: the first 64 lanes take a second tile.  Float32 against the sort-based threshold
    evaluated in float64 for all segments at once (its own error is 2^-29 of the bound: the factor 1 + 1e-6 below)."""
    TF, L = np.float32, 2
    ns = 8192 * 4 * 64 + 64
    rng = np.random.default_rng(5)
    V = (rng.standard_normal((L, ns)) * 3.0).astype(TF)          # row t: element t of every fiber
    y = _P(sipx, "identity", (ns, 1, L), FZ, TF, 1.0, 1.0)(V.reshape(-1).copy()).reshape(L, ns)
    W = V.astype(np.float64)
    u = -np.sort(-W, axis=0)
    cs = np.cumsum(u, axis=0)
    j = np.arange(1, L + 1)[:, None]
    rho = np.max(np.where(u * j > cs - 1.0, j, 0), axis=0)
    theta = (cs[rho - 1, np.arange(ns)] - 1.0) / rho
    spos = np.maximum(W, 0).sum(axis=0)
    inside = spos.astype(TF) == TF(1.0)
    ref = np.where(inside, np.maximum(W, 0), np.maximum(W - theta, 0))
    scale = np.maximum(np.abs(W), np.where(inside, 0.0, np.abs(theta)))
    err = np.abs(y.astype(np.float64) - ref)
    eps = float(np.finfo(TF).eps)
    worst = float(np.max(err / np.maximum(scale, 1e-300)) / eps)
    print(f"simplex lane route past its cap: worst error {worst:.3f} eps")
    assert np.all(err <= 2 * eps * scale * (1 + 1e-6)), worst
    assert np.any(y[:, -64:] != V[:, -64:]) and np.any(y[:, :64] != V[:, :64])


# ---- 2. inputs the projector must not write, entries on the threshold -------------------------------------------------------------------------
UNWRITTEN = [("identity", (33, 3, 4), FZ), ("identity", (33, 7, 3), FY), ("identity", (20, 9, 6), FX), ("identity", (12, 10, 5), ("slice", "y")),
             ("D_z", (20, 9, 6), FZ), ("identity", (5, 3, REG_MAX + 1), FZ)]


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("op,n,mode", UNWRITTEN)
def test_unwritten_inputs_come_back_bit_for_bit(sipx, TF, op, n, mode):
    rng = np.random.default_rng(7 + sum(n))
    segs = _segs(op, n, mode)
    v = np.zeros(R.rows(n, op), TF)
    for idx in segs:                                   # nonnegative with a -0.0 in front, sums between 0.6 and 1.9
        p = rng.random(len(idx)) + 0.01
        p[0] = 0.0
        v[idx] = (p / p.sum() * rng.uniform(0.6, 1.9)).astype(TF)
        v[idx[0]] = -0.0
    assert np.any(np.signbit(v) & (v == 0))
    assert l1_exact.same_bits(_P(sipx, op, n, mode, TF, 0.5, 2.0)(v.copy()), v), "a feasible nonnegative input was written"
    z = np.zeros_like(v)
    z[::2] = -0.0
    assert l1_exact.same_bits(_P(sipx, op, n, mode, TF, 0.0, 1.0)(z.copy()), z), "zeros with smin = 0 were written"
    # inside after clipping: only the negative entries change, to +0
    w = v.copy()
    for s, idx in enumerate(segs):
        if len(idx) > 1 and s % 2 == 0:
            w[idx[-1]] = -3.0 - s
    y = _P(sipx, op, n, mode, TF, 0.0, 2.0)(w.copy())
    neg = w < 0
    assert neg.any() and l1_exact.same_bits(y[~neg], w[~neg]) and np.all(y[neg] == 0) and not np.any(np.signbit(y[neg]))


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("n,mode", [((33, 3, 4), FZ), ((20, 9, 6), FX), ((12, 10, 5), ("slice", "x"))])
def test_entries_on_the_threshold_come_back_zero(sipx, TF, n, mode):
    """Segments (2, 1, -1, 1, -1, ...): theta = 1 exactly for the probability simplex, the projection is (1, 0, 0, ...); and (-2, -4, ...)
    on the lower side: theta = -3, (1, 0, ...)."""
    segs = _segs("identity", n, mode)
    v = np.zeros(R.rows(n, "identity"), TF)
    want = np.zeros_like(v)
    for s, idx in enumerate(segs):
        if s % 2 == 0:
            v[idx] = np.where(np.arange(len(idx)) % 2 == 1, 1.0, -1.0)
            v[idx[0]] = 2.0
        else:
            v[idx] = -4.0
            v[idx[0]] = -2.0
        want[idx[0]] = 1.0
    assert l1_exact.same_bits(_P(sipx, "identity", n, mode, TF, 1.0, 1.0)(v.copy()), want)


# ---- 3. the observer ---------------------------------------------------------------------------------------------------------------------------
OBSERVED = [("identity", (33, 3, 4), FZ), ("identity", (33, 7, 3), FY), ("identity", (20, 9, 6), FX),
            ("identity", (12, 10, 5), ("slice", "z")), ("identity", (5, 3, REG_MAX + 1), FZ)]


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("op,n,mode", OBSERVED)
def test_observed_bounds_leave_the_point_unwritten(sipx, TF, op, n, mode):
    g = _grid(sipx, n)
    v = np.abs(np.random.default_rng(5 + sum(n)).standard_normal(int(np.prod(n)))).astype(TF)
    s = sipx.segment_sums(v, g, op, mode)
    want = R.sums(v, n, op, mode, TF)
    assert s.dtype == TF and s.shape == want.shape
    assert np.all(np.abs(s.astype(np.float64) - want) <= float(np.finfo(TF).eps) * want)
    assert l1_exact.same_bits(_P(sipx, op, n, mode, TF, s.min(), s.max(), g)(v.copy()), v), "v was written although its bounds were observed on it"
    sd = sipx.segment_sums(torch.from_numpy(v).cuda(), g, op, mode)
    assert sd.is_cuda and l1_exact.same_bits(sd.cpu().numpy(), s), "the device form of the observer gives other bits"
    assert l1_exact.same_bits(sipx.segment_sums(v, g, op, mode), s), "two calls differ"
    if len(s) > 1 and s.min() < s.max():
        y = _P(sipx, op, n, mode, TF, s.min(), np.nextafter(s.max(), TF(0)), g)(v.copy())
        assert not l1_exact.same_bits(y, v)


def test_the_observer_sees_the_range_of_the_operator(sipx):
    TF, n = np.float64, (20, 9, 6)
    g = _grid(sipx, n, (3.0, 4.0, 5.0))
    x = np.random.default_rng(3).standard_normal(int(np.prod(n))).astype(TF)
    for op in ("D_z", "D_x"):
        v = sipx.TDOperator(op, g, TF) @ x
        s = sipx.segment_sums(x, g, op, FZ)
        want = R.sums(v, n, op, FZ, TF)
        assert np.all(np.abs(s - want) <= np.finfo(TF).eps * want)


# ---- 4. whole solves against the oracle (rules and tolerances of tests/test_gpu_l1_weighted.py, test_weighted_solve_matches_oracle) ----------
SOLVE_SETS = {"bounds+simplex-id-fz+l1-Dx": (True, [("simplex", "identity", FZ), ("l1", "D_x", None)]),
              "simplex-id-sz+l1-TV": (False, [("simplex", "identity", ("slice", "z")), ("l1", "TV", None)]),
              "bounds+simplex-Dz-fz": (True, [("simplex", "D_z", FZ)]),
              "bounds+simplex-id-fx": (True, [("simplex", "identity", FX)])}
SOLVE_CASES = [("bounds+simplex-id-fz+l1-Dx", (16, 12, 4), (25.0, 25.0, 25.0)), ("simplex-id-sz+l1-TV", (16, 12, 8), (25.0, 25.0, 25.0)),
               ("bounds+simplex-Dz-fz", (16, 12, 8), (25.0, 25.0, 25.0)), ("bounds+simplex-id-fx", (32, 24), (25.0, 6.0))]


def _whole(n):
    return ("matrix", "") if len(n) == 2 else ("tensor", "")


def _solve_problem(mod, name, n, h, TF, m, opt_kw):
    """The sets of SOLVE_SETS[name] for module `mod`; the simplex takes [0.5, 0.8] times the median sum of the positive parts of the
    segments of A m.  The oracle is set up with the l1 ball on the same operator as a placeholder, its projector then replaced by the
    exact reference."""
    g = mod.compgrid(h, n)
    opt = mod.PARSDMM_options(FL=TF, **opt_kw)
    bounds, sets = SOLVE_SETS[name]
    c = [mod.set_definitions("bounds", "identity", 1600.0, 3900.0, _whole(n))] if bounds else []
    swaps = []
    for kind, opn, mode in sets:
        s = np.asarray(O.get_TD_operator(O.compgrid(h, n), opn, TF)[0] @ m, TF)
        if kind == "l1":
            c.append(mod.set_definitions("l1", opn, 0.0, float(TF(0.5 * np.abs(s.astype(np.float64)).sum())), _whole(n)))
            continue
        med = float(np.median(R.sums(s, n, opn, mode, TF).astype(np.float64)))
        lo, hi = TF(0.5 * med), TF(0.8 * med)
        if mod is O:
            swaps.append((len(c), lambda x, lo=lo, hi=hi, opn=opn, mode=mode: _in_place(lambda a: R.project(a, n, opn, mode, lo, hi)[0].astype(TF), x)))
            c.append(mod.set_definitions("l1", opn, 0.0, 1.0, _whole(n)))
        else:
            c.append(mod.set_definitions("simplex", opn, float(lo), float(hi), mode))
    P, A, prop = mod.setup_constraints(c, g, TF)
    if mod is O:
        for i, f in swaps:
            P[i] = f
    A, AtA, l, y = mod.PARSDMM_precompute_distribute(A, prop, g, opt)
    return g, opt, P, A, prop, AtA


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("name,n,h", SOLVE_CASES)
def test_solve_matches_oracle(sipx, TF, name, n, h):
    m = _model(n, TF, seed=1 + len(SOLVE_SETS[name][1]))
    kw = dict(maxit=60)
    go, oo, Po, Ao, propo, AtAo = _solve_problem(O, name, n, h, TF, m, kw)
    gs, os_, Ps, As, props, AtAs = _solve_problem(sipx, name, n, h, TF, m, kw)
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
    print(f"{name} {n} {np.dtype(TF).name}: iterations {len(ls.obj)} / {len(lo.obj)}, separation {sep}, rel diff {err:.3e}")
    if sep is not None or len(ls.obj) != len(lo.obj):
        # after a separation: the oracle again with the engine's rho / gamma history forced on it
        gr, orr, Pr, Ar, propr, AtAr = _solve_problem(O, name, n, h, TF, m, dict(kw, maxit=len(ls.obj)))
        xr, lr, _, _ = O.PARSDMM(m.copy(), AtAr, Ar, propr, Pr, gr, orr, replay=(ls.rho, ls.gamma))
        err_replay = np.linalg.norm(xs.astype(np.float64) - xr) / np.linalg.norm(xr)
        assert err_replay < tol, (name, "replayed", sep, err_replay)
        tol = max(tol, 5e-4)
        assert _julia_max(ls.set_feasibility[-1]) <= max(_julia_max(lo.set_feasibility[-1]), float(os_.feas_tol))
    assert err < tol, (name, sep, err)
    p = len(SOLVE_SETS[name][1]) + int(SOLVE_SETS[name][0]) + 1
    assert ls.r_pri.shape == (len(ls.obj), p) and ls.set_feasibility.shape[1] == p - 1
    assert len(y_s) == p and [len(q) for q in y_s] == [len(q) for q in y_o]
    assert len(ls.obj) > 6, "the solve stopped before anything was compared"


# ---- 5. the device-resident solve, the reset, the statistics -----------------------------------------------------------------------------------
def test_device_form_gives_the_bits_of_the_host_form(sipx):
    TF, (name, n, h) = np.float32, SOLVE_CASES[0]
    m = _model(n, TF, seed=3)
    g, opt, P, A, prop, AtA = _solve_problem(sipx, name, n, h, TF, m, dict(maxit=30))
    args = (AtA, A, prop, P, g, opt)
    sipx.clear_context_cache()
    try:
        xh, logh, lh, yh = sipx.PARSDMM(m.copy(), *args)
        sipx.clear_context_cache()
        xd, logd, ld, yd = sipx.PARSDMM_device(torch.from_numpy(m.copy()).cuda(), *args)
    finally:
        sipx.clear_context_cache()
    assert xd.is_cuda and np.array_equal(xd.cpu().numpy(), xh)
    assert len(ld) == len(lh) and len(yd) == len(yh)
    for a, b in zip(list(ld) + list(yd), list(lh) + list(yh)):
        assert a.is_cuda and np.array_equal(a.cpu().numpy(), b)
    for f in LOG_FIELDS:
        a, b = np.asarray(getattr(logd, f)), np.asarray(getattr(logh, f))
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), f
    assert len(logh.obj) > 1, "the solve stopped before it began: nothing was compared"


def _fresh(sipx, args, m):
    AtA, A, prop, P, g, opt = args
    ctx = sipx.host.build_context(m, AtA, A, prop, P, g, opt)
    try:
        log, _ = ctx.parsdmm(opt)
        x, l, y = ctx.download()
    finally:
        ctx.close()
    return x, l, y, log


def _run(S, m):
    x, log, l, y = S(m)
    return x, l, y, log


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("case,route", [(0, "lane"), (1, "tile")])
def test_reset_gives_the_bits_of_a_new_context_and_the_route_is_reported(sipx, TF, case, route):
    name, n, h = SOLVE_CASES[case]
    m = _model(n, TF, seed=5)
    g, opt, P, A, prop, AtA = _solve_problem(sipx, name, n, h, TF, m, dict(maxit=25))
    args = (AtA, A, prop, P, g, opt)
    want = _fresh(sipx, args, m)
    with sipx.Solver(*args, TF) as S:
        _assert_same(_run(S, m.copy()), want)
        first = S.ctx.kernel_stats_all(-1)["simplex"]
        got = _run(S, m.copy())                      # (a reset of the live context)
        assert got[3].context_reused
        _assert_same(got, want)
        st = S.ctx.kernel_stats_all(-1)["simplex"]
    other = "tile" if route == "lane" else "lane"
    nseg = 16 * 12 if route == "lane" else n[2]
    for s in (first, st):
        assert s["calls"] >= 2 and s[route] == s["calls"] and s[other] == 0 and s["nseg"] == nseg, s
    assert st["calls"] == first["calls"], "the reset did not restart the counters"


# ---- 6. the engine's refusals through raw descriptors ------------------------------------------------------------------------------------------
def _desc(sipx, op, mode=1, dir=2, pmin=1.0, pmax=1.0, lb=None, ub=None, transform=0, component=0):
    d = sipx.host._SetDesc()
    d.op, d.proj, d.pmin, d.pmax, d.mode, d.dir, d.transform, d.component = op, 19, pmin, pmax, mode, dir, transform, component
    d.lb = None if lb is None else lb.ctypes.data_as(C.c_void_p)
    d.ub = None if ub is None else ub.ctypes.data_as(C.c_void_p)
    d.reserved = 0
    return d


def _refused(sipx, ctx, d):
    rc = sipx.lib().sipx_add_set(ctx.h, C.byref(d), None, None, 0)
    assert rc < 0, "the engine took the set"
    return sipx.lib().sipx_last_error().decode()


def test_engine_refusals(sipx):
    TF, H = np.float32, sipx.host
    OPS = H.OPS
    n = (16, 12, 8)
    g = _grid(sipx, n)
    w = np.ones(16 * 12, TF)
    ctx = sipx.Context(g, TF)
    try:
        assert _refused(sipx, ctx, _desc(sipx, OPS["identity"], mode=0)) == H.SIMPLEX_NEEDS_MODE
        for op in ("TV", "TV_xy"):
            assert _refused(sipx, ctx, _desc(sipx, OPS[op])) == H.SIMPLEX_ONE_BLOCK
        for tr in (1, 2):
            assert _refused(sipx, ctx, _desc(sipx, OPS["identity"], transform=tr)) == H.SIMPLEX_NO_TRANSFORM
        assert _refused(sipx, ctx, _desc(sipx, OPS["D_z"], component=1)) == H.SIMPLEX_NO_MINKOWSKI
        for kw in (dict(lb=w), dict(ub=w), dict(lb=w, ub=w)):
            assert _refused(sipx, ctx, _desc(sipx, OPS["identity"], **kw)) == H.SIMPLEX_NO_VECTORS
        for lo, hi in ((-0.5, 1.0), (2.0, 1.0), (0.0, 0.0), (0.0, float("inf")), (float("nan"), 1.0), (0.0, float("nan")), (0.0, 1e-60)):
            assert _refused(sipx, ctx, _desc(sipx, OPS["identity"], pmin=lo, pmax=hi)) == H.SIMPLEX_BAD_BOUNDS, (lo, hi)
        d = _desc(sipx, OPS["D_z"])
        d.proj = 99
        assert _refused(sipx, ctx, d) == "unknown projector kind"
        # what the engine takes; it holds no replaceable vectors
        assert sipx.lib().sipx_add_set(ctx.h, C.byref(_desc(sipx, OPS["D_z"])), None, None, 0) == 0
        assert sipx.lib().sipx_add_set(ctx.h, C.byref(_desc(sipx, OPS["identity"], mode=2, pmin=0.0)), None, None, 0) == 1
        assert sipx.lib().sipx_set_data(ctx.h, 0, w.ctypes.data_as(C.c_void_p), None) != 0
        assert "holds no replaceable vectors" in sipx.lib().sipx_last_error().decode()
    finally:
        ctx.close()
    ctx = sipx.Context(_grid(sipx, (16, 12)), TF)
    try:
        assert _refused(sipx, ctx, _desc(sipx, OPS["identity"], mode=2, dir=0)) == H.SIMPLEX_2D_SLICE
    finally:
        ctx.close()
    # a slab-decomposed or owned context
    msg = "the simplex set (simplex) takes single-process contexts only"
    ctx = sipx.Context(g, TF)
    try:
        ctx.set_decomp("slab")
        assert msg in _refused(sipx, ctx, _desc(sipx, OPS["D_z"]))
    finally:
        ctx.close()
    for shard in (lambda c: c.set_decomp("slab"), lambda c: c.set_owned([1, 1])):
        ctx = sipx.Context(g, TF)
        try:
            ctx.add_set(sipx.TDOperator("D_z", g, TF), _P(sipx, "D_z", n, FZ, TF, 1.0, 1.0))
            shard(ctx)
            with pytest.raises(sipx.SipxError, match=r"\(simplex\) takes single-process contexts only"):
                ctx.finalize(np.ones(16 * 12 * 8, TF), [10.0], 1.0)
        finally:
            ctx.close()
    # the stand-alone calls refuse what the set refuses
    ctx = sipx.Context(g, TF)
    try:
        out, x = np.zeros(16 * 12, TF), np.zeros(16 * 12 * 8, TF)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        cnt = C.c_int64()
        assert sipx.lib().sipx_segment_sums(ctx.h, OPS["TV"], 1, 2, p(x), p(out), C.byref(cnt)) != 0
        assert sipx.lib().sipx_last_error().decode() == H.SIMPLEX_ONE_BLOCK
        assert sipx.lib().sipx_segment_sums(ctx.h, OPS["D_z"], 0, 0, p(x), p(out), C.byref(cnt)) != 0
        assert sipx.lib().sipx_last_error().decode() == H.SIMPLEX_NEEDS_MODE
        assert sipx.lib().sipx_segment_sums(ctx.h, OPS["D_z"], 1, 2, None, None, C.byref(cnt)) == 0 and cnt.value == 16 * 12
        assert sipx.lib().sipx_segment_sums(ctx.h, OPS["D_z"], 1, 2, p(x), p(out), C.byref(cnt)) == 0 and not out.any()
        v = np.ones(16 * 12 * 7, TF)
        assert sipx.lib().sipx_project(ctx.h, C.byref(_desc(sipx, OPS["D_z"])), p(v), C.c_int64(len(v) - 1)) != 0
        assert f"{len(v)} entries on this grid, {len(v) - 1} given" in sipx.lib().sipx_last_error().decode()
        assert sipx.lib().sipx_project(ctx.h, C.byref(_desc(sipx, OPS["TV"])), p(v), C.c_int64(len(v))) != 0
        assert sipx.lib().sipx_last_error().decode() == H.SIMPLEX_ONE_BLOCK
        assert sipx.lib().sipx_project(ctx.h, C.byref(_desc(sipx, OPS["D_z"])), p(v), C.c_int64(len(v))) == 0
        assert np.allclose(v.reshape(7, 16 * 12).sum(axis=0), 1.0, rtol=1e-6)
        assert ctx.kernel_stats_all(-1)["simplex"] == {"calls": 1, "lane": 1, "tile": 0, "nseg": 16 * 12}
    finally:
        ctx.close()
