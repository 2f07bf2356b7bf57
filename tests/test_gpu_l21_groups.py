"""The l2,1 ball over fibers or slices on the GPU (csrc/l21_groups.h, csrc/ext_group.hip: GroupsProj) through sipx.Projector against
tests/l21_groups_ref.py: accuracy with mixed segment classes, all groups active (where a capped l1 search leaves the ball), groups on the
threshold, inputs and segments it must not write, the observed norm, the bit identities, whole solves against the oracle with its
projector swapped for the reference, the device-resident solve, replaced weights in a live Solver and the engine's refusals.

CASES.  The geometry list of tests/test_gpu_seg_norms.py on the identity -- tests/test_l21_groups_cpu.py proves from the header's own plan
that the fiber cases reach the four paths of seg_norm_plan and a ragged last tile, and that (96,96,10) slice z, (10,96,96) slice x and
(96,10,96) slice y have two or more chunks per slice with a ragged last one (L = 9216 against chunks of 5120 / 2560 entries, 320 / 160 in
the tiles of slice x) -- then difference operators along and across the segments, L = 1, (32,12,8): the 16-byte path, its slices in
one chunk, and (8200,3) fiber x: none of the listed fibers is too long for seg_norm_plan's LDS budget, this one is."""
import ctypes as C

import numpy as np
import pytest
import torch      # (before libsipx.so is loaded: one HIP runtime in the process)

from oracle import parsdmm_oracle as O
from tests import l1_exact
from tests import l21_groups_ref as G
from tests import l21_weighted_ref as R
from tests.test_gpu_l21_frames import LOG_FIELDS, _in_place, _julia_max, _model
from tests.test_gpu_set_data import _assert_same

pytestmark = pytest.mark.gpu

IDENTITY_CASES = [((33, 6, 5), ("fiber", "x")), ((300, 4, 3), ("fiber", "x")), ((5, 7, 33), ("fiber", "y")), ((5, 7, 33), ("fiber", "z")),
                  ((70, 3, 300), ("fiber", "z")), ((96, 96, 10), ("slice", "z")), ((10, 96, 96), ("slice", "x")),
                  ((96, 10, 96), ("slice", "y")), ((40, 28), ("fiber", "x")), ((40, 28), ("fiber", "z")), ((4, 5, 2), ("fiber", "z"))]
CASES = [("identity", n, mode) for n, mode in IDENTITY_CASES] + [
    ("D_z", (5, 7, 33), ("fiber", "z")),       # the difference runs along the fiber: L = 32
    ("D_x", (5, 7, 33), ("fiber", "z")),       # ... across it
    ("D_z", (96, 96, 10), ("slice", "z")),
    ("D_x", (40, 28), ("fiber", "x")),
    ("D_z", (4, 5, 2), ("fiber", "z")),        # L = 1: the l1 ball
    ("identity", (32, 12, 8), ("fiber", "z")), ("identity", (32, 12, 8), ("slice", "z")),      # n1 % 4 == 0: 16 bytes per thread
    ("identity", (8200, 3), ("fiber", "x"))]   # a fiber longer than seg_norm_plan keeps in LDS: its fourth path (segment / streaming)
PRECISIONS = [np.float32, np.float64]
_cache = {}


def _grid(sipx, n, h=None):
    return sipx.compgrid(tuple(1.0 for _ in n) if h is None else h, n)


def _P(sipx, op, n, mode, TF, tau, w=None, g=None):
    return sipx.Projector(sipx.set_definitions("l21_groups", op, 0.0, float(tau), mode, weights=w), g or _grid(sipx, n), TF)


def _segs(op, n, mode):
    key = ("s", op, n, mode)
    if key not in _cache:
        _cache[key] = G.segments(n, op, mode)
    return _cache[key]


def _input(op, n, mode, TF):
    """Segment s is heavy (s % 4 == 0), light (1), all zero with -0.0 entries (2) or plain (3); computed once, handed out as a copy."""
    key = ("v", op, n, mode, np.dtype(TF).name)
    if key not in _cache:
        rng = np.random.default_rng(20261020 + sum(n) + len(op))
        v = np.zeros(G.rows(n, op), TF)
        for s, idx in enumerate(_segs(op, n, mode)):
            x = rng.standard_normal(len(idx))
            if s % 4 == 0:
                v[idx] = 30.0 * x * np.exp(rng.standard_normal(len(idx)))
            elif s % 4 == 1:
                v[idx] = 1e-3 * x
            elif s % 4 == 2:
                v[idx[::2]] = -0.0
            else:
                v[idx] = x
        _cache[key] = v
    return _cache[key].copy()


def _weights(op, n, mode, TF, which=1):
    """Edge-type weights 1 / (1 + |heavy-tailed|) with a tenth set to 0 (segment 3, a plain one, among them)."""
    key = ("w", op, n, mode, np.dtype(TF).name, which)
    if key not in _cache:
        ns = len(_segs(op, n, mode))
        rng = np.random.default_rng(100 * which + 7 + sum(n))
        w = which / (1.0 + np.abs(rng.standard_normal(ns) * np.exp(rng.standard_normal(ns))))
        w[rng.random(ns) < 0.1] = 0.0
        if ns > 3:
            w[3] = 0.0
        _cache[key] = w.astype(TF)
        _cache[key].setflags(write=False)
    return _cache[key]


def _check(y, ref, v, TF, what):
    eps = float(np.finfo(TF).eps)
    av = np.abs(v.astype(np.float64))
    err = np.abs(y.astype(np.float64) - ref)
    worst = float(np.max(err / np.maximum(av, np.finfo(np.float64).tiny)) / eps)
    print(f"l21_groups {what} {np.dtype(TF).name}: worst error {worst:.3f} eps |v|")
    assert np.all(err <= 5 * eps * av), f"{what}: worst error {worst:.3f} eps |v|"


# ---- 1. the projector against the reference (and 6: two calls, no weights = ones; 4: weight-0 segments beside scaled neighbours) ----------
@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("op,n,mode", CASES)
def test_projector_matches_the_reference(sipx, TF, weighted, op, n, mode):
    v = _input(op, n, mode, TF)
    w = _weights(op, n, mode, TF) if weighted else None
    full = G.norm(v, n, op, mode, w)
    for frac in (0.5, 0.05):
        b = TF(frac * full)
        ref = G.project(v, n, op, mode, w, b)
        assert ref is not v
        P = _P(sipx, op, n, mode, TF, b, w)
        y = P(v.copy())
        _check(y, ref, v, TF, f"{op} {n} {mode} weights {weighted} frac {frac}")
        assert l1_exact.same_bits(P(v.copy()), y), "two calls differ"
        if not weighted:
            yo = _P(sipx, op, n, mode, TF, b, G.ones(n, op, mode, TF))(v.copy())
            assert l1_exact.same_bits(yo, y), "no weights and a vector of ones give different bits"
        else:
            segs = _segs(op, n, mode)
            zero = [s for s in range(len(segs)) if w[s] == 0]
            if zero:
                idx = np.concatenate([segs[s] for s in zero])
                assert l1_exact.same_bits(y[idx], v[idx]), "a segment of weight 0 was written"
                rest = np.setdiff1d(np.arange(len(v)), idx)
                assert np.any(y[rest] != v[rest])


# ---- 2. all groups active: the case the capped l1 search gets wrong -------------------------------------------------------------------------
@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("op,n,mode", [("identity", (5, 7, 33), ("fiber", "z")), ("identity", (96, 96, 10), ("slice", "z")),
                                       ("identity", (40, 28), ("fiber", "x")), ("D_z", (5, 7, 33), ("fiber", "z")),
                                       ("identity", (10, 96, 96), ("slice", "x"))])
def test_all_groups_active(sipx, TF, op, n, mode):
    rng = np.random.default_rng(3 + sum(n))
    c = 7.0
    v = rng.standard_normal(G.rows(n, op))
    segs = _segs(op, n, mode)
    for idx in segs:
        v[idx] *= c * rng.uniform(1.0, 1.2) / np.linalg.norm(v[idx])
    v = v.astype(TF)
    g = G.norms(v, n, op, mode, TF)
    assert np.all((g >= 0.999 * c) & (g <= 1.201 * c))
    tau = TF(0.5 * G.norm(v, n, op, mode))
    theta = R.exact_theta(g, np.ones(len(g), TF), tau)
    assert 0 < theta < g.min(), "not every group is active"
    y = _P(sipx, op, n, mode, TF, tau)(v.copy())
    _check(y, G.project(v, n, op, mode, None, tau), v, TF, f"all active {op} {n} {mode}")
    eps = float(np.finfo(TF).eps)
    assert abs(G.norm(y, n, op, mode) - float(tau)) <= 4 * eps * float(tau), (G.norm(y, n, op, mode), float(tau))
    if op == "identity":
        seen = sipx.l21_groups_norm(y, _grid(sipx, n), op, mode)
        assert abs(float(seen) - float(tau)) <= 4 * eps * float(tau), (float(seen), float(tau))


# ---- 3. groups exactly on the threshold ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("n,mode", [((5, 7, 33), ("fiber", "z")), ((96, 96, 10), ("slice", "z")), ((10, 96, 96), ("slice", "x"))])
def test_groups_on_the_threshold_are_zeroed(sipx, TF, n, mode):
    """(g, w) cycles through (5, 2) and (7, 1), active; (1, 1) and (2, 2), exactly on theta = 1; (0.5, 1), below it."""
    segs = _segs("identity", n, mode)
    kinds = [(5.0, 2.0), (7.0, 1.0), (1.0, 1.0), (2.0, 2.0), (0.5, 1.0)]
    assert len(segs) % 5 == 0 and len(segs[0]) >= 2
    v = np.zeros(G.rows(n, "identity"), TF)
    w = np.ones(len(segs), TF)
    for s, idx in enumerate(segs):
        gs, w[s] = kinds[s % 5]
        if gs == 5.0:
            v[idx[s % len(idx)]], v[idx[(s + 1) % len(idx)]] = 3.0, -4.0
        else:
            v[idx[(3 * s) % len(idx)]] = -gs if s % 2 else gs
    g = G.norms(v, n, "identity", mode, TF)
    assert np.array_equal(g, np.array([kinds[s % 5][0] for s in range(len(segs))], TF))
    k = len(segs) // 5
    tau = TF(k * (2 * 5 + 7) - k * (4 + 1))                  # S - theta C over the active groups, theta = 1
    assert R.exact_theta(g, w, tau) == 1.0
    y = _P(sipx, "identity", n, mode, TF, tau, w)(v.copy())
    for s, idx in enumerate(segs):
        if s % 5 >= 2:
            assert np.all(y[idx] == 0), f"segment {s} of kind {kinds[s % 5]} survived"
        else:
            f = TF(TF(3) / TF(5)) if s % 5 == 0 else TF(TF(6) / TF(7))
            assert l1_exact.same_bits(y[idx], (v[idx] * f).astype(TF)), s


# ---- 4. inputs the projector must not write --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("op,n,mode", [("identity", (5, 7, 33), ("fiber", "y")), ("D_z", (96, 96, 10), ("slice", "z")),
                                       ("D_x", (40, 28), ("fiber", "x")), ("identity", (32, 12, 8), ("slice", "z"))])
def test_feasible_and_zero_inputs_come_back_bit_for_bit(sipx, TF, op, n, mode):
    v, w = _input(op, n, mode, TF), _weights(op, n, mode, TF)
    v[::7] = -0.0
    for ww in (None, w):
        b = TF(2 * G.norm(v, n, op, mode, ww))
        assert np.any(np.signbit(v) & (v == 0))
        assert l1_exact.same_bits(_P(sipx, op, n, mode, TF, b, ww)(v.copy()), v)
        z = np.zeros_like(v)
        z[::2] = -0.0
        assert l1_exact.same_bits(_P(sipx, op, n, mode, TF, b, ww)(z.copy()), z)
    # all weights zero: no radius makes the projector write
    assert l1_exact.same_bits(_P(sipx, op, n, mode, TF, 1e-6, np.zeros(len(w), TF))(v.copy()), v)


# ---- 5. the observed radius ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("op,n,mode", [("identity", (5, 7, 33), ("fiber", "z")), ("D_z", (96, 96, 10), ("slice", "z")),
                                       ("D_x", (40, 28), ("fiber", "x")), ("identity", (10, 96, 96), ("slice", "x")),
                                       ("D_z", (5, 7, 33), ("fiber", "z")), ("identity", (32, 12, 8), ("slice", "z"))])
def test_observed_radius_leaves_the_point_unwritten(sipx, TF, weighted, op, n, mode):
    g = _grid(sipx, n, tuple(3.0 + a for a in range(len(n))))
    x = np.random.default_rng(5 + sum(n)).standard_normal(int(np.prod(n))).astype(TF)
    w = np.array(_weights(op, n, mode, TF)) if weighted else None
    v = sipx.TDOperator(op, g, TF) @ x
    tau = sipx.l21_groups_norm(x, g, op, mode, weights=w)
    assert isinstance(tau, TF)
    ref = G.norm(v, n, op, mode, w)
    assert abs(float(tau) - ref) <= 2 * float(np.finfo(TF).eps) * ref
    assert l1_exact.same_bits(_P(sipx, op, n, mode, TF, tau, w, g)(v.copy()), v), "A x was written although its radius was observed on x"
    td = sipx.l21_groups_norm(torch.from_numpy(x).cuda(), g, op, mode, weights=None if w is None else torch.from_numpy(w).cuda())
    assert td.is_cuda and td.shape == (1,) and l1_exact.same_bits(td.cpu().numpy(), np.array([tau], TF))
    y = _P(sipx, op, n, mode, TF, float(tau) * 0.999, w, g)(v.copy())
    assert not l1_exact.same_bits(y, v)


# ---- 6. the fiber norms are those of segment_norms, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("op,n,mode", [("identity", (70, 3, 300), ("fiber", "z")), ("D_z", (5, 7, 33), ("fiber", "z")),
                                       ("identity", (300, 4, 3), ("fiber", "x")), ("identity", (40, 28), ("fiber", "z"))])
def test_fiber_norms_are_segment_norms_bit_for_bit(sipx, TF, op, n, mode):
    """A one-hot weight vector makes the observed weighted norm the norm of one segment: (T)(1 * g_s) = g_s."""
    g = _grid(sipx, n)
    x = np.random.default_rng(9 + sum(n)).standard_normal(int(np.prod(n))).astype(TF)
    want = sipx.segment_norms(x, g, op, mode, "l2")
    assert len(want) == G.nseg(n, op, mode)
    for s in sorted({0, 1, len(want) // 3, len(want) // 2, len(want) - 1}):
        w = np.zeros(len(want), TF)
        w[s] = 1.0
        got = sipx.l21_groups_norm(x, g, op, mode, weights=w)
        assert l1_exact.same_bits(np.array([got]), want[s:s + 1]), (s, got, want[s])


# ---- 7. whole solves against the oracle (rules and tolerances of tests/test_gpu_l21_weighted.py, test_weighted_solve_matches_oracle) ------------
SOLVE_SETS = {"groups-Dz-fiber": [("D_z", ("fiber", "z"), False)],
              "groups-Dz-slice+l1-Dx": [("D_z", ("slice", "z"), False), ("D_x", None, False)],
              "wgroups-id-fiber": [("identity", ("fiber", "x"), True)]}
SOLVE_CASES = [("groups-Dz-fiber", (16, 12, 8), (25.0, 25.0, 25.0)), ("groups-Dz-slice+l1-Dx", (16, 12, 8), (25.0, 25.0, 25.0)),
               ("wgroups-id-fiber", (32, 24), (25.0, 6.0))]


def _whole(n):
    return ("matrix", "") if len(n) == 2 else ("tensor", "")


def _solve_problem(mod, name, n, h, TF, m, opt_kw, which=1):
    """{bounds, the sets of SOLVE_SETS[name]} for module `mod`; tau = half the norm of A m from the reference.  The oracle is set up with
    the l1 ball on the operator, its projector then replaced by the reference."""
    g = mod.compgrid(h, n)
    opt = mod.PARSDMM_options(FL=TF, **opt_kw)
    c = [mod.set_definitions("bounds", "identity", 1600.0, 3900.0, _whole(n))]
    swaps = []
    for opn, mode, weighted in SOLVE_SETS[name]:
        s = np.asarray(O.get_TD_operator(O.compgrid(h, n), opn, TF)[0] @ m, TF)
        if mode is None:                                   # a plain l1 set
            c.append(mod.set_definitions("l1", opn, 0.0, float(TF(0.5 * np.abs(s.astype(np.float64)).sum())), _whole(n)))
            continue
        w = np.array(_weights(opn, n, mode, TF, which)) if weighted else None
        r = TF(0.5 * G.norm(s, n, opn, mode, np.array(_weights(opn, n, mode, TF, 1)) if weighted else None))
        if mod is O:
            swaps.append((len(c), lambda x, r=r, w=w, opn=opn, mode=mode: _in_place(lambda a: G.project(a, n, opn, mode, w, r), x)))
            c.append(mod.set_definitions("l1", opn, 0.0, float(r), _whole(n)))
        else:
            c.append(mod.set_definitions("l21_groups", opn, 0.0, float(r), mode, weights=w))
    P, A, prop = mod.setup_constraints(c, g, TF)
    if mod is O:
        for i, f in swaps:
            P[i] = f
    A, AtA, l, y = mod.PARSDMM_precompute_distribute(A, prop, g, opt)
    return g, opt, P, A, prop, AtA


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("name,n,h", SOLVE_CASES)
def test_solve_matches_oracle(sipx, TF, name, n, h):
    m = _model(n, TF, seed=1 + len(SOLVE_SETS[name]))
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
    p = len(SOLVE_SETS[name]) + 2
    assert ls.r_pri.shape == (len(ls.obj), p) and ls.set_feasibility.shape[1] == p - 1
    assert len(y_s) == p and [len(q) for q in y_s] == [len(q) for q in y_o]
    assert len(ls.obj) > 6, "the solve stopped before anything was compared"


# ---- 8. the device-resident solve ----------------------------------------------------------------------------------------------------------------
def test_device_form_gives_the_bits_of_the_host_form(sipx):
    TF, (name, n, h) = np.float32, SOLVE_CASES[1]
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


# ---- 9, 10. set_data: new weights in a live Solver ---------------------------------------------------------------------------------------------
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
def test_set_data_then_reset_gives_the_bits_of_a_new_context(sipx, TF):
    """Built with weights 1 and solved; then set_data(weights 2) and the next solve (a reset): x, every l_i, y_i and log array equal a new
    context built with weights 2 (the radius stays that of weights 1: only lb is replaceable).  Host form, then device form."""
    name, n, h = SOLVE_CASES[2]
    opn, mode, _ = SOLVE_SETS[name][0]
    m = _model(n, TF, seed=5)

    def args_of(which):
        g, opt, P, A, prop, AtA = _solve_problem(sipx, name, n, h, TF, m, dict(maxit=25), which)
        return (AtA, A, prop, P, g, opt)
    args1, args2 = args_of(1), args_of(2)
    w2 = np.array(_weights(opn, n, mode, TF, 2))
    assert args2[3][1].pmax == args1[3][1].pmax and np.array_equal(args2[3][1].lb, w2)
    assert args1[3][1].data_len(args1[1][1]) == len(w2) == 24
    want1, want2 = _fresh(sipx, args1, m), _fresh(sipx, args2, m)
    assert not np.array_equal(want1[0], want2[0]), "the two weight vectors give the same solve: nothing is shown"
    with sipx.Solver(*args1, TF) as S:
        _assert_same(_run(S, m.copy()), want1)
        S.set_data(1, lb=w2)
        got = _run(S, m.copy())
        assert got[3].context_reused
        _assert_same(got, want2)
        st = S.ctx.kernel_stats_all(-1)["l21_groups"]
        assert 2 <= st["passes"] <= 25 and st["flag_reads"] == -(-st["passes"] // 8) and st["nseg"] == 24 and st["calls"] >= 2
        with pytest.raises(sipx.SipxError, match="the weights of an l2,1 set are its lb; it has no ub"):
            S.set_data(1, ub=w2)
        wb = w2.copy()
        wb[3] = -1.0
        with pytest.raises(sipx.SipxError, match=r"\(l21_groups\): weight 3 is negative, NaN or infinite"):
            S.set_data(1, lb=wb)
    dev = torch.device("cuda", 0)
    with sipx.Solver(*args1, TF) as S:
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        _assert_same(_run(S, t(m)), want1)
        S.set_data(1, lb=t(w2))
        _assert_same(_run(S, t(m)), want2)


def test_a_set_built_without_weights_refuses_set_data(sipx):
    TF, (name, n, h) = np.float32, SOLVE_CASES[0]
    m = _model(n, TF, seed=2)
    g, opt, P, A, prop, AtA = _solve_problem(sipx, name, n, h, TF, m, dict(maxit=5))
    w = np.ones(16 * 12, TF)
    with sipx.Solver(AtA, A, prop, P, g, opt, TF) as S:
        with pytest.raises(sipx.SipxError, match="holds no replaceable vectors"):
            S.set_data(1, lb=w)
    ctx = sipx.host.build_context(m, AtA, A, prop, P, g, opt)
    try:
        with pytest.raises(sipx.SipxError, match="holds no replaceable vectors"):
            ctx.set_data(1, lb=w)
    finally:
        ctx.close()


# ---- 11. the engine's refusals through raw descriptors ----------------------------------------------------------------------------------------
def _desc(sipx, op, w, mode=1, dir=2, pmax=1.0, count=None, ub=None, transform=0, component=0):
    d = sipx.host._SetDesc()
    d.op, d.proj, d.pmin, d.pmax, d.mode, d.dir, d.transform, d.component = op, 16, 0.0, pmax, mode, dir, transform, component
    d.lb = None if w is None else w.ctypes.data_as(C.c_void_p)
    d.ub = None if ub is None else ub.ctypes.data_as(C.c_void_p)
    d.reserved = (0 if w is None else len(w)) if count is None else count
    return d


def _refused(sipx, ctx, d):
    rc = sipx.lib().sipx_add_set(ctx.h, C.byref(d), None, None, 0)
    assert rc < 0, "the engine took the set"
    return sipx.lib().sipx_last_error().decode()


def test_engine_refusals(sipx):
    TF = np.float32
    OPS = sipx.host.OPS
    n = (16, 12, 8)
    g = _grid(sipx, n)
    w = np.ones(16 * 12, TF)                         # D_z, fiber z: one weight per pixel
    ctx = sipx.Context(g, TF)
    try:
        assert "needs a fiber or slice mode" in _refused(sipx, ctx, _desc(sipx, OPS["D_z"], None, mode=0))
        assert "use the l2 set" in _refused(sipx, ctx, _desc(sipx, OPS["identity"], None, mode=0))
        for op in ("TV", "TV_xy"):
            assert "groups the range of a one-block operator" in _refused(sipx, ctx, _desc(sipx, OPS[op], None))
        for tr in (1, 2):
            assert "(l21_groups) takes no transform" in _refused(sipx, ctx, _desc(sipx, OPS["identity"], None, transform=tr))
        assert "(l21_groups) takes no Minkowski component" in _refused(sipx, ctx, _desc(sipx, OPS["D_z"], None, component=1))
        msg = _refused(sipx, ctx, _desc(sipx, OPS["D_z"], w, count=191))
        assert "(l21_groups): 191 weights given, 192 are needed -- one per segment, a segment being a fiber along dimension 3" in msg
        assert "(16, 12, 7)" in msg
        assert "(l21_groups): 192 weights given, 7 are needed" in _refused(sipx, ctx, _desc(sipx, OPS["D_z"], w, mode=2))
        wb = w.copy()
        wb[7] = -1.0
        assert "the weighted l2,1 ball (l21_groups): weight 7 is negative, NaN or infinite" in _refused(sipx, ctx, _desc(sipx, OPS["D_z"], wb))
        assert "takes weights in lb and no ub" in _refused(sipx, ctx, _desc(sipx, OPS["D_z"], None, ub=w))
        assert _refused(sipx, ctx, _desc(sipx, OPS["D_z"], w, pmax=0.0)) == "Radius of L1 ball is negative"
        assert _refused(sipx, ctx, _desc(sipx, OPS["D_z"], w, pmax=float("nan"))) == "Radius of L1 ball is negative"
        # refusals that have not moved: the l2,1 ball off TV, an unknown projector kind
        d = _desc(sipx, OPS["D_z"], None, mode=0)
        d.proj = 14
        assert _refused(sipx, ctx, d) == "the l2,1 ball acts on the range of the TV operator: TD_OP must be TV (D2D, D3D)"
        d.proj = 99
        assert _refused(sipx, ctx, d) == "unknown projector kind"
        # what the engine takes: weights are replaceable, a set without them is not
        assert sipx.lib().sipx_add_set(ctx.h, C.byref(_desc(sipx, OPS["D_z"], w)), None, None, 0) == 0
        assert sipx.lib().sipx_add_set(ctx.h, C.byref(_desc(sipx, OPS["D_z"], None, mode=2)), None, None, 0) == 1
        assert sipx.lib().sipx_set_data(ctx.h, 0, w.ctypes.data_as(C.c_void_p), None) == 0
        assert sipx.lib().sipx_set_data(ctx.h, 0, None, w.ctypes.data_as(C.c_void_p)) != 0
        assert "the weights of an l2,1 set are its lb; it has no ub" in sipx.lib().sipx_last_error().decode()
        assert sipx.lib().sipx_set_data(ctx.h, 1, w.ctypes.data_as(C.c_void_p), None) != 0
        assert "holds no replaceable vectors" in sipx.lib().sipx_last_error().decode()
    finally:
        ctx.close()
    g2 = _grid(sipx, (16, 12))
    ctx = sipx.Context(g2, TF)
    try:
        assert "for 2D models, the mode of application for l21_groups sets" in _refused(sipx, ctx, _desc(sipx, OPS["identity"], None, mode=2, dir=0))
    finally:
        ctx.close()
    # a slab-decomposed or owned context
    msg = "(l21_groups) takes single-process contexts only"
    ctx = sipx.Context(g, TF)
    try:
        ctx.set_decomp("slab")
        assert msg in _refused(sipx, ctx, _desc(sipx, OPS["D_z"], None))
    finally:
        ctx.close()
    for shard in (lambda c: c.set_decomp("slab"), lambda c: c.set_owned([1, 1])):
        ctx = sipx.Context(g, TF)
        try:
            ctx.add_set(sipx.TDOperator("D_z", g, TF), _P(sipx, "D_z", n, ("fiber", "z"), TF, 1.0))
            shard(ctx)
            with pytest.raises(sipx.SipxError, match=r"\(l21_groups\) takes single-process contexts only"):
                ctx.finalize(np.ones(16 * 12 * 8, TF), [10.0], 1.0)
        finally:
            ctx.close()
    # the stand-alone observer refuses what the set refuses
    ctx = sipx.Context(g, TF)
    try:
        out, x = np.zeros(1, TF), np.zeros(16 * 12 * 8, TF)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert sipx.lib().sipx_l21_groups_norm(ctx.h, OPS["TV"], 1, 2, p(x), None, p(out)) != 0
        assert "one-block operator" in sipx.lib().sipx_last_error().decode()
        assert sipx.lib().sipx_l21_groups_norm(ctx.h, OPS["D_z"], 0, 0, p(x), None, p(out)) != 0
        assert "needs a fiber or slice mode" in sipx.lib().sipx_last_error().decode()
        wb = w.copy()
        wb[4] = np.nan
        assert sipx.lib().sipx_l21_groups_norm(ctx.h, OPS["D_z"], 1, 2, p(x), p(wb), p(out)) != 0
        assert "weight 4 is negative, NaN or infinite" in sipx.lib().sipx_last_error().decode()
        assert sipx.lib().sipx_l21_groups_norm(ctx.h, OPS["D_z"], 1, 2, p(x), None, p(out)) == 0 and out[0] == 0
    finally:
        ctx.close()
