"""The weighted l2,1 ball on the GPU (csrc/l21_weighted.h, csrc/ext_group.hip: BallProj's weighted route) through sipx.Projector
against tests/l21_weighted_ref.py: accuracy, inputs and groups it must not write, exact ties, the observed weighted norm, whole solves
against the oracle with its projector swapped for the reference, replaced weights in a live Solver, the device-resident solve and the
engine's refusals through the C ABI.

GRIDS.  ("TV", n): (4,3) and (5,4,3) are the smallest with every boundary class; (33,20) and (20,9,6) have an odd n1 (one entry per
thread); (64,48) and (32,12,8) have n1 % 4 == 0 (16 bytes per thread).  The pass kernel k_l21w_part launches min(ceil(entries / (256 VW
L21W_LOADS)), L21W_GRID = 1024) workgroups of 256 threads, every thread taking L21W_LOADS = 4 loads of VW entries per round: one round
of the full grid covers 1024 * 256 * 4 = 1 048 576 entries on the one-entry path.  (1025, 1027) has 1 052 675 groups: every thread takes
one unrolled round, and the first 4 099 threads a second, partial one through the tail loop.  ("joint", n): (5,4,3), (32,12,8), and
(4,3,16), the smallest grid at which l21_joint_plan cuts the z range (n3 / 8 = 2 chunks of 8 frames).  ("TV_xy", n): the whole-array
set on the in-plane gradient, both paths."""
import ctypes as C

import numpy as np
import pytest
import torch      # (before libsipx.so is loaded: one HIP runtime in the process)

from oracle import parsdmm_oracle as O
from tests import l1_exact, l21_joint_ref, l21_ref
from tests import l21_weighted_ref as R
from tests.test_gpu_l21_frames import LOG_FIELDS, _in_place, _julia_max, _model, _stacked
from tests.test_gpu_set_data import _assert_same
from tests.test_l21_weighted_cpu import FAMILIES, weights

pytestmark = pytest.mark.gpu

LARGE = (1025, 1027)
CASES = [("TV", n) for n in [(4, 3), (5, 4, 3), (33, 20), (20, 9, 6), (64, 48), (32, 12, 8), LARGE]] + \
        [("joint", n) for n in [(5, 4, 3), (32, 12, 8), (4, 3, 16)]] + [("TV_xy", n) for n in [(5, 4, 3), (32, 12, 8)]]
FRACS = [0.9, 0.5, 0.05]
PRECISIONS = [np.float32, np.float64]
SET = {"TV": ("l21", "TV"), "TV_xy": ("l21", "TV_xy"), "joint": ("l21_joint", "TV_xy")}
_cache = {}


def _grid(sipx, n, h=None):
    return sipx.compgrid(tuple(1.0 for _ in n) if h is None else h, n)


def _mode(n):
    return ("matrix", "") if len(n) == 2 else ("tensor", "")


def _P(sipx, kind, n, TF, tau, w, g=None):
    st, op = SET[kind]
    return sipx.Projector(sipx.set_definitions(st, op, 0.0, float(tau), _mode(n), weights=w), g or _grid(sipx, n), TF)


def _input(kind, n, TF):
    """Heavy-tailed randn * exp(randn) on every row of the M-vector; computed once, handed out as a copy."""
    key = ("v", kind, n, np.dtype(TF).name)
    if key not in _cache:
        rng = np.random.default_rng(20251020 + sum(n))
        M = R.rows(n, kind)
        _cache[key] = (rng.standard_normal(M) * np.exp(rng.standard_normal(M))).astype(TF)
    return _cache[key].copy()


def _weights(kind, n, family, TF):
    key = ("w", kind, n, family, np.dtype(TF).name)
    if key not in _cache:
        _cache[key] = weights(family, np.random.default_rng(7 + sum(n) + len(family)), R.ngroups(n, kind), TF)
        _cache[key].setflags(write=False)
    return _cache[key]


def test_the_large_grid_needs_a_second_round():
    N = int(np.prod(LARGE))
    assert LARGE[0] % 4 != 0 and 1024 * 256 * 4 < N < 1024 * 256 * 5 and 640 * 520 < 1024 * 256 * 4
    assert l21_joint_ref.plan(12, 16, 4)[0] == 2 and l21_joint_ref.plan(12, 15, 4)[0] == 1 and l21_joint_ref.plan(12, 16, 8)[0] == 2


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("frac", FRACS)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("kind,n", CASES)
def test_projector_matches_the_reference(sipx, TF, frac, family, kind, n):
    v, w = _input(kind, n, TF), _weights(kind, n, family, TF)
    b = TF(frac * R.norm(v, n, kind, w))
    ref = R.project(v, n, kind, w, b)
    assert ref is not v
    P = _P(sipx, kind, n, TF, b, w)
    y = P(v.copy())
    eps = float(np.finfo(TF).eps)
    av = np.abs(v.astype(np.float64))
    err = np.abs(y.astype(np.float64) - ref)
    worst = float(np.max(err / np.maximum(av, np.finfo(np.float64).tiny)) / eps)
    print(f"l21 weighted {kind} {n} {np.dtype(TF).name} {family} frac {frac}: worst error {worst:.3f} eps |v|")
    assert np.all(err <= 5 * eps * av), f"worst error {worst:.3f} eps |v|"
    assert l1_exact.same_bits(P(v.copy()), y), "two calls differ"
    if family == "ones" and kind != "TV_xy":      # all ones: the unweighted set's reference, at the same bound
        plain = l21_ref.project(v, n, b) if kind == "TV" else l21_joint_ref.project(v, n, b)
        assert plain is not v and np.all(np.abs(y.astype(np.float64) - plain) <= 5 * eps * av)
    if family == "masked":                        # groups of weight 0 come back bit for bit while their neighbours are shrunk
        G = R.members(n, kind)
        idx = G[np.asarray(w) == 0]
        idx = idx[idx >= 0]
        assert len(idx) and l1_exact.same_bits(y[idx], v[idx])
        rest = np.setdiff1d(np.arange(len(v)), idx)
        assert np.any(y[rest] != v[rest])


# ---- inputs the projector must not write -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("kind,n", [("TV", (33, 20)), ("TV", (32, 12, 8)), ("joint", (4, 3, 16)), ("TV_xy", (32, 12, 8))])
def test_feasible_and_zero_inputs_come_back_bit_for_bit(sipx, TF, kind, n):
    v, w = _input(kind, n, TF), _weights(kind, n, "edge", TF)
    v[::7] = -0.0
    v[3::11] = 0.0
    b = TF(2 * R.norm(v, n, kind, w))
    assert R.feasibility(R.norms(v, n, kind, TF), w, b) > 0 and np.any(np.signbit(v) & (v == 0))
    assert l1_exact.same_bits(_P(sipx, kind, n, TF, b, w)(v.copy()), v)
    z = np.zeros_like(v)
    z[::2] = -0.0
    assert l1_exact.same_bits(_P(sipx, kind, n, TF, b, w)(z.copy()), z)
    # all weights zero: no radius makes the projector write
    v = _input(kind, n, TF)
    assert l1_exact.same_bits(_P(sipx, kind, n, TF, 1e-6, np.zeros(R.ngroups(n, kind), TF))(v.copy()), v)


# ---- ties: integer components and power-of-two weights, exact in both precisions ------------------------------------------------------------
def _tie_input(n, TF):
    """Groups (g, w): three (7, 2), two (7, 1), nine or ten (5, 2) that sit exactly on theta = 2.5, the rest (1, 1) or empty."""
    G = l21_ref.groups(n)
    full = np.nonzero((G >= 0).all(axis=1))[0]
    pick = np.random.default_rng(41).permutation(full)
    nd = len(n)
    sevens = [(7, 0), (0, 7), (7, 0), (0, -7), (7, 0)] if nd == 2 else [(7, 0, 0), (0, 7, 0), (0, 0, 7), (0, -7, 0), (-7, 0, 0)]
    fives = [(3, 4), (5, 0), (4, -3), (0, 5), (-3, 4), (-5, 0), (4, 3), (0, -5), (3, -4)] if nd == 2 else \
            [(3, 4, 0), (5, 0, 0), (0, 3, 4), (0, 0, -5), (-3, 0, 4), (0, 5, 0), (0, -3, 4), (4, 3, 0), (0, 4, -3), (-4, 0, 3)]
    v = np.zeros(l21_ref.rows(n), TF)
    w = np.ones(G.shape[0], TF)
    kind = np.ones(G.shape[0], int)
    for p in range(G.shape[0]):
        mem = G[p][G[p] >= 0]
        if len(mem):
            v[mem[p % len(mem)]] = -1.0 if p % 3 == 0 else 1.0
        else:
            kind[p] = 0
    for k, (p, comp) in enumerate(zip(pick, sevens + fives)):
        v[G[p]] = comp
        kind[p] = (72 if k < 3 else 71) if k < 5 else 52
        w[p] = 1.0 if kind[p] == 71 else 2.0
    return v, w, G, kind


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("n", [(9, 7), (8, 6, 5)])
def test_groups_on_the_threshold_are_zeroed(sipx, TF, n):
    v, w, G, kind = _tie_input(n, TF)
    g = l21_ref.norms(v, n, TF)
    assert np.array_equal(g, np.where(kind > 9, kind // 10, kind).astype(TF))
    b = TF(3 * 4 + 2 * 4.5)                       # S - 2.5 C over the active groups: 3 (14 - 10) + 2 (7 - 2.5)
    assert R.exact_theta(g, w, b) == 2.5
    y = _P(sipx, "TV", n, TF, b, w)(v.copy())
    for k in (52, 1):
        mem = G[kind == k]
        assert np.all(y[mem[mem >= 0]] == 0), f"a group of kind {k} survived"
    eps = float(np.finfo(TF).eps)
    for k, f in ((72, 2.0 / 7.0), (71, 4.5 / 7.0)):
        mem = G[kind == k]
        mem = mem[mem >= 0]
        assert np.all(np.abs(y[mem] - v[mem].astype(np.float64) * f) <= 4 * eps * np.abs(v[mem]))
    assert np.count_nonzero(y) == 5


# ---- the observed weighted norm ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("kind,n", [("TV", (33, 20)), ("TV", (64, 48)), ("TV", (20, 9, 6)), ("TV", (32, 12, 8)), ("TV_xy", (32, 12, 8)),
                                    ("joint", (5, 4, 3)), ("joint", (4, 3, 16))])
def test_observed_radius_leaves_the_point_unwritten(sipx, TF, kind, n):
    g = _grid(sipx, n, tuple(3.0 + a for a in range(len(n))))
    st, op = SET[kind]
    x = np.random.default_rng(5 + sum(n)).standard_normal(int(np.prod(n))).astype(TF)
    w = _weights(kind, n, "lognormal", TF)
    v = sipx.TDOperator(op, g, TF) @ x
    observe = (lambda a, ww: sipx.l21_joint_norm(a, g, weights=ww)) if kind == "joint" else (lambda a, ww: sipx.l21_norm(a, g, op, weights=ww))
    tau = observe(x, w)
    assert isinstance(tau, TF)
    ref = R.norm(v, n, kind, w)
    assert abs(float(tau) - ref) <= 2 * float(np.finfo(TF).eps) * ref
    assert l1_exact.same_bits(_P(sipx, kind, n, TF, tau, w, g)(v.copy()), v), "A x was written although its radius was observed on x"
    td = observe(torch.from_numpy(x).cuda(), torch.from_numpy(np.array(w)).cuda())
    assert td.is_cuda and td.shape == (1,) and l1_exact.same_bits(td.cpu().numpy(), np.array([tau], TF))
    y = _P(sipx, kind, n, TF, float(tau) * 0.999, w, g)(v.copy())
    assert not l1_exact.same_bits(y, v)


# ---- whole solves against the oracle (rules and tolerances of tests/test_gpu_l21.py, test_l21_solve_matches_oracle) -----------------------------
SOLVE_SETS = {"wl21-TV": [("TV", "l21", "TV")], "wl21-TV+l1-Dz": [("TV", "l21", "TV"), (None, "l1", "D_z")],
              "wl21-joint": [("joint", "l21_joint", "TV_xy")]}
SOLVE_CASES = [(name, n, h) for name in ("wl21-TV", "wl21-TV+l1-Dz") for n, h in (((32, 24), (25.0, 6.0)), ((16, 12, 8), (25.0, 25.0, 25.0)))] + \
              [("wl21-joint", (16, 12, 8), (25.0, 25.0, 25.0))]


def _solve_weights(kind, n, TF, which=1):
    """Edge-type weights with a tenth of the groups masked; `which` picks one of two vectors (set_data)."""
    rng = np.random.default_rng(100 * which + sum(n))
    w = weights("edge", rng, R.ngroups(n, kind), np.float64) * which
    w[rng.random(len(w)) < 0.1] = 0.0
    return w.astype(TF)


def _solve_problem(mod, name, n, h, TF, m, opt_kw, which=1):
    """{bounds, the sets of SOLVE_SETS[name]} for module `mod`; tau = half the (weighted) norm of A m from the reference.  The oracle is
    set up with the l1 ball on the operator (TV_xy: its own D_y and D_x stacked, as a custom operator), its projector then replaced by
    the reference."""
    g = mod.compgrid(h, n)
    opt = mod.PARSDMM_options(FL=TF, **opt_kw)
    c = [mod.set_definitions("bounds", "identity", 1600.0, 3900.0, _mode(n))]
    swaps = []
    for kind, st, opn in SOLVE_SETS[name]:
        A = _stacked(n, h, TF) if opn == "TV_xy" else O.get_TD_operator(O.compgrid(h, n), opn, TF)[0]
        s = np.asarray(A @ m, TF)
        if kind:
            w = _solve_weights(kind, n, TF, which)
            r = TF(0.5 * R.norm(s, n, kind, w))
            swaps.append((len(c), lambda x, r=r, w=w, kind=kind: _in_place(lambda a, nn, rr: R.project(a, nn, kind, w, rr), x, n, r)))
        else:
            w = None
            r = TF(0.5 * np.abs(s.astype(np.float64)).sum())
        if mod is O:
            c.append(mod.set_definitions("l1", "identity" if opn == "TV_xy" else opn, 0.0, float(r), _mode(n),
                                         (A, False) if opn == "TV_xy" else ((), False)))
        elif w is None:
            c.append(mod.set_definitions(st, opn, 0.0, float(r), _mode(n)))
        else:
            c.append(mod.set_definitions(st, opn, 0.0, float(r), _mode(n), weights=w))
    P, A, prop = mod.setup_constraints(c, g, TF)
    if mod is O:
        for i, f in swaps:
            P[i] = f
    A, AtA, l, y = mod.PARSDMM_precompute_distribute(A, prop, g, opt)
    return g, opt, P, A, prop, AtA


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("name,n,h", SOLVE_CASES)
def test_weighted_solve_matches_oracle(sipx, TF, name, n, h):
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


# ---- the device-resident solve ---------------------------------------------------------------------------------------------------------------
def test_device_form_gives_the_bits_of_the_host_form(sipx):
    TF, n, h = np.float32, (32, 24), (25.0, 6.0)
    m = _model(n, TF, seed=3)
    g, opt, P, A, prop, AtA = _solve_problem(sipx, "wl21-TV+l1-Dz", n, h, TF, m, dict(maxit=30))
    args = (AtA, A, prop, P, g, opt)
    xh, logh, lh, yh = sipx.PARSDMM(m.copy(), *args)
    assert not logh.context_reused
    xd, logd, ld, yd = sipx.PARSDMM_device(torch.from_numpy(m.copy()).cuda(), *args)
    assert not logd.context_reused, "a weighted list is not cached"
    assert xd.is_cuda and np.array_equal(xd.cpu().numpy(), xh)
    assert len(ld) == len(lh) and len(yd) == len(yh)
    for a, b in zip(list(ld) + list(yd), list(lh) + list(yh)):
        assert a.is_cuda and np.array_equal(a.cpu().numpy(), b)
    for f in LOG_FIELDS:
        a, b = np.asarray(getattr(logd, f)), np.asarray(getattr(logh, f))
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), f
    assert len(logh.obj) > 1, "the solve stopped before it began: nothing was compared"


# ---- set_data: new weights in a live Solver --------------------------------------------------------------------------------------------------
def _fresh(sipx, args, m):
    """x, l, y and the log of a newly built context."""
    AtA, A, prop, P, g, opt = args
    ctx = sipx.host.build_context(m, AtA, A, prop, P, g, opt)
    try:
        log, _ = ctx.parsdmm(opt)
        x, l, y = ctx.download()
    finally:
        ctx.close()
    return x, l, y, log


def _run(S, m):
    """A Solver call in the order _assert_same takes."""
    x, log, l, y = S(m)
    return x, l, y, log


def _args(sipx, name, n, h, TF, m, which):
    g, opt, P, A, prop, AtA = _solve_problem(sipx, name, n, h, TF, m, dict(maxit=25), which)
    return (AtA, A, prop, P, g, opt)


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("name,n,h", [("wl21-TV+l1-Dz", (32, 24), (25.0, 6.0)), ("wl21-joint", (16, 12, 8), (25.0, 25.0, 25.0))])
def test_set_data_then_reset_gives_the_bits_of_a_new_context(sipx, TF, name, n, h):
    """Built with weights 1 and solved; then set_data(weights 2), the next solve (a reset): x, every l_i, y_i and log array equal a new
    context built with weights 2 (the radius stays the one of weights 1: only lb is replaceable).  Host form, then device form."""
    m = _model(n, TF, seed=5)
    args1 = _args(sipx, name, n, h, TF, m, 1)
    kind = SOLVE_SETS[name][0][0]
    w2 = _solve_weights(kind, n, TF, 2)
    args2 = _args(sipx, name, n, h, TF, m, 1)
    args2[3][1] = sipx.Projector(sipx.set_definitions(SET[kind][0], SET[kind][1], 0.0, args1[3][1].pmax, _mode(n), weights=w2), args1[4], TF)
    want1, want2 = _fresh(sipx, args1, m), _fresh(sipx, args2, m)
    assert not np.array_equal(want1[0], want2[0]), "the two weight vectors give the same solve: nothing is shown"
    with sipx.Solver(*args1, TF) as S:
        _assert_same(_run(S, m.copy()), want1)
        S.set_data(1, lb=w2)
        got = _run(S, m.copy())
        assert got[3].context_reused
        _assert_same(got, want2)
        with pytest.raises(sipx.SipxError, match="the weights of an l2,1 set are its lb; it has no ub"):
            S.set_data(1, ub=w2)
    with sipx.Solver(*args1, TF) as S:
        wb = w2.copy()
        wb[3] = -1.0
        with pytest.raises(sipx.SipxError, match="weight 3 is negative, NaN or infinite"):
            S.set_data(1, lb=wb)
    dev = torch.device("cuda", 0)
    with sipx.Solver(*args1, TF) as S:
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        _assert_same(_run(S, t(m)), want1)
        S.set_data(1, lb=t(w2))
        _assert_same(_run(S, t(m)), want2)
        # weights only device memory can bring -- negative, NaN, infinite -- count as 0: the bits of the solve with zeros in their place
        wb, wz = w2.copy(), w2.copy()
        wb[[2, 5, 9]] = [-1.0, np.nan, np.inf]
        wz[[2, 5, 9]] = 0.0
        S.set_data(1, lb=t(wb))
        got = _run(S, t(m))
    args3 = _args(sipx, name, n, h, TF, m, 1)
    args3[3][1] = sipx.Projector(sipx.set_definitions(SET[kind][0], SET[kind][1], 0.0, args1[3][1].pmax, _mode(n), weights=wz), args1[4], TF)
    _assert_same(got, _fresh(sipx, args3, m))


def test_a_set_built_without_weights_still_refuses(sipx):
    TF, n, h = np.float32, (32, 24), (25.0, 6.0)
    g = sipx.compgrid(h, n)
    c = [sipx.set_definitions("bounds", "identity", 1600.0, 3900.0, _mode(n)), sipx.set_definitions("l21", "TV", 0.0, 50.0, _mode(n))]
    P, A, prop = sipx.setup_constraints(c, g, TF)
    opt = sipx.PARSDMM_options(FL=TF, maxit=5)
    A, AtA, _, _ = sipx.PARSDMM_precompute_distribute(A, prop, g, opt)
    with sipx.Solver(AtA, A, prop, P, g, opt, TF) as S:
        with pytest.raises(sipx.SipxError, match="holds no replaceable vectors"):
            S.set_data(1, lb=np.ones(32 * 24, TF))


# ---- the engine's refusals through the C ABI ---------------------------------------------------------------------------------------------------
def _desc(sipx, op, w, proj=14, mode=0, dir=0, pmax=1.0, count=None, ub=None):
    d = sipx.host._SetDesc()
    d.op, d.proj, d.pmin, d.pmax, d.mode, d.dir, d.transform = op, proj, 0.0, pmax, mode, dir, 0
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
    TV, TVXY = sipx.host.OPS["TV"], sipx.host.OPS["TV_xy"]
    n = (16, 12, 8)
    N, L = 16 * 12 * 8, 16 * 12
    g = _grid(sipx, n)
    w, wj = np.ones(N, TF), np.ones(L, TF)
    ctx = sipx.Context(g, TF)
    try:
        # wrong length
        assert f"the weighted l2,1 ball (l21): {N - 1} weights given, {N} are needed -- one per grid point" in _refused(sipx, ctx, _desc(sipx, TV, w, count=N - 1))
        assert f"the weighted l2,1 ball (l21): 0 weights given, {N} are needed" in _refused(sipx, ctx, _desc(sipx, TV, w, count=0))
        assert f"the weighted l2,1 ball (l21_joint): {N} weights given, {L} are needed -- one per pixel" in _refused(sipx, ctx, _desc(sipx, TVXY, w, proj=15))
        # a negative or NaN weight from the host
        for bad, at in ((-1.0, 7), (np.nan, 0), (np.inf, N - 1)):
            wb = w.copy()
            wb[at] = bad
            assert f"the weighted l2,1 ball (l21): weight {at} is negative, NaN or infinite" in _refused(sipx, ctx, _desc(sipx, TV, wb))
        wb = wj.copy()
        wb[11] = -0.5
        assert "the weighted l2,1 ball (l21_joint): weight 11 is negative, NaN or infinite" in _refused(sipx, ctx, _desc(sipx, TVXY, wb, proj=15))
        # the per-frame mode with weights
        assert "the l2,1 ball per frame takes no weights (lb): use the whole-array set on TV_xy or the joint set" in \
            _refused(sipx, ctx, _desc(sipx, TVXY, w, mode=2, dir=2))
        # ub given
        for d in (_desc(sipx, TV, w, ub=w), _desc(sipx, TV, None, ub=w), _desc(sipx, TVXY, wj, proj=15, ub=wj)):
            assert "takes weights in lb and no ub" in _refused(sipx, ctx, d)
        # the radius is still checked
        assert _refused(sipx, ctx, _desc(sipx, TV, w, pmax=0.0)) == "Radius of L1 ball is negative"
        # sets the engine takes: the weights are replaceable, lb alone, of the right values
        assert sipx.lib().sipx_add_set(ctx.h, C.byref(_desc(sipx, TV, w)), None, None, 0) == 0
        assert sipx.lib().sipx_add_set(ctx.h, C.byref(_desc(sipx, TVXY, wj, proj=15)), None, None, 0) == 1
        assert sipx.lib().sipx_add_set(ctx.h, C.byref(_desc(sipx, TV, None)), None, None, 0) == 2
        assert sipx.lib().sipx_set_data(ctx.h, 0, w.ctypes.data_as(C.c_void_p), None) == 0
        assert sipx.lib().sipx_set_data(ctx.h, 0, None, w.ctypes.data_as(C.c_void_p)) != 0
        assert "the weights of an l2,1 set are its lb; it has no ub" in sipx.lib().sipx_last_error().decode()
        wb = w.copy()
        wb[5] = np.nan
        assert sipx.lib().sipx_set_data(ctx.h, 0, wb.ctypes.data_as(C.c_void_p), None) != 0
        assert "the weighted l2,1 ball (l21): weight 5 is negative, NaN or infinite" in sipx.lib().sipx_last_error().decode()
        assert sipx.lib().sipx_set_data(ctx.h, 2, w.ctypes.data_as(C.c_void_p), None) != 0
        assert "holds no replaceable vectors" in sipx.lib().sipx_last_error().decode()
    finally:
        ctx.close()
    # a slab-decomposed or owned context
    msg = "the l2,1 ball on the TV operator (isotropic total variation) takes single-process contexts only"
    ctx = sipx.Context(g, TF)
    try:
        ctx.set_decomp("slab")
        assert msg in _refused(sipx, ctx, _desc(sipx, TV, w))
    finally:
        ctx.close()
    for shard in (lambda c: c.set_decomp("slab"), lambda c: c.set_owned([1, 1])):
        ctx = sipx.Context(g, TF)
        try:
            ctx.add_set(sipx.TDOperator("TV", g, TF), _P(sipx, "TV", n, TF, 1.0, w))
            shard(ctx)
            with pytest.raises(sipx.SipxError, match="takes single-process contexts only"):
                ctx.finalize(np.ones(N, TF), [10.0], 1.0)
        finally:
            ctx.close()
    # the stand-alone observer refuses what the host refuses
    ctx = sipx.Context(g, TF)
    try:
        out, x = np.zeros(1, TF), np.zeros(N, TF)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        wb = w.copy()
        wb[4] = -2.0
        assert sipx.lib().sipx_l21_weighted_norm(ctx.h, TV, 0, p(x), p(wb), p(out)) != 0
        assert "weight 4 is negative, NaN or infinite" in sipx.lib().sipx_last_error().decode()
        assert sipx.lib().sipx_l21_weighted_norm(ctx.h, TV, 1, p(x), p(wj), p(out)) != 0
        assert "TD_OP must be TV_xy, mode tensor" in sipx.lib().sipx_last_error().decode()
        assert sipx.lib().sipx_l21_weighted_norm(ctx.h, 0, 0, p(x), p(w), p(out)) != 0
        assert "TD_OP must be TV" in sipx.lib().sipx_last_error().decode()
        assert sipx.lib().sipx_l21_weighted_norm(ctx.h, TV, 0, p(x), None, p(out)) != 0
    finally:
        ctx.close()


def test_passes_are_reported(sipx):
    TF, n, h = np.float32, (32, 24), (25.0, 6.0)
    m = _model(n, TF, seed=7)
    with sipx.Solver(*_args(sipx, "wl21-TV", n, h, TF, m, 1), TF) as S:
        S(m.copy())
        st = S.ctx.kernel_stats_all(-1)["l21_weighted"]
    assert 2 <= st["passes"] <= 32 * 24 + 1 and st["flag_reads"] == -(-st["passes"] // 8) and st["groups"] == 32 * 24 and st["calls"] >= 2
