"""The l2,1 ball across the blocks of a stacked operator on the GPU (csrc/l21_stacked.h, csrc/ext_group.hip: k_l21s_norms,
k_l21s_scale behind BallProj) and second-order isotropic TV, ("l21", "Hessian"): the projector through sipx.Projector against
tests/l21_stacked_ref.py, inputs it must not write, the observed radius (sipx.l21_stacked_norm), whole solves against the oracle with
its projector swapped for the reference (the way tests/test_gpu_l21.py runs its solves, with its iteration counts and tolerances), the
caller-supplied two-block operator that reproduces ("l21", "TV"), and the engine's refusals through the C ABI.

SIZES.  G in {1, 3, 4, 255, 256, 257, 1028} has both access widths (G % 4 == 0 in Float32, G % 2 == 0 in Float64: 16 bytes per thread;
otherwise one group per thread), a tail workgroup and more than one workgroup.  The kernels launch min(ceil(G / (256 VW)), 2048)
workgroups of 256 threads (l21s_norms / l21s_scale in ext_group.hip: fit_grid(G / VW, NB), NB = 2048, BLOCK = 256), VW = 4 (Float32) or
2 (Float64) groups per thread on the 16-byte path: one trip of the grid-stride loop covers 2048 * 256 * VW groups.  G_TRIP(TF) =
2048 * 256 * VW + VW is the first wide size with a second trip; G_TRIP + 1 takes the narrow path, whose trip is 2048 * 256 groups.

THE PROJECTOR ALONE takes the M-vector itself (sipx_project with `blocks`), so the input is exactly what the test chooses; the set is
built on a caller-supplied operator of M rows -- the identity on a grid of M points for the small sizes, so that the observer sees the
same vector, and an empty M x 12 matrix for the two large ones, where only the row count matters."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch      # (before libsipx.so is loaded: one HIP runtime in the process)

from oracle import parsdmm_oracle as O
from tests import l1_exact, l21_ref
from tests import l21_stacked_ref as R

pytestmark = pytest.mark.gpu

BLOCKS = [1, 2, 3, 6, 8]
SMALL_G = [1, 3, 4, 255, 256, 257, 1028]
FRACS = [0.9, 0.5, 0.05]
_inputs = {}


def g_trip(TF):
    return 2048 * 256 * (16 // np.dtype(TF).itemsize) + 16 // np.dtype(TF).itemsize


def _mode(n):
    return ("matrix", "") if len(n) == 2 else ("tensor", "")


def _P(sipx, M, B, TF, tau, small=True):
    """The projector of an M-vector in B blocks (see the docstring of the module)."""
    if small:
        grid, A = sipx.compgrid((1.0, 1.0), (M, 1)), sp.identity(M, format="csc", dtype=TF)
    else:
        grid, A = sipx.compgrid((1.0, 1.0), (4, 3)), sp.csc_matrix((M, 12), dtype=TF)
    c = sipx.set_definitions("l21_stacked", "custom", 0.0, float(tau), ("matrix", ""), custom_TD_OP=(A, False), blocks=B)
    return sipx.Projector(c, grid, TF)


def make_input(B, G, TF):
    """(v, sum_p g_p): heavy-tailed randn * exp(randn), one all-zero group and one group of -0.0 where G allows; computed once, handed out
    as a copy."""
    key = (B, G, np.dtype(TF).name)
    if key not in _inputs:
        rng = np.random.default_rng(20250901 + 31 * B + G % 1000)
        v = (rng.standard_normal(B * G) * np.exp(rng.standard_normal(B * G))).astype(TF).reshape(B, G)
        if G >= 3:
            v[:, G // 2] = 0.0
            v[:, G - 1] = -0.0
        v = np.ascontiguousarray(v.reshape(-1))
        _inputs[key] = (v, R.norm21(v, B))
    v, nrm = _inputs[key]
    return v.copy(), nrm


def _check(sipx, B, G, TF, frac, small):
    v, nrm = make_input(B, G, TF)
    b = TF(frac * nrm)
    ref = R.project(v, B, b)
    P = _P(sipx, B * G, B, TF, b, small)
    y = P(v.copy())
    eps = float(np.finfo(TF).eps)
    v64 = np.abs(v.astype(np.float64))
    err = np.abs(y.astype(np.float64) - ref)
    worst = float(np.max(err / np.maximum(v64, np.finfo(np.float64).tiny)) / eps)
    print(f"l21_stacked B {B} G {G} {np.dtype(TF).name} frac {frac}: worst error {worst:.3f} eps |v|")
    assert np.all(err <= 4 * eps * v64), f"worst error {worst:.3f} eps |v|"
    if G >= 3:      # zero groups stay zero, with the sign of their zeros
        Y = y.reshape(B, G)
        assert np.all(Y[:, G // 2] == 0) and not np.any(np.signbit(Y[:, G // 2]))
        assert np.all(Y[:, G - 1] == 0) and (ref is v or np.all(np.signbit(Y[:, G - 1])))
    assert l1_exact.same_bits(P(v.copy()), y), "two calls differ"
    return worst


def test_the_large_sizes_need_a_second_trip():
    assert g_trip(np.float32) == 2097156 and g_trip(np.float64) == 1048578
    for TF, W in ((np.float32, 4), (np.float64, 2)):
        G = g_trip(TF)
        assert G % W == 0 and G // W > 2048 * 256 and (G - W) // W == 2048 * 256 and (G + 1) % W != 0 and G + 1 > 2048 * 256


@pytest.mark.parametrize("TF", [np.float32, np.float64])
@pytest.mark.parametrize("G", SMALL_G)
@pytest.mark.parametrize("B", BLOCKS)
def test_projector_matches_the_reference(sipx, TF, B, G):
    for frac in FRACS:
        _check(sipx, B, G, TF, frac, True)


@pytest.mark.parametrize("TF", [np.float32, np.float64])
@pytest.mark.parametrize("odd", [0, 1])
@pytest.mark.parametrize("B", BLOCKS)
def test_projector_matches_the_reference_beyond_one_trip(sipx, TF, B, odd):
    _check(sipx, B, g_trip(TF) + odd, TF, 0.5, False)


# ---- inputs the projector must not write, and the extremes -------------------------------------------------------------------------------
@pytest.mark.parametrize("TF", [np.float32, np.float64])
@pytest.mark.parametrize("B,G", [(3, 257), (6, 1028), (2, 256), (8, 3)])
def test_feasible_and_zero_inputs_come_back_bit_for_bit(sipx, TF, B, G):
    v, nrm = make_input(B, G, TF)
    v[::7] = -0.0
    v[3::11] = 0.0
    b = TF(2 * R.norm21(v, B))
    assert l1_exact.feasibility(R.norms(v, B, TF), b) > 0 and np.any(np.signbit(v) & (v == 0))
    assert l1_exact.same_bits(_P(sipx, B * G, B, TF, b)(v.copy()), v)
    z = np.zeros_like(v)
    z[::2] = -0.0
    assert l1_exact.same_bits(_P(sipx, B * G, B, TF, b)(z.copy()), z)


@pytest.mark.parametrize("TF", [np.float32, np.float64])
@pytest.mark.parametrize("B,G", [(3, 257), (6, 1028), (1, 255), (8, 4)])
def test_observed_radius_leaves_the_point_unwritten(sipx, TF, B, G):
    """tau = the observed norm: unwritten; just inside it: projected.  The observer against the reference's sum, to the tolerance
    tests/test_gpu_l21.py holds l21_norm to."""
    M = B * G
    v, _ = make_input(B, G, TF)
    grid = sipx.compgrid((1.0, 1.0), (M, 1))
    A = sp.identity(M, format="csc", dtype=TF)
    tau = sipx.l21_stacked_norm(v, grid, A, blocks=B)
    assert isinstance(tau, TF)
    ref = float(np.sum(R.norms(v, B, TF).astype(l1_exact._WIDE)))
    assert abs(float(tau) - ref) <= 2 * float(np.finfo(TF).eps) * ref
    assert l1_exact.same_bits(_P(sipx, M, B, TF, tau)(v.copy()), v), "v was written although its radius was observed on it"
    td = sipx.l21_stacked_norm(torch.from_numpy(v).cuda(), grid, A, blocks=B)
    assert td.is_cuda and td.shape == (1,) and l1_exact.same_bits(td.cpu().numpy(), np.array([tau], TF))
    assert not l1_exact.same_bits(_P(sipx, M, B, TF, float(tau) * 0.999)(v.copy()), v)


@pytest.mark.parametrize("TF", [np.float32, np.float64])
@pytest.mark.parametrize("B,G", [(3, 257), (6, 256), (2, 1028)])
def test_tiny_radius_keeps_the_largest_groups_only(sipx, TF, B, G):
    v, _ = make_input(B, G, TF)
    Vb = v.reshape(B, G)
    Vb[:, 5] = TF(1e4) * (1 + np.arange(B))
    Vb[:, 100] = Vb[:, 5] * TF(0.999)
    g = R.norms(v, B, TF).astype(np.float64)
    order = np.argsort(g)[::-1]
    assert set(order[:2]) == {5, 100} and g[order[1]] > 4 * g[order[2]]
    b = TF(1e-3 * g[order[1]])
    y = _P(sipx, B * G, B, TF, b)(v.copy()).reshape(B, G)
    gy = np.sqrt((y.astype(np.float64) ** 2).sum(axis=0))
    assert np.count_nonzero(gy) <= 2 and gy[order[0]] > 0
    ref = R.project(v, B, b)
    assert np.all(np.abs(y.reshape(-1).astype(np.float64) - ref) <= 4 * float(np.finfo(TF).eps) * np.abs(v.astype(np.float64)))


def test_float64_group_barely_above_a_small_threshold(sipx):
    """The case csrc/l21.h describes: many large groups, theta small against S / C, and a group a little above theta.  A float64
    evaluation of theta = (S - tau) / C is off by ulps of S / C = 2^-30 here, a thousand times the bound of 4 eps |v| = 2^-60 on that
    group's output g - theta; the threshold refined on the active set in twice the working precision is good to 2^-52 theta.  The group
    lies 2^-20 above theta, a thousand times the search's own error, so it is in the search's active set whatever the search rounds.
    Every number is a dyadic rational, so the exact projection is known in closed form (fractions): the extended-precision sum of the
    shared reference would itself be off by 2^-31 / C on these inputs and is not used."""
    from fractions import Fraction as F
    TF, B, G, C = np.float64, 3, 1028, 1000
    K, theta0, delta = 5.0 * 2 ** 20, 2.0 ** -10, 2.0 ** -20 + 2.0 ** -31      # (2^-31: below an ulp of S = 2^-20, so a float64 sum rounds)
    v = np.zeros((B, G))
    v[0, :C], v[1, :C] = 3.0 * 2 ** 20, 4.0 * 2 ** 20       # g = 5 * 2^20, exactly
    v[0, ::2] *= -1
    v[2, 1010] = theta0 + delta                             # the one-member group barely above theta
    tau = C * K - C * theta0
    assert F(tau) == C * F(K) - C * F(theta0), "tau is exact"
    theta = F(theta0) + F(delta) / (C + 1)                  # (C K + theta0 + delta - tau) / (C + 1)
    assert F(K) > theta and F(theta0 + delta) > theta > 0
    v = np.ascontiguousarray(v.reshape(-1))
    g = R.norms(v, B, TF)
    assert np.all(g[:C] == K) and g[1010] == theta0 + delta and np.count_nonzero(g) == C + 1
    y = _P(sipx, B * G, B, TF, tau)(v.copy())
    eps = float(np.finfo(TF).eps)
    worst = 0.0
    for k in np.nonzero(v)[0]:
        gp = F(float(g[k % G]))
        want = F(float(v[k])) * (gp - theta) / gp
        err = abs(F(float(y[k])) - want)
        worst = max(worst, float(err / (F(eps) * abs(F(float(v[k]))))))
    print(f"barely above: y {y[2 * G + 1010]!r}, exact {float(F(delta) * C / (C + 1))!r}, worst error {worst:.3f} eps |v|")
    assert worst <= 4.0, worst
    assert np.all(y[v == 0] == 0)
    plain = (float(np.sum(g[g > theta0])) - tau) / (C + 1)      # what a float64 evaluation gives: outside the bound, so the case shows something
    assert abs(F(plain) - theta) > 4 * F(eps) * F(theta0 + delta)


# ---- whole solves against the oracle (rules and tolerances of tests/test_gpu_l21.py, test_l21_solve_matches_oracle) ------------------------
def _model(n, TF, seed):
    rng = np.random.default_rng(20240601 + seed)
    z = np.linspace(0, 1, n[-1]).reshape((1,) * (len(n) - 1) + (-1,))
    return (1500 + 2500 * z + 150 * rng.standard_normal(n)).astype(TF).reshape(-1, order="F")


def _julia_max(v):
    v = np.asarray(v, np.float64)
    return float("nan") if np.isnan(v).any() else float(v.max())


def _in_place(project, x):
    y = project(x)
    if y is not x:
        x[:] = y
    return x


SOLVE_SETS = {"Hessian": ["H"], "TV+Hessian": ["TV", "H"]}
SOLVE_GRIDS = [((12, 9), (25.0, 6.0)), ((16, 16), (1.0, 1.0)), ((8, 6, 5), (25.0, 25.0, 25.0)), ((8, 8, 4), (1.0, 2.0, 3.0))]


def _hessian_problem(mod, sipx, name, n, h, TF, m, opt_kw, tau_scale=0.5, bounds=True):
    """{bounds, the sets of SOLVE_SETS[name]} for module `mod`; tau = half the norm of A m from the reference.  The oracle takes the
    Hessian as a caller-supplied operator under an l1 set, whose projector is then replaced by the reference's."""
    g = mod.compgrid(h, n)
    opt = mod.PARSDMM_options(FL=TF, **opt_kw)
    c = [mod.set_definitions("bounds", "identity", 1600.0, 3900.0, _mode(n))] if bounds else []
    swaps = []
    H = sipx.get_TD_operator(sipx.compgrid(h, n), "Hessian", TF)[0]
    B = 3 if len(n) == 2 else 6
    for kind in SOLVE_SETS[name]:
        if kind == "TV":
            s = np.asarray(O.get_TD_operator(O.compgrid(h, n), "TV", TF)[0] @ m, TF)
            c.append(mod.set_definitions("l1", "TV", 0.0, float(TF(0.5 * np.abs(s.astype(np.float64)).sum())), _mode(n)))
            continue
        r = TF(tau_scale * R.norm21(H @ m, B)) if tau_scale else TF(1.0)
        if mod is O:
            swaps.append((len(c), lambda x, r=r: _in_place(lambda t: R.project(t, B, r), x)))
            sd = mod.set_definitions("l1", "identity", 0.0, float(r), _mode(n))
            sd.custom_TD_OP = (H.A, False)
            c.append(sd)
        else:
            c.append(mod.set_definitions("l21", "Hessian", 0.0, float(r), _mode(n)))
    P, A, prop = mod.setup_constraints(c, g, TF)
    for i, f in swaps:
        P[i] = f
    A, AtA, l, y = mod.PARSDMM_precompute_distribute(A, prop, g, opt)
    return g, opt, P, A, prop, AtA


def _compare(name, n, TF, ls, lo, xs, xo, os_, replay):
    """The comparison of tests/test_gpu_l21.py::test_l21_solve_matches_oracle, word for word."""
    K = min(6, len(lo.obj), len(ls.obj))
    rt = 5e-4 if TF == np.float32 else 1e-8
    assert np.array_equal(ls.cg_it[:K], lo.cg_it[:K]), (ls.cg_it[:K], lo.cg_it[:K])
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
        xr = replay(len(ls.obj), (ls.rho, ls.gamma))      # the oracle again with the engine's rho / gamma history forced on it
        err_replay = np.linalg.norm(xs.astype(np.float64) - xr) / np.linalg.norm(xr)
        assert err_replay < tol, (name, "replayed", sep, err_replay)
        tol = max(tol, 5e-4)
        assert _julia_max(ls.set_feasibility[-1]) <= max(_julia_max(lo.set_feasibility[-1]), float(os_.feas_tol))
    assert err < tol, (name, sep, err)
    assert len(ls.obj) > 6, "the solve stopped before anything was compared"


@pytest.mark.parametrize("TF", [np.float32, np.float64])
@pytest.mark.parametrize("n,h", SOLVE_GRIDS)
@pytest.mark.parametrize("name", list(SOLVE_SETS))
def test_hessian_solve_matches_oracle(sipx, TF, name, n, h):
    m = _model(n, TF, seed=1 + len(SOLVE_SETS[name]))
    kw = dict(maxit=60)
    go, oo, Po, Ao, propo, AtAo = _hessian_problem(O, sipx, name, n, h, TF, m, kw)
    gs, os_, Ps, As, props, AtAs = _hessian_problem(sipx, sipx, name, n, h, TF, m, kw)
    i = len(As) - 2
    assert As[i].kind == "custom" and AtAs[i] is None and len(props.AtA_offsets[i]) == 0, "the Hessian enters Q matrix-free"
    assert props.ncvx == propo.ncvx
    xo, lo, l_o, y_o = O.PARSDMM(m.copy(), AtAo, Ao, propo, Po, go, oo)
    xs, ls, l_s, y_s = sipx.PARSDMM(m.copy(), AtAs, As, props, Ps, gs, os_)

    def replay(maxit, hist):
        gr, orr, Pr, Ar, propr, AtAr = _hessian_problem(O, sipx, name, n, h, TF, m, dict(kw, maxit=maxit))
        return O.PARSDMM(m.copy(), AtAr, Ar, propr, Pr, gr, orr, replay=hist)[0]
    _compare(name, n, TF, ls, lo, xs, xo, os_, replay)
    p = len(SOLVE_SETS[name]) + 2
    assert ls.r_pri.shape == (len(ls.obj), p) and ls.set_feasibility.shape[1] == p - 1
    assert len(y_s) == p and [len(q) for q in y_s] == [len(q) for q in y_o]


# ---- the caller-supplied two-block operator [D_x; D_z], zero-padded to N rows each: the groups of ("l21", "TV") ------------------------------
def _padded_gradient(n, h, TF):
    """[D_x zero-padded to N rows; D_z zero-padded to N rows] on the 2-D grid n: row q N + p holds the forward difference along x (q = 0)
    or z (q = 1) that starts at p, a zero row on the far face -- the groups of l21.h, in the stacked layout."""
    n1, n2 = n
    N = n1 * n2
    ih = [TF(1) / TF(k) for k in h]
    c = np.unravel_index(np.arange(N), n, order="F")
    rows, cols, vals = [], [], []
    for q, (a, st) in enumerate(((0, 1), (1, n1))):
        p = np.nonzero(c[a] < n[a] - 1)[0]
        rows += [q * N + p, q * N + p]
        cols += [p, p + st]
        vals += [np.full(len(p), -ih[a], TF), np.full(len(p), ih[a], TF)]
    A = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(2 * N, N), dtype=TF)
    A.sort_indices()
    return A


@pytest.mark.parametrize("TF", [np.float32, np.float64])
@pytest.mark.parametrize("route", ["banded", "matrix-free"])
def test_two_block_gradient_reproduces_isotropic_tv(sipx, TF, route):
    n, h = (12, 9), (25.0, 6.0)
    m = _model(n, TF, seed=5)
    g = sipx.compgrid(h, n)
    opt = sipx.PARSDMM_options(FL=TF, maxit=60)
    TV = O.get_TD_operator(O.compgrid(h, n), "TV", TF)[0]
    r = TF(0.5 * l21_ref.norm21(np.asarray(TV @ m, TF), n))
    A2 = _padded_gradient(n, h, TF)
    assert abs(R.norm21(A2 @ m, 2) - l21_ref.norm21(np.asarray(TV @ m, TF), n)) <= 1e-12 * float(r), "the same groups"
    xs = {}
    for which in ("tv", "stacked"):
        c = [sipx.set_definitions("bounds", "identity", 1600.0, 3900.0, ("matrix", ""))]
        if which == "tv":
            c.append(sipx.set_definitions("l21", "TV", 0.0, float(r), ("matrix", "")))
        else:
            c.append(sipx.set_definitions("l21_stacked", "gradient", 0.0, float(r), ("matrix", ""), custom_TD_OP=(A2, False), blocks=2))
        P, A, prop = sipx.setup_constraints(c, g, TF)
        if which == "stacked" and route == "matrix-free":
            prop.banded[1] = False
        A, AtA, l, y = sipx.PARSDMM_precompute_distribute(A, prop, g, opt)
        if which == "stacked":
            assert (AtA[1] is None) == (route == "matrix-free") and len(prop.AtA_offsets[1]) == (0 if route == "matrix-free" else 5)
        x, log, l, y = sipx.PARSDMM(m.copy(), AtA, A, prop, P, g, opt)
        assert len(log.obj) > 6
        xs[which] = (x.astype(np.float64), log)
    err = np.linalg.norm(xs["stacked"][0] - xs["tv"][0]) / np.linalg.norm(xs["tv"][0])
    print(f"two-block gradient {route} {np.dtype(TF).name}: iterations {len(xs['stacked'][1].obj)} / {len(xs['tv'][1].obj)}, rel diff {err:.3e}")
    assert err < (5e-4 if TF == np.float32 else 1e-6), err


# ---- what second-order TV leaves alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("TF", [np.float32, np.float64])
@pytest.mark.parametrize("n", [(12, 9), (8, 6, 5)])
def test_affine_model_passes_unchanged(sipx, TF, n):
    """An affine model has H m = 0 (the mixed blocks: a few ulp of sqrt(2) max|m|, tests/test_l21_stacked_cpu.py), so it lies in the set
    for a small tau and the projection is m itself.  "Unchanged to solver tolerance": as close to m as the oracle's solve of the same
    problem gets, to the tolerance the solves above are held to; and the engine's result is in the set."""
    h = tuple(1.0 for _ in n)
    c = np.unravel_index(np.arange(int(np.prod(n))), n, order="F")
    m = (2000 + 30 * c[0] - 17 * c[1] + (11 * c[2] if len(n) == 3 else 0)).astype(TF)
    kw = dict(maxit=60)
    go, oo, Po, Ao, propo, AtAo = _hessian_problem(O, sipx, "Hessian", n, h, TF, m, kw, tau_scale=0, bounds=False)
    gs, os_, Ps, As, props, AtAs = _hessian_problem(sipx, sipx, "Hessian", n, h, TF, m, kw, tau_scale=0, bounds=False)
    tau = sipx.l21_stacked_norm(m, gs, "Hessian")
    assert float(tau) < 1.0 == Ps[0].pmax, "m is inside the set"
    xo, lo, _, _ = O.PARSDMM(m.copy(), AtAo, Ao, propo, Po, go, oo)
    xs, ls, _, _ = sipx.PARSDMM(m.copy(), AtAs, As, props, Ps, gs, os_)
    nm = np.linalg.norm(m.astype(np.float64))
    ds, do = np.linalg.norm(xs.astype(np.float64) - m) / nm, np.linalg.norm(xo - m) / nm
    tol = 5e-4 if TF == np.float32 else 1e-6
    print(f"affine {n} {np.dtype(TF).name}: |x - m| / |m| engine {ds:.3e} oracle {do:.3e}, iterations {len(ls.obj)} / {len(lo.obj)}")
    assert ds <= do + tol
    assert np.linalg.norm(xs.astype(np.float64) - xo) / np.linalg.norm(xo) < tol
    assert float(sipx.l21_stacked_norm(xs, gs, "Hessian")) <= 1.0 * (1 + float(os_.feas_tol))


@pytest.mark.parametrize("TF", [np.float32, np.float64])
def test_radius_observed_on_x_makes_the_solve_return_x(sipx, TF):
    """tau = sipx.l21_stacked_norm(m): A m is a point the projector does not write, so m is in the set and the solve returns it -- as
    closely as the oracle's solve with the same radius does."""
    n, h = (16, 16), (1.0, 1.0)
    m = _model(n, TF, seed=9)
    g = sipx.compgrid(h, n)
    tau = sipx.l21_stacked_norm(m, g, "Hessian")
    H = sipx.get_TD_operator(g, "Hessian", TF)[0]
    v = H @ m
    ref = float(np.sum(R.norms(v, 3, TF).astype(l1_exact._WIDE)))
    assert abs(float(tau) - ref) <= 2 * float(np.finfo(TF).eps) * ref * 4      # (H m on the device: the sums of four rounded terms a row)
    P = sipx.Projector(sipx.set_definitions("l21", "Hessian", 0.0, float(tau), ("matrix", "")), g, TF)
    opt = sipx.PARSDMM_options(FL=TF, maxit=60)
    Ps, A, prop = sipx.setup_constraints([sipx.set_definitions("l21", "Hessian", 0.0, float(tau), ("matrix", ""))], g, TF)
    A, AtA, l, y = sipx.PARSDMM_precompute_distribute(A, prop, g, opt)
    x, log, _, _ = sipx.PARSDMM(m.copy(), AtA, A, prop, Ps, g, opt)
    go = O.compgrid(h, n)
    co = [O.set_definitions("l1", "identity", 0.0, float(tau), ("matrix", ""))]
    co[0].custom_TD_OP = (H.A, False)
    Po, Ao, propo = O.setup_constraints(co, go, TF)
    r = TF(tau)
    Po[0] = lambda t: _in_place(lambda u: R.project(u, 3, r), t)
    oo = O.PARSDMM_options(FL=TF, maxit=60)
    Ao, AtAo, _, _ = O.PARSDMM_precompute_distribute(Ao, propo, go, oo)
    xo, lo, _, _ = O.PARSDMM(m.copy(), AtAo, Ao, propo, Po, go, oo)
    nm = np.linalg.norm(m.astype(np.float64))
    ds, do = np.linalg.norm(x.astype(np.float64) - m) / nm, np.linalg.norm(xo - m) / nm
    print(f"observed radius {np.dtype(TF).name}: |x - m| / |m| engine {ds:.3e} oracle {do:.3e}, iterations {len(log.obj)} / {len(lo.obj)}")
    assert ds <= do + (5e-4 if TF == np.float32 else 1e-6)
    assert P.pmax == float(tau)


# ---- the engine's refusals through the C ABI ---------------------------------------------------------------------------------------------------
def _desc(sipx, A, blocks, pmax=1.0, mode=0, transform=0, component=0, op=5):
    d = sipx.host._SetDesc()
    d.op, d.proj, d.pmin, d.pmax, d.mode, d.transform, d.component, d.blocks = op, 23, 0.0, pmax, mode, transform, component, blocks
    keep = []
    if A is not None:
        cp, ri, nz = (np.ascontiguousarray(A.indptr, np.int64), np.ascontiguousarray(A.indices, np.int64), np.ascontiguousarray(A.data))
        d.csc_colptr, d.csc_rowval, d.csc_nzval, d.csc_rows = cp.ctypes.data, ri.ctypes.data, nz.ctypes.data, A.shape[0]
        keep = [cp, ri, nz]
    return d, keep


def _refused(sipx, ctx, dk):
    rc = sipx.lib().sipx_add_set(ctx.h, C.byref(dk[0]), None, None, 0)
    assert rc < 0, "the engine took the set"
    return sipx.lib().sipx_last_error().decode()


def test_engine_refusals(sipx):
    TF = np.float32
    Hm = sipx.host
    n = (12, 9)
    g = sipx.compgrid((1.0, 1.0), n)
    H = sipx.get_TD_operator(g, "Hessian", TF)[0].A
    odd = sp.vstack([H, H[:1]], format="csc")
    odd.sort_indices()
    ctx = sipx.Context(g, TF)
    try:
        assert _refused(sipx, ctx, _desc(sipx, odd, 3)) == Hm.l21s_bad_rows(325, 3)
        assert _refused(sipx, ctx, _desc(sipx, H, 0)) == Hm.l21s_bad_blocks(0)
        assert _refused(sipx, ctx, _desc(sipx, H, 9)) == Hm.l21s_bad_blocks(9)
        assert _refused(sipx, ctx, _desc(sipx, None, 2, op=4)) == Hm.L21S_NEEDS_CSC
        assert _refused(sipx, ctx, _desc(sipx, H, 3, mode=1)) == Hm.L21S_WHOLE_ONLY
        assert _refused(sipx, ctx, _desc(sipx, H, 3, transform=1)) == Hm.L21S_NO_TRANSFORM
        assert _refused(sipx, ctx, _desc(sipx, H, 3, component=1)) == Hm.L21S_NO_MINKOWSKI
        for r in (0.0, -2.0, float("nan")):
            assert _refused(sipx, ctx, _desc(sipx, H, 3, pmax=r)) == "Radius of L1 ball is negative"
        d = _desc(sipx, H, 3)
        d[0].proj = Hm.PROJ["rank"]
        assert "library-backed projectors are not available" in _refused(sipx, ctx, d)
        # a set the engine takes: no replaceable vectors; sipx_project refuses a length that is no multiple of blocks
        d = _desc(sipx, H, 3)
        assert sipx.lib().sipx_add_set(ctx.h, C.byref(d[0]), None, None, 0) == 0
        ub = np.ones(4, TF)
        assert sipx.lib().sipx_set_data(ctx.h, 0, None, ub.ctypes.data_as(C.c_void_p)) != 0
        assert "holds no replaceable vectors" in sipx.lib().sipx_last_error().decode()
        v = np.zeros(325, TF)
        assert sipx.lib().sipx_project(ctx.h, C.byref(d[0]), v.ctypes.data_as(C.c_void_p), C.c_int64(len(v))) != 0
        assert sipx.lib().sipx_last_error().decode() == Hm.l21s_bad_rows(325, 3)
    finally:
        ctx.close()
    ctx = sipx.Context(g, TF)
    try:
        ctx.set_decomp("slab")
        assert _refused(sipx, ctx, _desc(sipx, H, 3)) == Hm.L21S_SHARDED
    finally:
        ctx.close()
    P = sipx.Projector(sipx.set_definitions("l21", "Hessian", 0.0, 1.0, ("matrix", "")), g, TF)
    for late in ("slab", "owned"):
        ctx = sipx.Context(g, TF)
        try:
            ctx.add_set(sipx.get_TD_operator(g, "Hessian", TF)[0], P)
            if late == "slab":
                ctx.set_decomp("slab")
            else:
                ctx.set_owned([1, 1])
            with pytest.raises(sipx.SipxError, match="takes single-process contexts only"):
                ctx.finalize(np.ones(108, TF), [10.0], 1.0)
        finally:
            ctx.close()
