"""The weighted l1 ball on the GPU (csrc/l1_weighted.h, csrc/ext_group.hip: L1WProj, k_l1w_part, k_l1w_apply) through sipx.Projector
against tests/l1_weighted_ref.py: accuracy, inputs and rows it must not write, the exact tie, the observed weighted norm, whole solves
against the oracle with its projector swapped for the reference, replaced weights in a live Solver, the device-resident solve and the
engine's refusals through the C ABI.

GRIDS.  Both kernels walk ONE flat array of nblk N entries (the blocks of the padded layout side by side) with the weights beside it,
0 at every row a block does not have.  identity (4,3): no pad at all, one workgroup.  D_x (5,4,3): the pad is the last entry of every
grid line; D_x (8,3,2): n1 % 4 == 0, so that pad lies INSIDE a 16-byte vector whose other entries are weighted (Float32: the 4th of 4,
Float64: the 2nd of 2) and its own bits are stored back.  D_z (5,4,3): the pad is the last plane, a run at the end of the array.  TV
(4,3) and (5,4,3), TV_xy (5,4,3): the smallest grids with every boundary class, two and three blocks.  TV (33,20) and (20,9,6): an odd
n1, one entry per lane.  TV (64,48) and (32,12,8), TV_xy (32,12,8): n1 % 4 == 0, 16 bytes per lane and array.  TV (725,727): an odd n1
(the one-entry path) whose 2 N = 1 054 150 entries just exceed one sweep of the full pass grid, L21W_GRID * 256 * L21W_LOADS = 1024 * 256
* 4 = 1 048 576 entries: every thread takes one unrolled round and the first 5 574 a second one through the tail loop; the apply
kernel, capped at NB = 2048 workgroups of 256, takes three grid-stride rounds there.  That grid runs with two weight families and two fractions only."""
import ctypes as C

import numpy as np
import pytest
import torch      # (before libsipx.so is loaded: one HIP runtime in the process)

from oracle import parsdmm_oracle as O
from tests import l1_exact
from tests import l1_weighted_ref as R
from tests.test_gpu_l21_frames import LOG_FIELDS, _in_place, _julia_max, _model, _stacked
from tests.test_gpu_set_data import _assert_same
from tests.test_l1_weighted_cpu import TIE_SIGN, tie
from tests.test_l21_weighted_cpu import FAMILIES, weights

pytestmark = pytest.mark.gpu

LARGE = ("TV", (725, 727))
L21W_GRID, BLOCK, L21W_LOADS = 1024, 256, 4      # csrc/ext_group.hip
CASES = [("identity", (4, 3)), ("D_x", (5, 4, 3)), ("D_x", (8, 3, 2)), ("D_z", (5, 4, 3)), ("TV", (4, 3)), ("TV", (5, 4, 3)), ("TV_xy", (5, 4, 3)),
         ("TV", (33, 20)), ("TV", (20, 9, 6)), ("TV", (64, 48)), ("TV", (32, 12, 8)), ("TV_xy", (32, 12, 8))]
FRACS = [0.9, 0.5, 0.05]
PRECISIONS = [np.float32, np.float64]
ALL = [(op, n, fam, fr) for op, n in CASES for fam in FAMILIES for fr in FRACS] + \
      [LARGE + (fam, fr) for fam in ("edge", "lognormal") for fr in (0.5, 0.05)]
_cache = {}
_worst = {}


def _grid(sipx, n, h=None):
    return sipx.compgrid(tuple(1.0 for _ in n) if h is None else h, n)


def _mode(n):
    return ("matrix", "") if len(n) == 2 else ("tensor", "")


def _P(sipx, op, n, TF, tau, w, g=None):
    return sipx.Projector(sipx.set_definitions("l1_weighted", op, 0.0, float(tau), _mode(n), weights=w), g or _grid(sipx, n), TF)


def _input(op, n, TF):
    """Heavy-tailed randn * exp(randn) on every row; computed once, handed out as a copy."""
    key = ("v", op, n, np.dtype(TF).name)
    if key not in _cache:
        rng = np.random.default_rng(20251021 + sum(n) + len(op))
        M = R.rows(n, op)
        _cache[key] = (rng.standard_normal(M) * np.exp(rng.standard_normal(M))).astype(TF)
    return _cache[key].copy()


def _weights(op, n, family, TF):
    key = ("w", op, n, family, np.dtype(TF).name)
    if key not in _cache:
        _cache[key] = weights(family, np.random.default_rng(9 + sum(n) + len(family) + len(op)), R.rows(n, op), TF)
        _cache[key].setflags(write=False)
    return _cache[key]


def test_the_large_grid_needs_a_second_round():
    op, n = LARGE
    N = int(np.prod(n))
    sweep = L21W_GRID * BLOCK * L21W_LOADS
    assert sweep == 1048576 and n[0] % 4 != 0 and len(R.block_dirs(n, op)) == 2
    assert sweep < 2 * N < sweep + L21W_GRID * BLOCK, "more than one unrolled round of the full grid, less than one more tail round"
    assert all(max(len(R.block_dirs(m, o)), 1) * int(np.prod(m)) < sweep for o, m in CASES)
    # the pads the small grids are chosen for
    assert np.array_equal(np.setdiff1d(np.arange(48), R.members((8, 3, 2), "D_x")), np.arange(7, 48, 8))
    assert np.array_equal(np.setdiff1d(np.arange(60), R.members((5, 4, 3), "D_z")), np.arange(40, 60))


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("op,n,family,frac", ALL)
def test_projector_matches_the_reference(sipx, TF, op, n, family, frac):
    """|y - y*| <= 2 eps |v_i| per entry.  theta* (1 + d1) for the one rounding of theta to T, the product's rounding (1 + d2) and the
    subtraction's give at most u (2 theta w_i + |v_i|) <= 3 u |v_i| = 1.5 eps |v_i| for a surviving entry (theta w_i < |v_i|, u = eps / 2);
    an entry the two sides classify differently lies within 2 u theta w_i of the threshold; the search's own slack is far below eps.
    Worst ratio observed on the MI355X over all cases: 0.77 (Float32), 0.77 (Float64) of eps |v_i|."""
    v, w = _input(op, n, TF), _weights(op, n, family, TF)
    b = TF(frac * R.norm(v, w))
    ref = R.project(v, w, b)
    assert ref is not v
    P = _P(sipx, op, n, TF, b, w)
    y = P(v.copy())
    eps = float(np.finfo(TF).eps)
    av = np.abs(v.astype(R.W))
    err = np.abs(y.astype(R.W) - ref.astype(R.W))
    worst = float(np.max(err / np.maximum(av, np.finfo(np.float64).tiny)) / eps)
    _worst[np.dtype(TF).name] = max(_worst.get(np.dtype(TF).name, 0.0), worst)
    print(f"l1 weighted {op} {n} {np.dtype(TF).name} {family} frac {frac}: worst error {worst:.3f} eps |v|; so far {_worst}")
    assert np.all(err <= 2 * eps * av), f"worst error {worst:.3f} eps |v|"
    assert l1_exact.same_bits(P(v.copy()), y), "two calls differ"
    if family == "ones":                          # all ones: the plain l1 ball's exact threshold, at the same bound
        # (one zero more: the reference's scan never takes ALL entries as active, `rho + 1 < lv`, a cap the weighted rule does not carry
        # over -- csrc/l21_weighted.h; with a zero appended, which is never active, the scan may take every entry of v)
        th, cnt, _ = l1_exact.exact_theta(np.append(np.abs(v), TF(0)), b)
        assert 0 < cnt <= len(v)
        plain = np.sign(v.astype(R.W)) * np.maximum(av - R.W(th), 0)
        assert np.all(np.abs(y.astype(R.W) - plain) <= 2 * eps * av)
    if family == "masked":                        # rows of weight 0 come back bit for bit while the others are shrunk
        free = np.asarray(w) == 0
        assert free.any() and l1_exact.same_bits(y[free], v[free])
        assert np.any(y[~free] != v[~free])


# ---- inputs the projector must not write -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("op,n", [("identity", (4, 3)), ("D_x", (8, 3, 2)), ("TV", (33, 20)), ("TV", (32, 12, 8)), ("TV_xy", (32, 12, 8))])
def test_feasible_and_zero_inputs_come_back_bit_for_bit(sipx, TF, op, n):
    v, w = _input(op, n, TF), _weights(op, n, "edge", TF)
    v[::7] = -0.0
    v[3::11] = 0.0
    b = TF(2 * R.norm(v, w))
    assert R.feasibility(np.abs(v), w, b) > 0 and np.any(np.signbit(v) & (v == 0))
    assert l1_exact.same_bits(_P(sipx, op, n, TF, b, w)(v.copy()), v)
    z = np.zeros_like(v)
    z[::2] = -0.0
    assert l1_exact.same_bits(_P(sipx, op, n, TF, b, w)(z.copy()), z)
    # all weights zero: no radius makes the projector write
    v = _input(op, n, TF)
    assert l1_exact.same_bits(_P(sipx, op, n, TF, 1e-6, np.zeros(len(v), TF))(v.copy()), v)


# ---- the tie: integers and power-of-two weights, exact in both precisions ----------------------------------------------------------------------
@pytest.mark.parametrize("TF", PRECISIONS)
def test_entries_on_the_threshold_are_zeroed(sipx, TF):
    v, w, tau = tie(TF)
    assert R.theta_star(np.abs(v), w, tau) == 2.5 and np.signbit(v[6]) and v[6] == 0
    y = _P(sipx, "identity", (4, 2), TF, tau, w)(v.copy())
    want = (np.array([0, 2, 4.5, 0, 2, 4.5, 0, 0], TF) * np.array(TIE_SIGN, TF)).astype(TF)
    assert l1_exact.same_bits(y, want), (y, want)


# ---- the observed weighted norm ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("op,n", [("identity", (33, 20)), ("D_x", (8, 3, 2)), ("D_z", (20, 9, 6)), ("TV", (33, 20)), ("TV", (64, 48)),
                                  ("TV", (32, 12, 8)), ("TV_xy", (32, 12, 8))])
def test_observed_radius_leaves_the_point_unwritten(sipx, TF, op, n):
    g = _grid(sipx, n, tuple(3.0 + a for a in range(len(n))))
    x = np.random.default_rng(5 + sum(n)).standard_normal(int(np.prod(n))).astype(TF)
    w = _weights(op, n, "lognormal", TF)
    v = sipx.TDOperator(op, g, TF) @ x
    tau = sipx.l1_weighted_norm(x, g, op, w)
    assert isinstance(tau, TF)
    # (T)asum of the serial emulation, up to the reordering of the pass tree: 4 eps relative
    e_asum = R.emulate_search(np.abs(v), w, TF(np.inf))[2]
    assert abs(float(tau) - float(e_asum)) <= 4 * float(np.finfo(TF).eps) * float(e_asum)
    assert l1_exact.same_bits(_P(sipx, op, n, TF, tau, w, g)(v.copy()), v), "A x was written although its radius was observed on x"
    td = sipx.l1_weighted_norm(torch.from_numpy(x).cuda(), g, op, torch.from_numpy(np.array(w)).cuda())
    assert td.is_cuda and td.shape == (1,) and l1_exact.same_bits(td.cpu().numpy(), np.array([tau], TF))
    y = _P(sipx, op, n, TF, float(tau) * 0.999, w, g)(v.copy())
    assert not l1_exact.same_bits(y, v)


# ---- whole solves against the oracle (rules and tolerances of tests/test_gpu_l21.py, test_l21_solve_matches_oracle) -----------------------------
SOLVE_SETS = {"wl1-TV": [(True, "TV")], "wl1-Dz+l1-Dx": [(True, "D_z"), (False, "D_x")], "wl1-TVxy": [(True, "TV_xy")]}
SOLVE_CASES = [("wl1-TV", (32, 24), (25.0, 6.0)), ("wl1-Dz+l1-Dx", (16, 12, 8), (25.0, 25.0, 25.0)), ("wl1-TVxy", (16, 12, 8), (25.0, 25.0, 25.0))]


def _solve_weights(op, n, TF, which=1):
    """Edge-type weights with a tenth of the rows free; `which` picks one of two vectors (set_data)."""
    rng = np.random.default_rng(100 * which + sum(n) + len(op))
    w = weights("edge", rng, R.rows(n, op), np.float64) * which
    w[rng.random(len(w)) < 0.1] = 0.0
    return w.astype(TF)


def _solve_problem(mod, name, n, h, TF, m, opt_kw, which=1):
    """{bounds, the sets of SOLVE_SETS[name]} for module `mod`; tau = half the (weighted) l1 norm of A m.  The oracle is set up with the
    plain l1 ball on the operator (TV_xy: its own D_y and D_x stacked, as a custom operator), its projector then replaced by the
    reference."""
    g = mod.compgrid(h, n)
    opt = mod.PARSDMM_options(FL=TF, **opt_kw)
    c = [mod.set_definitions("bounds", "identity", 1600.0, 3900.0, _mode(n))]
    swaps = []
    for weighted, opn in SOLVE_SETS[name]:
        A = _stacked(n, h, TF) if opn == "TV_xy" else O.get_TD_operator(O.compgrid(h, n), opn, TF)[0]
        s = np.asarray(A @ m, TF)
        if weighted:
            w = _solve_weights(opn, n, TF, which)
            r = TF(0.5 * R.norm(s, w))
            swaps.append((len(c), lambda x, r=r, w=w: _in_place(lambda a, rr: R.project(a, w, rr), x, r)))
        else:
            w = None
            r = TF(0.5 * np.abs(s.astype(np.float64)).sum())
        if mod is O:
            c.append(mod.set_definitions("l1", "identity" if opn == "TV_xy" else opn, 0.0, float(r), _mode(n),
                                         (A, False) if opn == "TV_xy" else ((), False)))
        elif w is None:
            c.append(mod.set_definitions("l1", opn, 0.0, float(r), _mode(n)))
        else:
            c.append(mod.set_definitions("l1_weighted", opn, 0.0, float(r), _mode(n), weights=w))
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
    TF, n, h = np.float32, (16, 12, 8), (25.0, 25.0, 25.0)
    m = _model(n, TF, seed=3)
    g, opt, P, A, prop, AtA = _solve_problem(sipx, "wl1-Dz+l1-Dx", n, h, TF, m, dict(maxit=30))
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
@pytest.mark.parametrize("name,n,h", [("wl1-TV", (32, 24), (25.0, 6.0)), ("wl1-Dz+l1-Dx", (16, 12, 8), (25.0, 25.0, 25.0))])
def test_set_data_then_reset_gives_the_bits_of_a_new_context(sipx, TF, name, n, h):
    """Built with weights 1 and solved; then set_data(weights 2), the next solve (a reset): x, every l_i, y_i and log array equal a new
    context built with weights 2 (the radius stays the one of weights 1: only lb is replaceable).  Host form, then device form."""
    m = _model(n, TF, seed=5)
    args1 = _args(sipx, name, n, h, TF, m, 1)
    op = SOLVE_SETS[name][0][1]
    w2 = _solve_weights(op, n, TF, 2)

    def with_weights(w):
        a = _args(sipx, name, n, h, TF, m, 1)
        a[3][1] = sipx.Projector(sipx.set_definitions("l1_weighted", op, 0.0, args1[3][1].pmax, _mode(n), weights=w), args1[4], TF)
        return a
    want1, want2 = _fresh(sipx, args1, m), _fresh(sipx, with_weights(w2), m)
    assert not np.array_equal(want1[0], want2[0]), "the two weight vectors give the same solve: nothing is shown"
    with sipx.Solver(*args1, TF) as S:
        _assert_same(_run(S, m.copy()), want1)
        S.set_data(1, lb=w2)
        got = _run(S, m.copy())
        assert got[3].context_reused
        _assert_same(got, want2)
        with pytest.raises(sipx.SipxError, match="the weights of the weighted l1 ball are its lb; it has no ub"):
            S.set_data(1, ub=w2)
    with sipx.Solver(*args1, TF) as S:
        wb = w2.copy()
        wb[3] = -1.0
        with pytest.raises(sipx.SipxError, match=r"the weighted l1 ball \(l1_weighted\): weight 3 is negative, NaN or infinite"):
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
    _assert_same(got, _fresh(sipx, with_weights(wz), m))


# ---- the engine's refusals through the C ABI ---------------------------------------------------------------------------------------------------
def _desc(sipx, op, w, proj=18, mode=0, dir=0, pmax=1.0, count=None, ub=None, transform=0, component=0):
    d = sipx.host._SetDesc()
    d.op, d.proj, d.pmin, d.pmax, d.mode, d.dir, d.transform, d.component = op, proj, 0.0, pmax, mode, dir, transform, component
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
    TV, DX, ID = OPS["TV"], OPS["D_x"], OPS["identity"]
    n = (16, 12, 8)
    N = 16 * 12 * 8
    M = R.rows(n, "TV")
    g = _grid(sipx, n)
    w = np.ones(M, TF)
    ctx = sipx.Context(g, TF)
    try:
        # wrong count
        assert f"the weighted l1 ball (l1_weighted): {M - 1} weights given, {M} are needed -- one per row of the operator, in the order of A x" \
            == _refused(sipx, ctx, _desc(sipx, TV, w, count=M - 1))
        assert f"the weighted l1 ball (l1_weighted): {M} weights given, {N} are needed" in _refused(sipx, ctx, _desc(sipx, ID, w))
        assert f"the weighted l1 ball (l1_weighted): 0 weights given, {M} are needed" in _refused(sipx, ctx, _desc(sipx, TV, w, count=0))
        # a bad weight from the host, the first offender named
        for bad, at in ((-1.0, 7), (np.nan, 0), (np.inf, M - 1)):
            wb = w.copy()
            wb[at] = bad
            assert _refused(sipx, ctx, _desc(sipx, TV, wb)) == f"the weighted l1 ball (l1_weighted): weight {at} is negative, NaN or infinite " \
                "-- every weight must be finite and >= 0 (0 leaves its row free)"
        # ub given
        for d in (_desc(sipx, TV, w, ub=w), _desc(sipx, TV, None, ub=w, count=M)):
            assert _refused(sipx, ctx, d) == "the weighted l1 ball (l1_weighted) takes weights in lb and no ub: the radius is pmax"
        # fiber / slice modes
        for op, mode, dirn in ((TV, 1, 0), (DX, 1, 2), (ID, 2, 2)):
            assert _refused(sipx, ctx, _desc(sipx, op, w, mode=mode, dir=dirn)) == \
                "the weighted l1 ball (l1_weighted) applies to the whole array (matrix / tensor mode): per fiber or slice use " \
                "(\"l1\", op, mode) with segment_norms=True, which takes one radius per segment"
        # transforms
        wi = np.ones(N, TF)
        for tr in (1, 2):
            assert _refused(sipx, ctx, _desc(sipx, ID, wi, transform=tr)) == \
                "the weighted l1 ball (l1_weighted) takes no transform (DFT, DCT, wavelet): its weights are one per row of identity, D_x, " \
                "D_y, D_z, TV or TV_xy -- behind a transform use the plain (\"l1\", transform)"
        # a Minkowski component
        assert _refused(sipx, ctx, _desc(sipx, TV, w, component=1)) == \
            "the weighted l1 ball (l1_weighted) takes no Minkowski component: use the plain (\"l1\", op) there"
        # the radius
        for pm in (0.0, float("nan"), -2.0):
            assert _refused(sipx, ctx, _desc(sipx, TV, w, pmax=pm)) == "Radius of L1 ball is negative"
        # a set the engine takes: the weights are replaceable, lb alone, of the right values
        assert sipx.lib().sipx_add_set(ctx.h, C.byref(_desc(sipx, TV, w)), None, None, 0) == 0
        assert sipx.lib().sipx_add_set(ctx.h, C.byref(_desc(sipx, TV, None, proj=2)), None, None, 0) == 1
        assert sipx.lib().sipx_set_data(ctx.h, 0, w.ctypes.data_as(C.c_void_p), None) == 0
        assert sipx.lib().sipx_set_data(ctx.h, 0, None, w.ctypes.data_as(C.c_void_p)) != 0
        assert "the weights of the weighted l1 ball are its lb; it has no ub (the radius is fixed at sipx_add_set)" in sipx.lib().sipx_last_error().decode()
        wb = w.copy()
        wb[5] = np.nan
        assert sipx.lib().sipx_set_data(ctx.h, 0, wb.ctypes.data_as(C.c_void_p), None) != 0
        assert "the weighted l1 ball (l1_weighted): weight 5 is negative, NaN or infinite" in sipx.lib().sipx_last_error().decode()
        assert sipx.lib().sipx_set_data(ctx.h, 1, w.ctypes.data_as(C.c_void_p), None) != 0
        assert "holds no replaceable vectors" in sipx.lib().sipx_last_error().decode()
    finally:
        ctx.close()
    # a slab-decomposed or owned context
    msg = "the weighted l1 ball (l1_weighted) takes single-process contexts only"
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
    # the stand-alone calls refuse what the host refuses
    ctx = sipx.Context(g, TF)
    try:
        out, x = np.zeros(1, TF), np.zeros(N, TF)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        wb = w.copy()
        wb[4] = -2.0
        assert sipx.lib().sipx_l1_weighted_norm(ctx.h, TV, p(x), p(wb), p(out)) != 0
        assert "weight 4 is negative, NaN or infinite" in sipx.lib().sipx_last_error().decode()
        assert sipx.lib().sipx_l1_weighted_norm(ctx.h, OPS["custom"], p(x), p(w), p(out)) != 0
        assert "takes no custom operator" in sipx.lib().sipx_last_error().decode()
        assert sipx.lib().sipx_l1_weighted_norm(ctx.h, TV, p(x), None, p(out)) != 0
        v = np.ones(M, TF)
        assert sipx.lib().sipx_project(ctx.h, C.byref(_desc(sipx, TV, None, count=M)), p(v), C.c_int64(M)) != 0
        assert "needs its weights in lb" in sipx.lib().sipx_last_error().decode()
        assert sipx.lib().sipx_project(ctx.h, C.byref(_desc(sipx, TV, w)), p(v), C.c_int64(M - 1)) != 0
        assert f"{M} entries on this grid, {M - 1} given" in sipx.lib().sipx_last_error().decode()
    finally:
        ctx.close()


def test_passes_are_reported(sipx):
    TF, n, h = np.float32, (32, 24), (25.0, 6.0)
    m = _model(n, TF, seed=7)
    with sipx.Solver(*_args(sipx, "wl1-TV", n, h, TF, m, 1), TF) as S:
        S(m.copy())
        st = S.ctx.kernel_stats_all(-1)
    st1, st21 = st["l1_weighted"], st["l21_weighted"]
    assert 2 <= st1["passes"] <= 2 * 32 * 24 + 1 and st1["flag_reads"] == -(-st1["passes"] // 8) and st1["n"] == 2 * 32 * 24 and st1["calls"] >= 2
    assert st21 == {"passes": 0, "flag_reads": 0, "calls": 0, "groups": 0}, "the weighted l2,1 row counts the weighted l1 set"
