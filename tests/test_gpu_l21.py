"""Isotropic total variation on the GPU: the ("l21", "TV") projector (csrc/l21.h, csrc/ext_group.hip) through sipx.Projector against
tests/l21_ref.py, inputs it must not write, exact ties, the observed radius (sipx.l21_norm), whole solves against the oracle with its
projector swapped for the reference, the device-resident solve and the engine's refusals through the C ABI.

GRIDS: (4,3) and (5,4,3) are the smallest with every boundary class; (33,20) and (20,9,6) have an odd n1 (one point per thread);
(64,48) and (32,12,8) have n1 % 4 == 0 (16 bytes per thread).  The kernels launch min(ceil(points / (256 VW)), 2048) workgroups of
256 threads, VW = 4 (Float32) or 2 (Float64) points per thread on the 16-byte path: one sweep of the launch grid covers 2048 * 256 *
4 = 2 097 152 points in Float32.  (2048, 1028) has 2 105 344: the grid-stride loops take a second, partial sweep in both
precisions -- the 332 800 points of (640, 520) would not."""
import ctypes as C

import numpy as np
import pytest
import torch      # (before libsipx.so is loaded: one HIP runtime in the process)

from oracle import parsdmm_oracle as O
from tests import l1_exact, l21_ref

pytestmark = pytest.mark.gpu

GRIDS = [(4, 3), (5, 4, 3), (33, 20), (20, 9, 6), (64, 48), (32, 12, 8), (2048, 1028)]
FRACS = [0.9, 0.5, 0.05]
_inputs = {}


def _grid(sipx, n):
    return sipx.compgrid(tuple(1.0 for _ in n), n)


def _mode(n):
    return ("matrix", "") if len(n) == 2 else ("tensor", "")


def _P(sipx, n, TF, tau):
    return sipx.Projector(sipx.set_definitions("l21", "TV", 0.0, float(tau), _mode(n)), _grid(sipx, n), TF)


def make_input(n, TF):
    """(v, ||v||_2,1): heavy-tailed randn * exp(randn) on every row of the M-vector; computed once, handed out as a copy."""
    key = (n, np.dtype(TF).name)
    if key not in _inputs:
        rng = np.random.default_rng(20250501 + sum(n))
        M = l21_ref.rows(n)
        v = (rng.standard_normal(M) * np.exp(rng.standard_normal(M))).astype(TF)
        _inputs[key] = (v, l21_ref.norm21(v, n))
    v, nrm = _inputs[key]
    return v.copy(), nrm


def test_the_large_grid_needs_a_second_sweep():
    n = GRIDS[-1]
    assert n[0] % 4 == 0 and int(np.prod(n)) // 4 > 2048 * 256 and (640 * 520) // 4 < 2048 * 256


@pytest.mark.parametrize("TF", [np.float32, np.float64])
@pytest.mark.parametrize("frac", FRACS)
@pytest.mark.parametrize("n", GRIDS)
def test_projector_matches_the_reference(sipx, TF, frac, n):
    v, nrm = make_input(n, TF)
    b = TF(frac * nrm)
    ref = l21_ref.project(v, n, b)
    assert ref is not v
    P = _P(sipx, n, TF, b)
    y = P(v.copy())
    eps = float(np.finfo(TF).eps)
    err = np.abs(y.astype(np.float64) - ref)
    bound = 4 * eps * np.abs(v.astype(np.float64))
    worst = float(np.max(err / np.maximum(np.abs(v.astype(np.float64)), np.finfo(np.float64).tiny)) / eps)
    print(f"l21 {n} {np.dtype(TF).name} frac {frac}: worst error {worst:.3f} eps |v|, zeroed groups "
          f"{int((l21_ref.norms(y, n, TF) == 0).sum())} of {int(np.prod(n))}")
    assert np.all(err <= bound), f"worst error {worst:.3f} eps |v|"
    assert l1_exact.same_bits(P(v.copy()), y), "two calls differ"


# ---- inputs the projector must not write ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("TF", [np.float32, np.float64])
@pytest.mark.parametrize("n", [(33, 20), (32, 12, 8)])
def test_feasible_and_zero_inputs_come_back_bit_for_bit(sipx, TF, n):
    v, nrm = make_input(n, TF)
    v[::7] = -0.0
    v[3::11] = 0.0
    b = TF(2 * l21_ref.norm21(v, n))
    assert l1_exact.feasibility(l21_ref.norms(v, n, TF), b) > 0 and np.any(np.signbit(v) & (v == 0))
    assert l1_exact.same_bits(_P(sipx, n, TF, b)(v.copy()), v)
    z = np.zeros_like(v)
    z[::2] = -0.0
    assert l1_exact.same_bits(_P(sipx, n, TF, b)(z.copy()), z)


# ---- ties: integer components, exact norms in both precisions ------------------------------------------------------------------------------
def _tie_input(n, TF):
    G = l21_ref.groups(n)
    full = np.nonzero((G >= 0).all(axis=1))[0]                    # points with every member
    rng = np.random.default_rng(41)
    pick = rng.permutation(full)
    nd = len(n)
    sevens = [(7, 0), (0, 7), (7, 0), (0, 7)] if nd == 2 else [(7, 0, 0), (0, 7, 0), (0, 0, 7), (0, -7, 0)]
    fives = [(3, 4), (5, 0), (4, -3), (0, 5), (-3, 4), (-5, 0), (4, 3), (0, -5), (3, -4)] if nd == 2 else \
            [(3, 4, 0), (5, 0, 0), (0, 3, 4), (0, 0, -5), (-3, 0, 4), (0, 5, 0), (0, -3, 4), (4, 3, 0), (0, 4, -3), (-4, 0, 3)]
    v = np.zeros(l21_ref.rows(n), TF)
    kind = np.ones(G.shape[0], int)                               # the rest: norm 1
    for p in range(G.shape[0]):
        mem = G[p][G[p] >= 0]
        if len(mem):
            v[mem[p % len(mem)]] = -1.0 if p % 3 == 0 else 1.0
        else:
            kind[p] = 0
    for p, comp in zip(pick, sevens + fives):
        v[G[p]] = comp
        kind[p] = 7 if 7 in np.abs(comp) else 5
    return v, G, kind


@pytest.mark.parametrize("TF", [np.float32, np.float64])
@pytest.mark.parametrize("n", [(9, 7), (8, 6, 5)])
def test_groups_on_the_threshold_are_zeroed(sipx, TF, n):
    v, G, kind = _tie_input(n, TF)
    g = l21_ref.norms(v, n, TF)
    assert np.array_equal(g, kind.astype(TF)) and (kind == 7).sum() == 4 and (kind == 5).sum() >= 8
    b = TF(8.0)
    assert l1_exact.exact_theta(g.astype(np.float64), b)[0] == 5.0
    y = _P(sipx, n, TF, b)(v.copy())
    for k in (5, 1):
        mem = G[kind == k]
        assert np.all(y[mem[mem >= 0]] == 0), f"a group of norm {k} survived"
    mem = G[kind == 7]
    mem = mem[mem >= 0]
    want = v[mem].astype(np.float64) * (2.0 / 7.0)
    assert np.all(np.abs(y[mem] - want) <= 4 * float(np.finfo(TF).eps) * np.abs(v[mem]))
    assert np.count_nonzero(y) == 4


# ---- the observed radius ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("TF", [np.float32, np.float64])
@pytest.mark.parametrize("n", [(33, 20), (64, 48), (20, 9, 6), (32, 12, 8)])
def test_observed_radius_leaves_the_point_unwritten(sipx, TF, n):
    g = sipx.compgrid(tuple(3.0 + a for a in range(len(n))), n)
    x = np.random.default_rng(5 + sum(n)).standard_normal(int(np.prod(n))).astype(TF)
    v = sipx.TDOperator("TV", g, TF) @ x
    tau = sipx.l21_norm(x, g)
    assert isinstance(tau, TF)
    ref = float(np.sum(l21_ref.norms(v, n, TF).astype(l1_exact._WIDE)))
    assert abs(float(tau) - ref) <= 2 * float(np.finfo(TF).eps) * ref
    P = sipx.Projector(sipx.set_definitions("l21", "TV", 0.0, float(tau), _mode(n)), g, TF)
    assert l1_exact.same_bits(P(v.copy()), v), "TV x was written although its radius was observed on x"
    td = sipx.l21_norm(torch.from_numpy(x).cuda(), g)
    assert td.is_cuda and td.shape == (1,) and l1_exact.same_bits(td.cpu().numpy(), np.array([tau], TF))
    # ... and just inside the observed norm the point is projected
    y = sipx.Projector(sipx.set_definitions("l21", "TV", 0.0, float(tau) * 0.999, _mode(n)), g, TF)(v.copy())
    assert not l1_exact.same_bits(y, v)


# ---- whole solves against the oracle (rules and tolerances of test_gpu_seg_norms.py, test_segmented_sets_solve_matches_oracle) -----------
def _model(n, TF, seed):
    rng = np.random.default_rng(20240601 + seed)
    z = np.linspace(0, 1, n[-1]).reshape((1,) * (len(n) - 1) + (-1,))
    return (1500 + 2500 * z + 150 * rng.standard_normal(n)).astype(TF).reshape(-1, order="F")


def _julia_max(v):
    v = np.asarray(v, np.float64)
    return float("nan") if np.isnan(v).any() else float(v.max())


def _project_in_place(x, n, r):
    """l21_ref.project as the oracle calls its projectors: x is overwritten, and returned."""
    y = l21_ref.project(x, n, r)
    if y is not x:
        x[:] = y
    return x


SOLVE_SETS = {"l21-TV": [("l21", "TV")], "l21-TV+l1-Dz": [("l21", "TV"), ("l1", "D_z")]}
SOLVE_CASES = [(name, n, h) for name in SOLVE_SETS for n, h in (((32, 24), (25.0, 6.0)), ((16, 12, 8), (25.0, 25.0, 25.0)))]


def _solve_problem(mod, name, n, h, TF, m, opt_kw):
    """{bounds, the sets of SOLVE_SETS[name]} for module `mod`; tau = half the norm of A m from the reference.  The oracle is set up
    with ("l1", "TV") and its projector then replaced by l21_ref.project."""
    g = mod.compgrid(h, n)
    opt = mod.PARSDMM_options(FL=TF, **opt_kw)
    c = [mod.set_definitions("bounds", "identity", 1600.0, 3900.0, _mode(n))]
    swaps = []
    for st, opn in SOLVE_SETS[name]:
        A = O.get_TD_operator(O.compgrid(h, n), opn, TF)[0]
        s = np.asarray(A @ m, TF)
        if st == "l21":
            r = TF(0.5 * l21_ref.norm21(s, n))
            swaps.append((len(c), lambda x, r=r: _project_in_place(x, n, r)))
        else:
            r = TF(0.5 * np.abs(s.astype(np.float64)).sum())
        c.append(mod.set_definitions("l1" if mod is O else st, opn, 0.0, float(r), _mode(n)))
    P, A, prop = mod.setup_constraints(c, g, TF)
    if mod is O:
        for i, f in swaps:
            P[i] = f
    A, AtA, l, y = mod.PARSDMM_precompute_distribute(A, prop, g, opt)
    return g, opt, P, A, prop, AtA


@pytest.mark.parametrize("TF", [np.float32, np.float64])
@pytest.mark.parametrize("name,n,h", SOLVE_CASES)
def test_l21_solve_matches_oracle(sipx, TF, name, n, h):
    m = _model(n, TF, seed=1 + len(SOLVE_SETS[name]))
    kw = dict(maxit=60)
    go, oo, Po, Ao, propo, AtAo = _solve_problem(O, name, n, h, TF, m, kw)
    gs, os_, Ps, As, props, AtAs = _solve_problem(sipx, name, n, h, TF, m, kw)
    assert props.ncvx == propo.ncvx and props.TD_n == propo.TD_n
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


# ---- the device-resident solve (tests/test_gpu_device_io.py: equality with the host form) -------------------------------------------------
LOG_FIELDS = ("set_feasibility", "r_dual", "r_pri", "r_dual_total", "r_pri_total", "obj", "evol_x", "rho", "gamma", "cg_it", "cg_relres")


def test_device_form_gives_the_bits_of_the_host_form(sipx):
    TF, n, h = np.float32, (32, 24), (25.0, 6.0)
    m = _model(n, TF, seed=3)
    g, opt, P, A, prop, AtA = _solve_problem(sipx, "l21-TV+l1-Dz", n, h, TF, m, dict(maxit=30))
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


# ---- the engine's refusals through the C ABI -----------------------------------------------------------------------------------------------
def _desc(sipx, op, mode=0, pmax=1.0, transform=0, dir=0):
    d = sipx.host._SetDesc()
    d.op, d.proj, d.pmin, d.pmax, d.mode, d.dir, d.transform = op, 14, 0.0, pmax, mode, dir, transform
    return d


def _refused(sipx, ctx, d):
    rc = sipx.lib().sipx_add_set(ctx.h, C.byref(d), None, None, 0)
    assert rc < 0, "the engine took the set"
    return sipx.lib().sipx_last_error().decode()


def test_engine_refusals(sipx):
    TF = np.float32
    TV = sipx.host.OPS["TV"]
    for n in ((16, 12), (16, 12, 8)):
        g = _grid(sipx, n)
        ctx = sipx.Context(g, TF)
        try:
            for op in ("identity", "D_x", "D_z"):
                assert "the l2,1 ball acts on the range of the TV operator: TD_OP must be TV" in _refused(sipx, ctx, _desc(sipx, sipx.host.OPS[op]))
            # (every existing refusal keeps its text: fiber / slice modes on a multi-block operator)
            assert "fiber / slice modes need an operator with one block" in _refused(sipx, ctx, _desc(sipx, TV, mode=1))
            assert "the l2,1 ball acts on the range of the TV operator" in _refused(sipx, ctx, _desc(sipx, 0, mode=1))
            for r in (0.0, -2.0, float("nan")):
                assert _refused(sipx, ctx, _desc(sipx, TV, pmax=r)) == "Radius of L1 ball is negative"
            assert "sets behind the DCT act in their own domain" in _refused(sipx, ctx, _desc(sipx, TV, transform=1))
            assert "sets behind the wavelet transform act in their own domain" in _refused(sipx, ctx, _desc(sipx, TV, transform=2))
            # the other materialised projectors still refuse the operator
            d = _desc(sipx, TV)
            d.proj = sipx.host.PROJ["rank"]
            assert "this projector needs an operator with one block" in _refused(sipx, ctx, d)
            # a set the engine takes: no replaceable vectors; sipx_project refuses any other length
            assert sipx.lib().sipx_add_set(ctx.h, C.byref(_desc(sipx, TV)), None, None, 0) == 0
            ub = np.ones(4, TF)
            assert sipx.lib().sipx_set_data(ctx.h, 0, None, ub.ctypes.data_as(C.c_void_p)) != 0
            assert "holds no replaceable vectors" in sipx.lib().sipx_last_error().decode()
            v = np.zeros(int(np.prod(n)), TF)
            assert sipx.lib().sipx_project(ctx.h, C.byref(_desc(sipx, TV)), v.ctypes.data_as(C.c_void_p), C.c_int64(len(v))) != 0
            assert f"TV range: {l21_ref.rows(n)} entries on this grid, {len(v)} given" in sipx.lib().sipx_last_error().decode()
        finally:
            ctx.close()
        # a context that was given a slab decomposition: at sipx_add_set, or at sipx_finalize when the decomposition came later
        msg = "the l2,1 ball on the TV operator (isotropic total variation) takes single-process contexts only"
        ctx = sipx.Context(g, TF)
        try:
            ctx.set_decomp("slab")
            assert msg in _refused(sipx, ctx, _desc(sipx, TV))
        finally:
            ctx.close()
        ctx = sipx.Context(g, TF)
        try:
            ctx.add_set(sipx.TDOperator("TV", g, TF), _P(sipx, n, TF, 1.0))
            ctx.set_decomp("slab")
            with pytest.raises(sipx.SipxError, match="takes single-process contexts only"):
                ctx.finalize(np.ones(int(np.prod(n)), TF), [10.0], 1.0)
        finally:
            ctx.close()
        ctx = sipx.Context(g, TF)
        try:
            ctx.add_set(sipx.TDOperator("TV", g, TF), _P(sipx, n, TF, 1.0))
            ctx.set_owned([1, 1])
            with pytest.raises(sipx.SipxError, match="takes single-process contexts only"):
                ctx.finalize(np.ones(int(np.prod(n)), TF), [10.0], 1.0)
        finally:
            ctx.close()
