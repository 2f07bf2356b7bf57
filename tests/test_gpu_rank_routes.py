"""The rank projector's subspace routes (csrc/ext_rank.hip: cold ramp, warm-started filtered block iteration, compaction,
inertia certificate, the two warm states) held call by call to the optimal rank-r truncation.

The criterion is tests/rank_exact.py: the distance of an output to the best rank-r matrix (`excess`) and to rank r
(`rankdefect`), both relative to the input slice -- continuous in the input where the truncated matrix itself is not (ties).
The bound per slice is tau = 4 max(defect of oracle.project_rank on the same input, unit roundoff); at the strict acceptance
level (SIPX_RANK_STRICT=1) the oracle term is dropped.  The strict level is a claim of the Float32 Gram route only: the Float64
control (one-sided Jacobi SVD, no route) keeps the oracle term under both settings.  Reference: src/projectors/project_rank!.jl:3-48,
src/projectors/project_nuclear!.jl:3-62, src/update_y_l.jl:64-78."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import parsdmm_oracle as O      # checker only
from tests import rank_exact as R

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
A3, B3 = (72, 76, 5), (128, 128, 6)
Z = ("slice", "z")
MAT = ("matrix", "")


# ---- the stand-alone projector with its route counters -------------------------------------------------------------------------
def cold_call(sipx, kind, n, TF, pmax, mode, v):
    """host.Projector.__call__ (sipx_project: always a cold start), plus the context's rank_route counters."""
    H = sipx.host
    g = sipx.compgrid(tuple(1.0 for _ in n), n)
    P = H.Projector(sipx.set_definitions(kind, "identity", 0, pmax, mode), g, TF)
    ctx = H.Context(g, TF)
    try:
        P.check_rows(H.TDOperator("identity", g, TF))
        d = P.desc("identity", False)
        out = v.copy()
        H._chk(H.lib().sipx_project(ctx.h, C.byref(d), H._ptr(out), C.c_int64(len(out))))
        rr = ctx.kernel_stats_all(-1)["rank_route"]
    finally:
        ctx.close()
    return out, rr


# ---- section 2: the inputs of the cold calls -----------------------------------------------------------------------------------
def _gap_slices(shape, nsl, r, rng, **kw):
    return [R.gapped(shape, r, rng, **kw) for _ in range(nsl)]


def _spectrum(case, n, rng):
    """(slices, r, output must equal the input) of spectrum case 1-8 on the grid n.  r = 2 on 72 x 76 (b = 18: the routes are on
    from k = 72), r = 3 on 128 x 128; case 3 has the r = 4 the issue gives it (on 72 x 76 that is the full decomposition)."""
    shape, nsl = n[:2], n[2]
    r = 2 if min(shape) < 76 else 3
    if case == "1-gap":
        return _gap_slices(shape, nsl, 3, rng), r, False
    if case == "2-flat":
        return [R.flat(shape, rng) for _ in range(nsl)], r, False
    if case == "3-exact-rank2-r4":
        return [R.exact_rank2(shape, rng) for _ in range(nsl)], 4, True
    if case == "4-tie":
        return [R.tied(shape, rng, r) for _ in range(nsl)], r, False
    if case == "5-zero-slices":
        s = _gap_slices(shape, nsl, 3, rng)
        s[0][:] = 0.0; s[3][:] = 0.0
        return s, r, False
    if case == "6-mixed":
        mk = (lambda: R.gapped(shape, 3, rng), lambda: R.flat(shape, rng), lambda: R.exact_rank2(shape, rng))
        return [mk[i % 3]() for i in range(nsl)], r, False
    if case == "7-scaled-1e-12":
        return _gap_slices(shape, nsl, 3, rng, scale=1e-12), r, False
    if case == "7-scaled-1e+12":
        return _gap_slices(shape, nsl, 3, rng, scale=1e12), r, False
    if case == "8-single-entry":
        s = _gap_slices(shape, nsl, 3, rng)
        s[0] = R.single_entry(shape, rng); s[2] = R.single_entry(shape, rng, -7.0)
        return s, r, False
    raise KeyError(case)


SPECTRA = ["1-gap", "2-flat", "3-exact-rank2-r4", "4-tie", "5-zero-slices", "6-mixed", "7-scaled-1e-12", "7-scaled-1e+12",
           "8-single-entry"]

# name -> (grid, application mode, r, what the counters must say: "off" = routes off (full decomposition), "on", "identity" = r >= k)
SHAPES = {
    "k71-r2": ((71, 80), MAT, 2, "off"), "k72-r2": ((72, 80), MAT, 2, "on"),
    "k103-r2": ((103, 110), MAT, 2, "on"), "k104-r2": ((104, 110), MAT, 2, "on"),       # 16 against 24 guard columns
    "256-r40": ((256, 256), MAT, 40, "on"), "256-r41": ((256, 256), MAT, 41, "on"),     # b = 64, then back to 16 guards: b = 57
    "r=k": ((72, 76), MAT, 72, "identity"), "r=k-1": ((72, 76), MAT, 71, "off"),
    "tall-200x72": ((200, 72), MAT, 2, "on"), "wide-72x200": ((72, 200), MAT, 2, "on"),      # right against left Gram matrix
    "slice-z": ((72, 76, 5), Z, 2, "on"), "slice-x": ((5, 72, 76), ("slice", "x"), 2, "on"),
    "slice-y": ((72, 5, 76), ("slice", "y"), 2, "on"),
    "batch-1": ((72, 76, 1), Z, 2, "on"), "batch-3": ((72, 76, 3), Z, 2, "on"), "batch-9": ((72, 76, 9), Z, 2, "on"),
}


@functools.lru_cache(maxsize=None)
def _case(name, TF):
    """(x, grid, mode, r, oracle output, expectation, output must equal the input): built once, shared by both acceptance levels."""
    rng = np.random.default_rng(hash_name(name))
    same = False
    if name in SHAPES:
        n, mode, r, expect = SHAPES[name]
        if len(n) == 2:
            x = R.gapped(n, r if r in (40, 41) else 3, rng).reshape(-1, order="F")       # (rank 3 + noise; rank r for the large r)
        else:
            d = mode[1]
            shape = tuple(v for i, v in enumerate(n) if i != {"x": 0, "y": 1, "z": 2}[d])
            nsl = n[{"x": 0, "y": 1, "z": 2}[d]]
            x = R.stack(_gap_slices(shape, nsl, 3, rng), d)
    else:
        grid, case = name.split(":")
        n, mode, expect = {"A": A3, "B": B3}[grid], Z, "on"
        sl, r, same = _spectrum(case, n, rng)
        x = R.stack(sl)
    x = np.ascontiguousarray(x.astype(TF))
    x.setflags(write=False)
    yo = O.project_rank(x.copy(), r, n, mode)
    yo.setflags(write=False)
    return x, n, mode, r, yo, expect, same


def hash_name(name):
    return int.from_bytes(name.encode(), "little") % (2 ** 31)


def _hold_cold(sipx, name, TF, strict):
    x, n, mode, r, yo, expect, same = _case(name, TF)
    y, rr = cold_call(sipx, "rank", n, TF, r, mode, x)
    recs = R.check_rank_output(x, y, yo, r, n, mode, TF, strict=strict and TF == F32, label=name)
    for rec in recs:
        print(name, "strict" if strict else "default", {k: (float("%.3g" % v) if isinstance(v, float) else v) for k, v in rec.items()}, rr)
    for X, Y in zip(R.slices_of(x, n, mode), R.slices_of(y, n, mode)):
        if not X.any():
            assert not Y.any(), name                           # a zero slice comes back as exact zeros
    if same:                                                   # exact rank below r: the output is the input
        for X, Y, rec in zip(R.slices_of(x, n, mode), R.slices_of(y, n, mode), recs):
            assert np.linalg.norm(Y - X) <= rec["tau"] * np.linalg.norm(X), name
    # the counters: `calls` counts every call that enters the Gram route (Float32, something to truncate)
    if TF == F64 or expect == "identity":
        assert rr["calls"] == 0 and rr["warm_started_subspace"] == 0 and rr["full_decomposition"] == 0, rr
    else:
        assert rr["calls"] == 1 and rr["warm_started_subspace"] + rr["full_decomposition"] == 1, rr
        if expect == "off":
            assert rr["warm_started_subspace"] == 0 and rr["products_with_gram"] == 0, rr
    if expect == "identity":
        assert np.array_equal(y, x)
    return recs, rr


@pytest.mark.parametrize("strict", ["0", "1"])
@pytest.mark.parametrize("name", list(SHAPES) + [g + ":" + c for g in "AB" for c in SPECTRA])
def test_cold_call(sipx, monkeypatch, name, strict):
    """One stand-alone call (a cold start) per shape threshold, orientation, slice direction, batch size and spectrum."""
    monkeypatch.setenv("SIPX_RANK_STRICT", strict)
    _hold_cold(sipx, name, F32, strict == "1")


@pytest.mark.parametrize("strict", ["0", "1"])
def test_cold_call_float64_control(sipx, monkeypatch, strict):
    """Float64 takes the one-sided Jacobi SVD, never a route: the control of the measure itself."""
    monkeypatch.setenv("SIPX_RANK_STRICT", strict)
    _hold_cold(sipx, "A:1-gap", F64, strict == "1")


@pytest.mark.parametrize("strict", ["0", "1"])
@pytest.mark.parametrize("name", ["A:5-zero-slices", "A:6-mixed", "B:5-zero-slices", "B:6-mixed"])
def test_cold_call_without_compaction(sipx, monkeypatch, name, strict):
    """SIPX_RANK_PACK=0 (every filter on the whole batch): the same bounds.  Bit equality with the packed route is not asked
    for -- the library may pick another GEMM kernel for another batch size."""
    monkeypatch.setenv("SIPX_RANK_STRICT", strict)
    monkeypatch.setenv("SIPX_RANK_PACK", "0")
    _hold_cold(sipx, name, F32, strict == "1")


def test_cold_calls_take_the_ramp_and_the_full_decomposition(sipx, monkeypatch):
    """The counters of three calls: routes off (k = 71) -- the full decomposition; a gap behind the block -- the ramp from a
    cold start is accepted; an all-zero batch -- nothing to project, counted as served without a decomposition."""
    monkeypatch.setenv("SIPX_RANK_STRICT", "0")
    _, rr = _hold_cold(sipx, "k71-r2", F32, False)
    assert rr["full_decomposition"] == 1
    _, rr = _hold_cold(sipx, "B:1-gap", F32, False)
    assert rr["warm_started_subspace"] == 1 and rr["products_with_gram"] > 0, rr
    z = np.zeros(int(np.prod(A3)), F32)
    y, rr = cold_call(sipx, "rank", A3, F32, 2, Z, z)
    assert not y.any() and rr["calls"] == 1 and rr["full_decomposition"] == 0, rr


# ---- section 3: warm calls, iteration by iteration inside a solve --------------------------------------------------------------
MAXIT = 31
LO, HI = 1000.0, 4500.0


def _pattern(shape, rank, rng, amp=300.0, noise=2.0):
    """A velocity-like slice: a constant, `rank` directions far above white noise (the constant is one more direction)."""
    U, V = rng.standard_normal((shape[0], rank)), rng.standard_normal((rank, shape[1]))
    return 2500.0 + amp * (U @ V) / rank + noise * rng.standard_normal(shape)


def _model(name):
    """(m, grid, slice direction, r, family)"""
    rng = np.random.default_rng(hash_name(name))
    if name == "gap-r2":
        n, d, r = A3, "z", 2
        sl = [_pattern(n[:2], 1, rng) for _ in range(n[2])]
    elif name == "flat-r2":
        n, d, r = A3, "z", 2
        sl = [1500.0 + 2500.0 * k / (n[2] - 1) + 150.0 * rng.standard_normal(n[:2]) for k in range(n[2])]
    elif name == "gap-r3-slice-x":
        n, d, r = (5, 80, 84), "x", 3                 # (b = 19: the routes need k >= 76)
        sl = [_pattern((80, 84), 2, rng) for _ in range(5)]
    elif name == "gap-128-r8":
        n, d, r = B3, "z", 8
        sl = [_pattern(n[:2], 7, rng) for _ in range(n[2])]
    elif name == "gap-constant-slices":
        n, d, r = A3, "z", 2
        sl = [_pattern(n[:2], 1, rng) for _ in range(n[2])]
        sl[0][:] = 2500.0; sl[3][:] = 3100.0
    else:
        raise KeyError(name)
    return R.stack(sl, d).astype(F32), n, d, r, name.split("-")[0]


MODELS = ["gap-r2", "flat-r2", "gap-r3-slice-x", "gap-128-r8", "gap-constant-slices"]


def _problem(sipx, n, d, r):
    g = sipx.compgrid((10.0, 10.0, 10.0), n)
    c = [sipx.set_definitions("bounds", "identity", LO, HI, ("matrix", "")),
         sipx.set_definitions("rank", "identity", 0, r, ("slice", d))]
    opt = sipx.PARSDMM_options(FL=F32, maxit=MAXIT, adjust_rho=False, adjust_gamma=False)
    opt.evol_rel_tol = opt.feas_tol = opt.obj_tol = 0.0                  # run all iterations
    P, A, prop = sipx.setup_constraints(c, g, F32)
    A, AtA, l, y = sipx.PARSDMM_precompute_distribute(A, prop, g, opt)
    return g, opt, P, A, prop, AtA


RK = 1          # the rank set among (bounds, rank, distance)
_SOLVES = {}


def _run_solve(sipx, name, strict):
    """Steps the solve one iteration at a time; every y of the rank set is held against the input update_y_l handed the
    projector (oracle.update_y_l: gamma x_t + (1 - gamma) y_{t-1} - l_{t-1} / rho, rebuilt in float64 from the downloads and
    the logged rho, gamma), every logged feasibility of the rank set against the exact truncation of the downloaded x."""
    key = (name, strict)
    if key in _SOLVES:
        return _SOLVES[key]
    m, n, d, r, family = _model(name)
    mode = ("slice", d)
    g, opt, P, A, prop, AtA = _problem(sipx, n, d, r)
    bad, recs, feas = [], [], []
    ctx = sipx.host.build_context(m, AtA, A, prop, P, g, opt)
    try:
        c0 = ctx.kernel_stats_all(-1)["rank_route"]
        ctx.parsdmm_begin(opt)
        log = ctx._run[2]
        _, l_prev, y_prev = ctx.download()
        for t in range(1, MAXIT + 1):
            ctx.parsdmm_steps(1)
            x, l, y = ctx.download()
            rho, gam = float(log["rho"][t - 1, RK]), float(log["gamma"][t - 1, RK])
            assert rho > 0.0 and gam == 0.75, (t, rho, gam)           # (a non-convex set: gamma = 0.75 and stays, PARSDMM_initialize.jl:107-114)
            vin = gam * x.astype(F64) + (1.0 - gam) * y_prev[RK].astype(F64) - l_prev[RK].astype(F64) / rho
            vin32 = vin.astype(F32)
            yo = O.project_rank(vin32.copy(), r, n, mode)
            rs = R.check_rank_output(vin, y[RK], yo, r, n, mode, F32, strict=strict, label="%s it %d" % (name, t), x_oracle=vin32,
                                     collect=bad)
            for rec in rs:
                rec["it"] = t
            recs += rs
            if t % 10 == 0:
                # ||P(s) - s|| / (||s|| + 100 eps) of the w = 1 state against the exact truncation; per slice the two differ by
                # excess * ||X||, so the whole by at most the taus of the slices summed in quadrature
                s64 = x.astype(F64)
                so = O.project_rank(x.copy(), r, n, mode)
                num2 = bound2 = 0.0
                for Xs, Ys in zip(R.slices_of(s64, n, mode), R.slices_of(so, n, mode)):
                    num2 += float(np.linalg.norm(R.truncate(Xs, r) - Xs)) ** 2
                    bound2 += (R.tau(Xs, Ys, r, F32, strict) * float(np.linalg.norm(Xs))) ** 2
                den = float(np.linalg.norm(s64)) + 100.0 * float(np.finfo(F32).eps)
                feas.append(dict(it=t, exact=np.sqrt(num2) / den, bound=np.sqrt(bound2) / den))
            l_prev, y_prev = l, y
        c1 = ctx.kernel_stats_all(-1)["rank_route"]
        for f in feas:
            f["logged"] = float(log["set_feasibility"][f["it"] // 10, RK])
    finally:
        ctx.close()
    out = dict(bad=bad, recs=recs, feas=feas, family=family, counters={k: c1[k] - c0[k] for k in c1}, before=c0)
    _SOLVES[key] = out
    return out


@pytest.mark.parametrize("strict", ["0", "1"])
@pytest.mark.parametrize("name", MODELS)
def test_every_warm_call_of_a_solve(sipx, monkeypatch, name, strict):
    """31 iterations, no step, slice or case exempt.  The counters: 31 prox calls (state w = 0) and the three feasibility
    estimates of iterations 10, 20, 30 (state w = 1, restarted from vectors ten iterations old); the warm route ran."""
    monkeypatch.setenv("SIPX_RANK_STRICT", strict)
    res = _run_solve(sipx, name, strict == "1")
    worst = max(res["recs"], key=lambda q: max(q["excess"], q["rankdefect"]) / q["tau"] if q["tau"] else 0.0)
    print(name, "strict" if strict == "1" else "default", "worst of", len(res["recs"]), "slices:", worst, res["counters"], res["feas"])
    assert not res["bad"], res["bad"][:10]
    assert len(res["recs"]) == MAXIT * 5 or len(res["recs"]) == MAXIT * 6
    cnt = res["counters"]
    assert cnt["calls"] == MAXIT + 3, (cnt, res["before"])
    assert cnt["warm_started_subspace"] + cnt["full_decomposition"] == cnt["calls"] and cnt["warm_started_subspace"] >= 1, cnt
    assert [f["it"] for f in res["feas"]] == [10, 20, 30]
    for f in res["feas"]:
        assert abs(f["logged"] - f["exact"]) <= f["bound"] + 2.0 ** -23 * f["exact"], f      # (the log holds Float32 values)


@pytest.mark.parametrize("strict", ["0", "1"])
def test_the_warm_route_carries_the_gap_family(sipx, monkeypatch, strict):
    monkeypatch.setenv("SIPX_RANK_STRICT", strict)
    calls = warm = 0
    for name in MODELS:
        if name.startswith("gap"):
            cnt = _run_solve(sipx, name, strict == "1")["counters"]
            calls += cnt["calls"]; warm += cnt["warm_started_subspace"]
    assert 2 * warm >= calls, (warm, calls)


LOG_FIELDS = ("set_feasibility", "r_dual", "r_pri", "r_dual_total", "r_pri_total", "obj", "evol_x", "rho", "gamma", "cg_it", "cg_relres")


def test_reset_forgets_both_warm_states(sipx, monkeypatch):
    """sipx_reset on a context whose rank projector carries the subspaces of another model (ExtProj::reset): the solve that
    follows gives the bits of a newly built context -- x, l, y and the whole log."""
    monkeypatch.setenv("SIPX_RANK_STRICT", "0")
    mA, n, d, r, _ = _model("gap-r2")
    mB = _model("flat-r2")[0]
    g, opt, P, A, prop, AtA = _problem(sipx, n, d, r)
    ref = sipx.host.build_context(mB, AtA, A, prop, P, g, opt)
    try:
        log_ref, _ = ref.parsdmm(opt)
        x_ref, l_ref, y_ref = ref.download()
        cnt_ref = ref.kernel_stats_all(-1)["rank_route"]
    finally:
        ref.close()
    ctx = sipx.host.build_context(mA, AtA, A, prop, P, g, opt)
    try:
        ctx.parsdmm(opt)
        assert ctx.kernel_stats_all(-1)["rank_route"]["warm_started_subspace"] >= 1          # there is a state to forget
        ctx.reset(mB, [float(F32(v)) for v in opt.rho_ini], float(F32(opt.gamma_ini)))
        log, _ = ctx.parsdmm(opt)
        x, l, y = ctx.download()
        cnt = ctx.kernel_stats_all(-1)["rank_route"]
    finally:
        ctx.close()
    assert np.array_equal(x, x_ref)
    for a, b in zip(l + y, l_ref + y_ref):
        assert np.array_equal(a, b)
    for f in LOG_FIELDS:
        a, b = np.asarray(getattr(log, f)), np.asarray(getattr(log_ref, f))
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), f
    assert cnt["warm_started_subspace"] == cnt_ref["warm_started_subspace"] and cnt["products_with_gram"] == cnt_ref["products_with_gram"]


# ---- section 4: the nuclear-norm ball on the same shapes -----------------------------------------------------------------------
def _nuc(X):
    return float(np.linalg.svd(X, compute_uv=False).sum())


@pytest.mark.parametrize("case", ["exact-rank2", "zero-slice", "one-inside", "one-singular-value"])
def test_nuclear_ball_on_route_sized_slices(sipx, case):
    """The Gram route of k_nuc_factors divides by sigma_j: zero eigenvalues, a zero slice, a slice that must stay as it is
    (flag = 0), a radius that leaves one singular value.  oracle.project_nuclear at the 2e-5 of test_rank_and_nuclear_slice_modes."""
    rng = np.random.default_rng(hash_name(case))
    n, shape = A3, A3[:2]
    if case == "exact-rank2":
        sl = [R.exact_rank2(shape, rng) for _ in range(5)]
        sigma = 0.5 * min(_nuc(S) for S in sl)
    elif case == "zero-slice":
        sl = _gap_slices(shape, 5, 3, rng)
        sl[2][:] = 0.0
        sigma = 0.5 * min(_nuc(S) for S in sl if S.any())
    elif case == "one-inside":
        sl = _gap_slices(shape, 5, 3, rng)
        sl[3] *= 0.01
        sigma = 0.5 * min(_nuc(S) for i, S in enumerate(sl) if i != 3)
        assert _nuc(sl[3]) < 0.5 * sigma
    else:
        sl = _gap_slices(shape, 5, 3, rng)                    # sigma = 1, 0.75, 0.5, noise: theta = 1 - 0.2 stays above sigma_2
        sigma = 0.2
    x = R.stack(sl).astype(F32)
    want = O.project_nuclear(x.copy(), F32(sigma), n, Z)
    got, _ = cold_call(sipx, "nuclear", n, F32, sigma, Z, x)
    assert np.linalg.norm(got.astype(F64) - want) <= 2e-5 * np.linalg.norm(want), case
    G, X = R.slices_of(got, n, Z), R.slices_of(x, n, Z)
    if case == "zero-slice":
        assert not G[2].any()
    if case == "one-inside":
        assert np.array_equal(G[3], X[3])                     # inside the ball: bit for bit
        assert not np.array_equal(G[2], X[2])
    if case == "one-singular-value":
        for Y in G:
            s = np.linalg.svd(Y, compute_uv=False)
            assert s[1] <= 2e-5 * s[0] and abs(s.sum() - sigma) <= 50 * 2e-5 * sigma
    if case != "one-inside":
        for Y in G:
            if Y.any():
                assert abs(_nuc(Y) - sigma) <= 50 * 2e-5 * sigma          # on the sphere, as test_rank_and_nuclear_slice_modes asks
