"""One radius per fiber / per slice for the l1 ball, the l2 ball and the annulus (csrc/seg_norm.h, k_seg_norm with rmin / rmax), the
observation kernel behind sipx.segment_norms (k_seg_observe) and the radii as replaceable data of a live context.

Every test runs at the shapes of tests/test_gpu_seg_norms.CASES, which tests/test_seg_norms_cpu.py proves to reach the four paths
{segment, tile} x {LDS, streaming}, a ragged last tile, a segment shorter than a wave and one longer than the workgroup.  The
references are tests/l1_exact.py (l1: the exact threshold per segment) and tests/seg_radii_ref.py (the oracle's whole-vector
projector with the segment's own scalars)."""
import numpy as np
import pytest
import torch      # (before libsipx.so is loaded: one HIP runtime in the process, see host._check_one_hip_runtime)

from oracle import parsdmm_oracle as O
from tests import l1_exact, seg_norms_ref, seg_radii_ref
from tests.test_gpu_seg_norms import (CASES, CLASSES, SOLVE_SETS, _julia_max, _model, _norm_bounds, classify, make_input)
from tests.test_gpu_set_data import _assert_same, _rho_gamma

pytestmark = pytest.mark.gpu

PRECISIONS = [np.float32, np.float64]
SEED = 20250909      # (a draw with which every case holds two segments of every class: tests/test_seg_radii_cpu.py proves it from the reference)
_inputs = {}


def _grid(sipx, n):
    return sipx.compgrid(tuple(1.0 for _ in n), n)


def _P(sipx, st, mn, mx, mode, n, TF):
    c = sipx.set_definitions(st, "identity", mn, mx, mode)
    P, A, prop = sipx.setup_constraints([c], _grid(sipx, n), TF, segment_norms=True)
    assert prop.ncvx == [False]
    return P[0]


# ---- 1. l1: the exact threshold per segment, every segment with its own radius -----------------------------------------------------
def l1_radii(n, mode):
    """b_s = 8 * 2^(q_s - 2), q_s in 0 .. 3: powers of two (2, 4, 8, 16), numbers of both precisions, so the tie segments stay exact."""
    nseg = len(seg_norms_ref.segment_indices(n, mode))
    q = np.random.default_rng(20250907 + sum(n) + ord(mode[1])).integers(0, 4, nseg)
    return 8.0 * 2.0 ** (q - 2.0)


def make_radii_input(n, mode, TF):
    """(v, segment index arrays, radii): tests/test_gpu_seg_norms.make_input with segment s of class CLASSES[s % 5] built against its
    own radius b_s.  Computed once per (n, mode, TF), handed out as a copy."""
    key = (n, mode, np.dtype(TF).name)
    if key not in _inputs:
        rng = np.random.default_rng(SEED + sum(n) + len(mode[1]) + ord(mode[1]))
        segs = seg_norms_ref.segment_indices(n, mode)
        radii = l1_radii(n, mode)
        v = np.zeros(int(np.prod(n)), np.float64)
        for s, ind in enumerate(segs):
            L, b = len(ind), radii[s]
            cls = CLASSES[s % 5]
            if cls in ("feasible", "heavy"):
                h = rng.standard_normal(L) * np.exp(rng.standard_normal(L))
                h *= (0.5 if cls == "feasible" else 2.5) * b / np.abs(h).sum()
                if cls == "heavy" and L >= 4:
                    h[rng.choice(L, max(1, L // 16), replace=False)] = -0.0
                v[ind] = h
            elif cls == "zero":
                z = np.zeros(L)
                z[::2] = -0.0
                v[ind] = z
            elif cls == "all_active":
                v[ind] = (b / L) * (1.5 + 0.1 * rng.random(L)) * rng.choice([-1.0, 1.0], L)
            else:
                k = 4 if L >= 6 else (2 if L >= 4 else 1)     # a power of two: b / k is exact
                t = np.ones(L)
                t[:k] = 1.0 + b / k
                t[k + (L - k) // 2:] = 0.25 if L - k > 2 else 1.0
                v[ind] = rng.permutation(t) * rng.choice([-1.0, 1.0], L)
        _inputs[key] = (v.astype(TF), segs, radii.astype(TF))
    v, segs, radii = _inputs[key]
    return v.copy(), segs, radii.copy()


def radii_class_counts(n, mode, TF):
    """Segments of each class with respect to their own radius, from the reference alone (classify: l1_exact.feasibility, exact_theta)."""
    v, segs, radii = make_radii_input(n, mode, TF)
    counts = dict.fromkeys(CLASSES + ("negzero",), 0)
    for s, ind in enumerate(segs):
        for c in classify(v[ind], radii[s]):
            counts[c] += 1
    return counts


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("n,mode", CASES)
def test_l1_segments_hold_the_exact_threshold_of_their_own_radius(sipx, TF, n, mode):
    v, segs, radii = make_radii_input(n, mode, TF)
    assert len(np.unique(radii)) >= 3
    counts = radii_class_counts(n, mode, TF)
    assert all(c >= 2 for c in counts.values()), counts
    P = _P(sipx, "l1", 0.0, radii, mode, n, TF)
    assert P.seg_radii and P.ub.dtype == TF
    y = P(v.copy())
    for s, ind in enumerate(segs):
        try:
            l1_exact.check_l1_output(v[ind], y[ind], radii[s])
        except AssertionError as e:
            raise AssertionError(f"segment {s} ({CLASSES[s % 5]}, L = {len(ind)}, b = {radii[s]}): {e}") from None
    assert l1_exact.same_bits(P(v.copy()), y), "two calls differ"


# ---- 2. l2 and annulus: all radii distinct -----------------------------------------------------------------------------------------
def l2_radii(n, mode, TF):
    """(v, segs, lo_s, hi_s): lo, hi are the bounds of the scalar test on its input (_norm_bounds: two norms below, two above, away from
    rounding), segment s gets lo (1 + s / nseg) and hi (1 + s / nseg) -- all distinct -- and the segment itself is scaled by the same
    factor, so that it stays on the side of its own radii on which the scalar test has it (with one input for all radii the growing
    radii would swallow the segments above them).  The factor of the segment is rounded to a multiple of 1 / 64, so that the tie
    segments (3, 1 and 1 / 4 times it) keep exact squares and sums, as in the scalar test; the radii are not rounded.  A segment paired
    with another segment's radii is scaled or filled wrongly."""
    key = ("l2", n, mode, np.dtype(TF).name)
    if key not in _inputs:
        v, segs = make_input(n, mode, TF)
        lo, hi = _norm_bounds(v, segs, TF)
        f = 1.0 + np.arange(len(segs)) / len(segs)
        for s, ind in enumerate(segs):
            v[ind] = (v[ind].astype(np.float64) * (np.round(f[s] * 64.0) / 64.0)).astype(TF)
        _inputs[key] = (v, segs, (float(lo) * f).astype(TF), (float(hi) * f).astype(TF))
    v, segs, lo_s, hi_s = _inputs[key]
    return v.copy(), segs, lo_s.copy(), hi_s.copy()


def l2_counts(v, segs, lo_s, hi_s, st):
    nrm = [np.linalg.norm(v[ind].astype(np.float64)) for ind in segs]
    lows = [0.0 if st == "l2" else float(q) for q in lo_s]
    return dict(above=sum(q > float(h) for q, h in zip(nrm, hi_s)), inside=sum(l <= q <= float(h) for q, l, h in zip(nrm, lows, hi_s)),
                zero=sum(q == 0 for q in nrm), below=sum(0 < q < l for q, l in zip(nrm, lows)))


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("st", ["l2", "annulus"])
@pytest.mark.parametrize("n,mode", CASES)
def test_l2_and_annulus_segments_match_the_reference_with_their_own_radii(sipx, TF, st, n, mode):
    v, segs, lo_s, hi_s = l2_radii(n, mode, TF)
    assert len(np.unique(hi_s)) == len(segs) and len(np.unique(lo_s)) == len(segs)
    cnt = l2_counts(v, segs, lo_s, hi_s, st)
    assert cnt["above"] >= 2 and cnt["inside"] >= 2 and cnt["zero"] >= 2 and (st == "l2" or cnt["below"] >= 2), cnt
    P = _P(sipx, st, 0.0 if st == "l2" else lo_s, hi_s, mode, n, TF)
    ref = seg_radii_ref.project_segments(v.copy(), n, mode, st, lo_s, hi_s)
    y = P(v.copy())
    assert np.allclose(y, ref, rtol=4 * np.finfo(TF).eps, atol=0)
    for s, ind in enumerate(segs):
        q = np.linalg.norm(v[ind].astype(np.float64))
        if (0 if st == "l2" else float(lo_s[s])) <= q <= float(hi_s[s]):
            assert l1_exact.same_bits(y[ind], v[ind]), f"segment {s} inside its set was touched"
        if st == "annulus" and q == 0:                               # sigma_min / sqrt(L), exactly, with the segment's own sigma_min
            assert np.all(y[ind] == TF(np.float64(lo_s[s]) / np.sqrt(float(len(ind))))), s
    assert l1_exact.same_bits(P(v.copy()), y), "two calls differ"


# ---- 3. an all-equal vector is the scalar set ------------------------------------------------------------------------------------
@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("st", ["l1", "l2", "annulus"])
@pytest.mark.parametrize("n,mode", CASES)
def test_an_all_equal_vector_gives_the_bits_of_the_scalar_set(sipx, TF, st, n, mode):
    v, segs = make_input(n, mode, TF)
    lo, hi = _norm_bounds(v, segs, TF)
    mn, mx = (0.0, TF(8.0)) if st == "l1" else ((0.0 if st == "l2" else lo), hi)
    nseg = len(segs)
    scalar = _P(sipx, st, float(mn), float(mx), mode, n, TF)(v.copy())
    assert not l1_exact.same_bits(scalar, v)
    forms = [(mn, np.full(nseg, mx, TF))]
    if st == "annulus":
        forms += [(np.full(nseg, mn, TF), np.full(nseg, mx, TF)), (np.full(nseg, mn, TF), mx)]      # a scalar beside a vector: repeated
    for a, b in forms:
        assert l1_exact.same_bits(_P(sipx, st, a, b, mode, n, TF)(v.copy()), scalar), (type(a), type(b))


# ---- 4. segment_norms --------------------------------------------------------------------------------------------------------------
def _ops(n, mode):
    """identity, the difference operator along the segment direction and one across it."""
    names = {0: "D_x", 1: "D_y", 2: "D_z"} if len(n) == 3 else {0: "D_x", 1: "D_z"}
    ax = seg_norms_ref.axis_of(n, mode)
    return ["identity", names[ax], names[(ax + 1) % len(n)]]


def _tdn(n, opn):
    n = list(n)
    if opn != "identity":
        n[{"D_x": 0, "D_y": 1, "D_z": len(n) - 1}[opn]] -= 1
    return tuple(n)


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("n,mode", CASES)
def test_segment_norms_and_the_closure_contract(sipx, TF, n, mode):
    """The observed norms against a float64 reduction of the engine's own A x: relative error at most eps(float32) in Float32 and
    L eps(float64) in Float64 (float64 accumulation, one rounding), exactly 0 for a zero segment.  Then the contract: radii observed on
    x make A x a point the projector does not write.  An all-zero segment observes 0, which no host path takes as an l1 radius: such a
    segment gets the radius 1 (it lies in every ball).  The closure needs A x as an array of its own grid; D_z on (4, 5, 2) leaves one
    plane, which the host reads as a 2-D grid without fibers along z, so that one combination is held to its norms only."""
    g = _grid(sipx, n)
    x, _ = make_input(n, mode, TF)
    dev = torch.device("cuda", 0)
    for opn in _ops(n, mode):
        tdn = _tdn(n, opn)
        s = np.asarray(sipx.TDOperator(opn, g, TF) @ x, TF)
        segs = seg_norms_ref.segment_indices(tdn, mode)
        L = len(segs[0])
        obs = {}
        for norm in ("l1", "l2"):
            got = sipx.segment_norms(x, g, opn, mode, norm)
            want = seg_radii_ref.norms(s, tdn, mode, norm)
            assert got.dtype == TF and got.shape == (len(segs),)
            bound = float(np.finfo(np.float32).eps) if TF == np.float32 else L * float(np.finfo(np.float64).eps)
            nz = want > 0
            err = np.abs(got[nz].astype(np.float64) - want[nz]) / want[nz]
            print(f"segment_norms {n} {mode} {opn} {norm} {np.dtype(TF).name}: max rel. error {err.max() if err.size else 0.0:.3e} (bound {bound:.3e})")
            assert np.all(err <= bound), (opn, norm, float(err.max()), bound)
            assert np.all(got[~nz] == 0)
            if opn == "identity":
                assert (~nz).sum() >= 2
            t = sipx.segment_norms(torch.from_numpy(x).to(dev), g, opn, mode, norm)
            assert t.device == dev and l1_exact.same_bits(t.cpu().numpy(), got)
            obs[norm] = got
        if len(tdn) == 3 and tdn[2] == 1:
            continue
        for st, mn, mx in (("l1", 0.0, np.where(obs["l1"] > 0, obs["l1"], TF(1.0)).astype(TF)), ("l2", 0.0, obs["l2"]),
                           ("annulus", obs["l2"], obs["l2"])):
            y = _P(sipx, st, mn, mx, mode, tdn, TF)(s.copy())
            assert l1_exact.same_bits(y, s), (opn, st)


# ---- 5. the radii as replaceable data of a live context ------------------------------------------------------------------------
KW = dict(maxit=30, evol_rel_tol=0.0, feas_tol=0.0, obj_tol=0.0)      # every iteration runs
LIVE = {
    "l1-slice-z-DxDy": ((24, 20, 6), (25.0, 25.0, 25.0), [("l1", "D_x", ("slice", "z")), ("l1", "D_y", ("slice", "z"))]),
    "l2-fiber-x": ((24, 20), (25.0, 6.0), [("l2", "identity", ("fiber", "x"))]),
}


def _live_setup(sipx, name, TF, k, scalar=False):
    """{bounds, the sets of LIVE[name]}; radius vector k (1 or 2) of a set: the segment's own norm of A m_k times a factor that varies
    with the segment and with k.  -> (args of build_context / Solver, m_k, {set index: radii})."""
    n, h, sets = LIVE[name]
    m = (_model(n, TF, seed=40 + k) * TF(1.0 - 0.03 * k)).astype(TF)
    g = sipx.compgrid(h, n)
    opt = sipx.PARSDMM_options(FL=TF, **KW)
    c = [sipx.set_definitions("bounds", "identity", 1600.0, 3900.0, ("matrix", ""))]
    data = {}
    for i, (st, opn, mode) in enumerate(sets):
        tdn = _tdn(n, opn)
        s = np.asarray(O.get_TD_operator(O.compgrid(h, n), opn, TF)[0] @ m, np.float64)
        nrm = seg_radii_ref.norms(s, tdn, mode, st)
        r = (nrm * (0.4 + 0.1 * k) * (1.0 + 0.5 * np.arange(len(nrm)) / len(nrm))).astype(TF)
        data[i + 1] = r
        c.append(sipx.set_definitions(st, opn, 0.0, float(r.mean()) if scalar else r, mode))
    P, A, prop = sipx.setup_constraints(c, g, TF, segment_norms=True)
    A, AtA, _, _ = sipx.PARSDMM_precompute_distribute(A, prop, g, opt)
    return (AtA, A, prop, P, g, opt), m, data


_fresh_cache = {}


def _fresh(sipx, name, TF, k):
    key = (name, np.dtype(TF).name, k)
    if key not in _fresh_cache:
        (AtA, A, prop, P, g, opt), m, _ = _live_setup(sipx, name, TF, k)
        ctx = sipx.host.build_context(m, AtA, A, prop, P, g, opt)
        try:
            log, _ = ctx.parsdmm(opt)
            x, l, y = ctx.download()
        finally:
            ctx.close()
        for a in [x] + l + y:
            a.setflags(write=False)
        _fresh_cache[key] = (x, l, y, log)
    return _fresh_cache[key]


@pytest.mark.parametrize("TF", PRECISIONS, ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(LIVE))
def test_set_data_with_new_radii_then_reset_gives_the_bits_of_a_new_context(sipx, name, TF):
    args1, m1, data1 = _live_setup(sipx, name, TF, 1)
    _, m2, data2 = _live_setup(sipx, name, TF, 2)
    want1, want2 = _fresh(sipx, name, TF, 1), _fresh(sipx, name, TF, 2)
    assert not np.array_equal(want1[0], want2[0])
    AtA, A, prop, P, g, opt = args1
    assert [p.data_len(a) for p, a in zip(P, A)] == [None] + [len(r) for r in data1.values()]
    rho, gamma = _rho_gamma(opt, TF)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    # the host form
    ctx = sipx.host.build_context(m1, AtA, A, prop, P, g, opt)
    try:
        log, _ = ctx.parsdmm(opt)
        _assert_same(ctx.download() + (log,), want1)
        before = ctx.device_bytes()["context"]
        for i, r in data2.items():
            ctx.set_data(i, ub=r)
        ctx.reset(m2, rho, gamma)
        log, _ = ctx.parsdmm(opt)
        _assert_same(ctx.download() + (log,), want2)
        assert ctx.device_bytes()["context"] == before, "set_data allocated on a finalized context"
    finally:
        ctx.close()
    # the device form through the Solver: nothing crosses PCIe
    with sipx.Solver(*args1, TF) as S:
        x, log, l, y = S(t(m1))
        _assert_same((x, l, y, log), want1)
        io = S.ctx.io_bytes()
        for i, r in data2.items():
            S.set_data(i, ub=t(r))
        x, log, l, y = S(t(m2))
        assert log.context_reused and S.ctx.io_bytes() == io
        _assert_same((x, l, y, log), want2)
    # a first build from device data: the Projectors hold placeholders
    args, _, _ = _live_setup(sipx, name, TF, 1)
    for i in data2:
        args[3][i].ub = np.ones_like(args[3][i].ub)
    with sipx.Solver(*args, TF) as S:
        for i, r in data2.items():
            S.set_data(i, ub=t(r))
        x, log, l, y = S(t(m2))
        assert not log.context_reused
        _assert_same((x, l, y, log), want2)


@pytest.mark.parametrize("name", list(LIVE))
def test_scalar_built_segmented_sets_hold_no_replaceable_vectors(sipx, name):
    TF = np.float32
    (AtA, A, prop, P, g, opt), m, data = _live_setup(sipx, name, TF, 1, scalar=True)
    assert all(p.data_len(a) is None for p, a in zip(P, A))
    ctx = sipx.host.build_context(m, AtA, A, prop, P, g, opt)
    try:
        log, _ = ctx.parsdmm(opt)
        x1 = ctx.download()[0]
        for i, r in data.items():
            with pytest.raises(sipx.SipxError, match=r"holds no replaceable vectors.*build a new context"):
                ctx.set_data(i, ub=r)
        ctx.reset(m, *_rho_gamma(opt, TF))                    # the context stays usable
        log2, _ = ctx.parsdmm(opt)
        assert np.array_equal(ctx.download()[0], x1) and np.array_equal(log2.obj, log.obj)
    finally:
        ctx.close()
    with sipx.Solver(AtA, A, prop, P, g, opt, TF) as S:
        with pytest.raises(sipx.SipxError, match=r"holds no replaceable vectors.*build a new Solver"):
            S.set_data(1, ub=data[1])


# ---- 6. solves against the oracle (cases, rules and tolerances of test_segmented_sets_solve_matches_oracle) --------------------------
RADII_SOLVE_CASES = [(name, (16, 12, 8), (25.0, 25.0, 25.0)) for name in ("l1-fiber-z-Dz", "l1-slice-z-DxDy", "l2-fiber-x")] + \
                    [(name, (32, 24), (25.0, 6.0)) for name in ("l1-fiber-z-Dz", "l2-fiber-x")]


def _solve_problem(mod, name, n, h, TF, m, opt_kw):
    """{bounds, the sets of SOLVE_SETS[name]}; radii: the segment's own norm of A m times 0.5 (1 + 0.5 s / nseg).  The oracle is set up
    with the whole-array form of each set and its projector then replaced by the per-segment reference."""
    g = mod.compgrid(h, n)
    opt = mod.PARSDMM_options(FL=TF, **opt_kw)
    c = [mod.set_definitions("bounds", "identity", 1600.0, 3900.0, ("matrix", ""))]
    swaps = []
    for st, opn, mode in SOLVE_SETS[name]:
        A, _, _, tdn, _ = O.get_TD_operator(O.compgrid(h, n), opn, TF)
        tdn = tuple(int(q) for q in tdn)
        nrm = seg_radii_ref.norms(np.asarray(A @ m, np.float64), tdn, mode, st)
        r = (nrm * 0.5 * (1.0 + 0.5 * np.arange(len(nrm)) / len(nrm))).astype(TF)
        c.append(mod.set_definitions(st, opn, 0.0, float(r.mean()) if mod is O else r, ("matrix", "") if mod is O else mode))
        swaps.append((len(c) - 1, lambda x, tdn=tdn, mode=mode, st=st, r=r: seg_radii_ref.project_segments(x, tdn, mode, st, None, r)))
    if mod is O:
        P, A, prop = mod.setup_constraints(c, g, TF)
        for i, f in swaps:
            P[i] = f
    else:
        P, A, prop = mod.setup_constraints(c, g, TF, segment_norms=True)
    A, AtA, l, y = mod.PARSDMM_precompute_distribute(A, prop, g, opt)
    return g, opt, P, A, prop, AtA


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("name,n,h", RADII_SOLVE_CASES)
def test_solves_with_per_segment_radii_match_the_oracle(sipx, TF, name, n, h):
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


@pytest.mark.parametrize("n,mode", [((16, 12), ("fiber", "z")), ((10, 8, 6), ("slice", "z"))])
def test_single_l1_set_with_per_segment_radii_equals_projector(sipx, n, mode):
    TF = np.float64
    g = _grid(sipx, n)
    opt = sipx.PARSDMM_options(FL=TF, maxit=400, feas_tol=1e-10, obj_tol=1e-10, evol_rel_tol=1e-12)
    m = np.random.default_rng(13).standard_normal(int(np.prod(n)))
    nrm = seg_radii_ref.norms(m, n, mode, "l1")
    r = nrm * 0.4 * (1.0 + 0.5 * np.arange(len(nrm)) / len(nrm))
    ref = seg_radii_ref.project_segments(m.copy(), n, mode, "l1", None, r)
    c = sipx.set_definitions("l1", "identity", 0.0, r, mode)
    P, A, prop = sipx.setup_constraints([c], g, TF, segment_norms=True)
    assert prop.ncvx == [False]
    A, AtA, l, y = sipx.PARSDMM_precompute_distribute(A, prop, g, opt)
    x, log, l, y = sipx.PARSDMM(m.copy(), AtA, A, prop, P, g, opt)
    assert np.linalg.norm(x - ref) / np.linalg.norm(ref) < 1e-7


# ---- 7. radii from device memory that no host path would take; sharded contexts -----------------------------------------------------
def test_an_l1_radius_from_device_memory_that_is_not_positive_zeroes_its_segment(sipx):
    """The host refuses such a vector; from device memory it cannot be looked at.  sipx.h: a segment whose radius is not > 0 (NaN
    included) is set to zero, the projection onto the ball of radius 0; the other segments are projected as usual and the solve ends."""
    TF, n, mode = np.float64, (16, 12), ("fiber", "z")
    g = _grid(sipx, n)
    opt = sipx.PARSDMM_options(FL=TF, maxit=400, feas_tol=1e-10, obj_tol=1e-10, evol_rel_tol=1e-12)
    m = np.random.default_rng(17).standard_normal(int(np.prod(n)))
    segs = seg_norms_ref.segment_indices(n, mode)
    nrm = seg_radii_ref.norms(m, n, mode, "l1")
    r = nrm * 0.4 * (1.0 + 0.5 * np.arange(len(nrm)) / len(nrm))
    bad = {3: 0.0, 5: -1.0, 7: float("nan")}
    good = r.copy()
    ref = seg_radii_ref.project_segments(m.copy(), n, mode, "l1", None, good)
    for s, val in bad.items():
        r[s] = val
        ref[segs[s]] = 0.0
    with pytest.raises(sipx.SipxError, match="Radius of L1 ball is negative"):
        sipx.setup_constraints([sipx.set_definitions("l1", "identity", 0.0, r, mode)], g, TF, segment_norms=True)
    P, A, prop = sipx.setup_constraints([sipx.set_definitions("l1", "identity", 0.0, good, mode)], g, TF, segment_norms=True)
    A, AtA, _, _ = sipx.PARSDMM_precompute_distribute(A, prop, g, opt)
    dev = torch.device("cuda", 0)
    with sipx.Solver(AtA, A, prop, P, g, opt, TF) as S:
        with pytest.raises(sipx.SipxError, match="Radius of L1 ball is negative"):
            S.set_data(0, ub=r)
    with sipx.Solver(AtA, A, prop, P, g, opt, TF) as S:
        S.set_data(0, ub=torch.from_numpy(r).to(dev))
        x, log, _, _ = S(m.copy())
    # (x is the iterate of the x-step, zero there up to the CG tolerance; the segment's y is the projector's own output)
    assert np.all(np.isfinite(x)) and all(np.abs(x[segs[s]]).max() <= 1e-12 for s in bad)
    assert np.linalg.norm(x - ref) / np.linalg.norm(ref) < 1e-7


def test_contexts_with_set_ownership_refuse_vector_radii_and_name_the_way_out(sipx):
    TF, n, mode = np.float32, (16, 12, 8), ("slice", "z")
    g = sipx.compgrid((25.0, 25.0, 25.0), n)
    opt = sipx.PARSDMM_options(FL=TF, maxit=5)
    m = _model(n, TF, seed=3)
    P, A, prop = sipx.setup_constraints([sipx.set_definitions("l2", "identity", 0.0, np.full(8, 1e4), mode),
                                         sipx.set_definitions("l2", "identity", 0.0, 1e4, mode)], g, TF, segment_norms=True)
    A, AtA, _, _ = sipx.PARSDMM_precompute_distribute(A, prop, g, opt)
    ctx = sipx.Context(g, TF)
    try:
        ctx.set_owned([1])
        with pytest.raises(sipx.SipxError, match=r"single-process contexts only.*scalar radius, or a single process"):
            ctx.add_set(A[0], P[0])
        assert ctx.add_set(A[1], P[1]) == 0                    # a scalar segmented set keeps its route
    finally:
        ctx.close()
    with pytest.raises(sipx.SipxError, match=r"scalar radius, or a single process"):       # ownership given after the set: at finalize
        sipx.host.build_context(m, AtA, A, prop, P, g, opt, owned=[1, 1, 1])
