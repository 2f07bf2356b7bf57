"""l1 ball, l2 ball and annulus per fiber / per slice (csrc/seg_norm.h) on the GPU: the projector through sipx.Projector on the
identity against the exact threshold of tests/l1_exact.py (l1) and against the oracle's whole-vector projectors applied per segment
(tests/seg_norms_ref.py: l2, annulus), and whole solves against the oracle with its projector swapped for that reference.

CASES are chosen so that tests/test_seg_norms_cpu.py proves, from the kernel's own plan function, that they reach the four paths
{segment, tile} x {LDS, streaming} in both precisions, a ragged last tile, a segment shorter than a wave and one longer than the
workgroup.  Every case has at least ten segments: each input mixes five classes of segments, two of each at least."""
import numpy as np
import pytest

from oracle import parsdmm_oracle as O
from tests import l1_exact, seg_norms_ref

pytestmark = pytest.mark.gpu

# (grid, application mode)
CASES = [
    ((33, 6, 5), ("fiber", "x")),
    ((300, 4, 3), ("fiber", "x")),
    ((5, 7, 33), ("fiber", "y")),
    ((5, 7, 33), ("fiber", "z")),
    ((70, 3, 300), ("fiber", "z")),
    ((96, 96, 10), ("slice", "z")),
    ((10, 96, 96), ("slice", "x")),
    ((96, 10, 96), ("slice", "y")),
    ((40, 28), ("fiber", "x")),
    ((40, 28), ("fiber", "z")),
    ((4, 5, 2), ("fiber", "z")),
]
RADIUS = 8.0          # the l1 radius of every case: a number of both precisions, so the tie segments below are exact
CLASSES = ("feasible", "heavy", "zero", "all_active", "ties")
_inputs = {}


def make_input(n, mode, TF):
    """(v, segment index arrays); segment s is of class CLASSES[s % 5] with respect to the l1 ball of radius RADIUS:
    feasible     heavy-tailed, ||.||_1 = b / 2
    heavy        heavy-tailed randn * exp(randn), ||.||_1 = 2.5 b, with entries of -0.0
    zero         all zero, some of them -0.0
    all_active   every entry stays active: (b / L) (1.5 + 0.1 u), the reference's lv - 1 cap decides
    ties         k entries of 1 + b / k and a group of ones: theta is exactly 1, the group sits on the threshold
    The array is computed once per (n, mode, TF) and handed out as a copy."""
    key = (n, mode, np.dtype(TF).name)
    if key not in _inputs:
        rng = np.random.default_rng(20250301 + sum(n) + len(mode[1]) + ord(mode[1]))
        segs = seg_norms_ref.segment_indices(n, mode)
        v = np.zeros(int(np.prod(n)), np.float64)
        b = RADIUS
        for s, ind in enumerate(segs):
            L = len(ind)
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
        _inputs[key] = (v.astype(TF), segs)
    v, segs = _inputs[key]
    return v.copy(), segs


def classify(seg, b):
    """Classes of one segment from the reference alone (l1_exact.feasibility, exact_theta)."""
    out = set()
    a = np.abs(seg.astype(np.float64))
    fz = l1_exact.feasibility(seg, b)
    if not a.any():
        out.add("zero")
    elif fz > 0:
        out.add("feasible")
    if np.any(np.signbit(seg) & (seg == 0)):
        out.add("negzero")
    if fz < 0:
        th, C, _ = l1_exact.exact_theta(a, b)
        if a.min() > (a.sum() - float(b)) / len(a):
            out.add("all_active")                             # Michelot's first theta leaves every entry active
        elif np.any(a == th):
            out.add("ties")
        elif 1 <= C < len(a):
            out.add("heavy")
    return out


def class_counts(n, mode, TF):
    v, segs = make_input(n, mode, TF)
    counts = dict.fromkeys(CLASSES + ("negzero",), 0)
    for ind in segs:
        for c in classify(v[ind], TF(RADIUS)):
            counts[c] += 1
    return counts


def _grid(sipx, n):
    return sipx.compgrid(tuple(1.0 for _ in n), n)


def _P(sipx, st, mn, mx, mode, n, TF):
    return sipx.Projector(sipx.set_definitions(st, "identity", mn, mx, mode), _grid(sipx, n), TF)


@pytest.mark.parametrize("TF", [np.float32, np.float64])
@pytest.mark.parametrize("n,mode", CASES)
def test_l1_segments_hold_the_exact_threshold(sipx, TF, n, mode):
    v, segs = make_input(n, mode, TF)
    b = TF(RADIUS)
    counts = class_counts(n, mode, TF)
    assert all(c >= 2 for c in counts.values()), counts
    P = _P(sipx, "l1", 0.0, float(b), mode, n, TF)
    y = P(v.copy())
    for s, ind in enumerate(segs):
        try:
            l1_exact.check_l1_output(v[ind], y[ind], b)
        except AssertionError as e:
            raise AssertionError(f"segment {s} ({CLASSES[s % 5]}, L = {len(ind)}): {e}") from None
    assert l1_exact.same_bits(P(v.copy()), y), "two calls differ"


def _norm_bounds(v, segs, TF):
    """(sigma_min, sigma_max) as TF numbers: two of the non-zero segments' norms below, two above, the rest inside, away from rounding."""
    nrm = np.unique([np.linalg.norm(v[ind].astype(np.float64)) for ind in segs if v[ind].any()])      # (the tie segments share one)
    assert len(nrm) >= 6
    lo, hi = TF(np.sqrt(nrm[1] * nrm[2])), TF(np.sqrt(nrm[-3] * nrm[-2]))
    eps = float(np.finfo(TF).eps)
    assert nrm[1] * (1 + 8 * eps) < float(lo) < nrm[2] * (1 - 8 * eps) and nrm[-3] * (1 + 8 * eps) < float(hi) < nrm[-2] * (1 - 8 * eps)
    return lo, hi


@pytest.mark.parametrize("TF", [np.float32, np.float64])
@pytest.mark.parametrize("st", ["l2", "annulus"])
@pytest.mark.parametrize("n,mode", CASES)
def test_l2_and_annulus_segments_match_the_reference(sipx, TF, st, n, mode):
    v, segs = make_input(n, mode, TF)
    lo, hi = _norm_bounds(v, segs, TF)
    if st == "l2":
        fun = lambda x: O.project_l2(x, hi)
        P = _P(sipx, "l2", 0.0, float(hi), mode, n, TF)
    else:
        fun = lambda x: O.project_annulus(x, lo, hi)
        P = _P(sipx, "annulus", float(lo), float(hi), mode, n, TF)
    ref = seg_norms_ref.project_segments(v.copy(), n, mode, fun)
    y = P(v.copy())
    assert np.allclose(y, ref, rtol=4 * np.finfo(TF).eps, atol=0)
    nrm = [np.linalg.norm(v[ind].astype(np.float64)) for ind in segs]
    inside = [ind for ind, q in zip(segs, nrm) if (0 if st == "l2" else float(lo)) <= q <= float(hi)]
    zero = [ind for ind, q in zip(segs, nrm) if q == 0]
    assert len(inside) >= 2 and len(zero) >= 2 and sum(q > float(hi) for q in nrm) >= 2
    assert all(l1_exact.same_bits(y[ind], v[ind]) for ind in inside), "a segment inside the set was touched"
    if st == "annulus":
        assert sum(0 < q < float(lo) for q in nrm) >= 2
        for ind in zero:                                            # sigma_min / sqrt(L), exactly
            assert l1_exact.same_bits(y[ind], ref[ind]) and np.all(y[ind] == TF(np.float64(lo) / np.sqrt(float(len(ind)))))
    assert l1_exact.same_bits(P(v.copy()), y), "two calls differ"


# ---- one set on the identity: PARSDMM(m) == P(m) (test_gpu_parity.py, test_single_identity_set_equals_projector) -----------------
@pytest.mark.parametrize("n,mode", [((16, 12), ("fiber", "z")), ((10, 8, 6), ("slice", "z"))])
def test_single_segmented_l1_set_equals_projector(sipx, n, mode):
    TF = np.float64
    g = _grid(sipx, n)
    opt = sipx.PARSDMM_options(FL=TF, maxit=400, feas_tol=1e-10, obj_tol=1e-10, evol_rel_tol=1e-12)
    m = np.random.default_rng(13).standard_normal(int(np.prod(n)))
    segs = seg_norms_ref.segment_indices(n, mode)
    b = 0.4 * float(np.mean([np.abs(m[ind]).sum() for ind in segs]))
    ref = seg_norms_ref.project_segments(m.copy(), n, mode, lambda x: O.project_l1_Duchi(x, b))
    c = sipx.set_definitions("l1", "identity", 0.0, b, mode)
    P, A, prop = sipx.setup_constraints([c], g, TF, segment_norms=True)
    assert prop.ncvx == [False]
    A, AtA, l, y = sipx.PARSDMM_precompute_distribute(A, prop, g, opt)
    x, log, l, y = sipx.PARSDMM(m.copy(), AtA, A, prop, P, g, opt)
    assert np.linalg.norm(x - ref) / np.linalg.norm(ref) < 1e-7


# ---- whole solves against the oracle (rules and tolerances of test_gpu_parity.py, test_parsdmm_matches_oracle) -------------------
def _model(n, TF, seed):
    rng = np.random.default_rng(20240601 + seed)
    z = np.linspace(0, 1, n[-1]).reshape((1,) * (len(n) - 1) + (-1,))
    return (1500 + 2500 * z + 150 * rng.standard_normal(n)).astype(TF).reshape(-1, order="F")


def _julia_max(v):
    v = np.asarray(v, np.float64)
    return float("nan") if np.isnan(v).any() else float(v.max())


# name -> sets besides the bounds: (set type, operator, mode)
SOLVE_SETS = {
    "l1-fiber-z-Dz": [("l1", "D_z", ("fiber", "z"))],
    "l1-slice-z-DxDy": [("l1", "D_x", ("slice", "z")), ("l1", "D_y", ("slice", "z"))],
    "l2-fiber-x": [("l2", "identity", ("fiber", "x"))],
    "annulus-slice-y": [("annulus", "identity", ("slice", "y"))],
}
# a 2-D grid has no slices (refused) and no D_y
SOLVE_CASES = [(name, (16, 12, 8), (25.0, 25.0, 25.0)) for name in SOLVE_SETS] + \
              [(name, (32, 24), (25.0, 6.0)) for name in ("l1-fiber-z-Dz", "l2-fiber-x")]


def _solve_problem(mod, name, n, h, TF, m, opt_kw):
    """The list {bounds, the sets of SOLVE_SETS[name]} for module `mod`; radii: half the mean per-segment norm of A m.  The oracle is
    set up with the whole-array form of each set and its projector then replaced by the per-segment reference."""
    g = mod.compgrid(h, n)
    opt = mod.PARSDMM_options(FL=TF, **opt_kw)
    c = [mod.set_definitions("bounds", "identity", 1600.0, 3900.0, ("matrix", ""))]
    swaps = []
    for st, opn, mode in SOLVE_SETS[name]:
        A, _, _, tdn, _ = O.get_TD_operator(O.compgrid(h, n), opn, TF)
        tdn = tuple(int(q) for q in tdn)
        s = np.asarray(A @ m, np.float64)
        segs = seg_norms_ref.segment_indices(tdn, mode)
        if st == "l1":
            r = TF(0.5 * np.mean([np.abs(s[ind]).sum() for ind in segs]))
            mn, mx, fun = 0.0, float(r), (lambda x, r=r: O.project_l1_Duchi(x, r))
        else:
            r = TF(0.5 * np.mean([np.linalg.norm(s[ind]) for ind in segs]))
            if st == "l2":
                mn, mx, fun = 0.0, float(r), (lambda x, r=r: O.project_l2(x, r))
            else:
                r0 = TF(0.9 * float(r))
                mn, mx, fun = float(r0), float(r), (lambda x, r0=r0, r=r: O.project_annulus(x, r0, r))
        c.append(mod.set_definitions(st, opn, mn, mx, ("matrix", "") if mod is O else mode))
        swaps.append((len(c) - 1, lambda x, tdn=tdn, mode=mode, fun=fun: seg_norms_ref.project_segments(x, tdn, mode, fun)))
    if mod is O:
        P, A, prop = mod.setup_constraints(c, g, TF)
        for i, f in swaps:
            P[i] = f
    else:
        P, A, prop = mod.setup_constraints(c, g, TF, segment_norms=True)
    A, AtA, l, y = mod.PARSDMM_precompute_distribute(A, prop, g, opt)
    return g, opt, P, A, prop, AtA


@pytest.mark.parametrize("TF", [np.float32, np.float64])
@pytest.mark.parametrize("name,n,h", SOLVE_CASES)
def test_segmented_sets_solve_matches_oracle(sipx, TF, name, n, h):
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
