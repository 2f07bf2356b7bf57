"""The l2,0 sets on TV / TV_xy on the GPU (csrc/l20.h, csrc/ext_group.hip: L20Proj, L20FrameProj) through sipx.Projector,
sipx.tv_group_norms and whole solves: the selection held to tests/card_exact.check_card_output on the device's own key, the key held bit
for bit to (T)sqrt of the float64 sum of squares in block order (the joint key to the bound of tests/test_gpu_l21_joint.py), tie groups
across the k-th place on both selection routes and across the cut of a streamed frame, inputs that must not be written, repeatability,
reset and set_data, whole solves against the oracle with its projector swapped for tests/l20_ref.project, the device-resident solve and
the refusals through the C ABI.

v is handed to sipx.Projector as the M-vector of the range, so any v is allowed, not only gradients; the key of such a v is the
reference's, which section 2 holds the device's to.  CASES: tests/l20_cases.py; tests/test_l20_cpu.py shows from the plans that they
reach both widths of the apply kernel, both selection routes, both paths of the frame plan in each precision and a joint chunk plan
with two or more ragged chunks.

The solve models are piecewise constant with exactly k edge groups plus small noise: with fewer than k edges the k-th and the (k+1)-th
key are both noise and no gap can be held between them, so a selection flip between the engine and the oracle -- another problem, not
a rounding error -- could not be told from a fault.

Measured on an MI355X: 140 tests in 4.1 s; the joint key is at most 0.47 (Float32) and 0.99 (Float64) eps from the unrounded norm and has
the bits of the chunked reference; the smallest gap between the k-th and the (k+1)-th key over the oracle's projections is 0.563 (2-D),
0.587 (per frame), 0.740 (joint); x agrees with the oracle to 0 (Float32) and 3e-15 (Float64)."""
import ctypes as C

import numpy as np
import pytest
import torch      # (before libsipx.so is loaded: one HIP runtime in the process)

from oracle import parsdmm_oracle as O
from tests import card_exact, l1_exact, l21_joint_ref
from tests import l20_cases as CS
from tests import l20_ref as R
from tests.test_gpu_l21_frames import LOG_FIELDS, _in_place, _julia_max, _stacked
from tests.test_gpu_l21_joint import bound as joint_bound
from tests.test_gpu_set_data import _assert_same

pytestmark = pytest.mark.gpu

PRECISIONS = [np.float32, np.float64]
SMALL, SEARCH = 1, 2
MIN_GAP = 1e-3


def _grid(sipx, n):
    return sipx.compgrid(tuple(1.0 for _ in n), n)      # unit spacing: A x on the host has the bits of A x on the device


def _mode(n, form):
    return ("slice", "z") if form == "frames" else (("matrix", "") if len(n) == 2 else ("tensor", ""))


def _P(sipx, op, n, form, TF, k):
    return sipx.Projector(sipx.set_definitions("l20_joint" if form == "joint" else "l20", op, 0, k, _mode(n, form)), _grid(sipx, n), TF)


class _route:
    """Projectors built inside the block take the forced selection route."""
    def __init__(self, sipx, route):
        self.sipx, self.route = sipx, route

    def __enter__(self):
        assert self.sipx.lib().sipx_card_groups_route(self.route) == 0

    def __exit__(self, *a):
        assert self.sipx.lib().sipx_card_groups_route(0) == 0


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _xv(sipx, op, n, TF):
    """(x, v = A x): a blocky x with heavy-tailed noise on two thirds of the grid and flat ground elsewhere, so that some groups are zero."""
    key = ("xv", op, tuple(n), np.dtype(TF).name)
    if key not in CS._cache:
        rng = np.random.default_rng(77 + sum(n))
        N = int(np.prod(n))
        x = 3.0 * rng.integers(0, 4, N) + rng.standard_normal(N) * np.exp(rng.standard_normal(N))
        x[rng.random(N) < 0.35] = 2.0
        x = x.astype(TF)
        v = np.asarray(sipx.TDOperator(op, _grid(sipx, n), TF) @ x, TF)
        x.setflags(write=False)
        v.setflags(write=False)
        CS._cache[key] = (x, v)
    return CS._cache[key]


def _pools(g, n, form, k):
    """[(slice of the points / pixels that compete, their keys, their budget)]"""
    if form != "frames":
        return [(slice(0, len(g)), g, int(k))]
    L = int(n[0]) * int(n[1])
    ks = np.broadcast_to(np.asarray(k), (int(n[2]),))
    return [(slice(f * L, (f + 1) * L), g[f * L:(f + 1) * L], int(ks[f])) for f in range(int(n[2]))]


def _check_selection(v, y, g, k, op, n, form, what):
    """Kept groups are v bit for bit, dropped ones all +0, and the kept set is the stable selection on g.  With at most k non-zero keys
    nothing may be written; otherwise tau > 0, so a group of norm 0 is dropped and written like any other.  The rows of y outside every
    group do not exist: the pads of the device layout show only through the rows coming back right."""
    TF = v.dtype.type
    G = R.members(n, op)
    has = G >= 0
    Gs = np.where(has, G, 0)
    same = ((_bits(v)[Gs] == _bits(y)[Gs]) | ~has).all(axis=1)
    zero = ((_bits(y)[Gs] == 0) | ~has).all(axis=1)
    if form == "joint":
        n3 = int(n[2])
        same, zero = same.reshape(n3, -1).all(axis=0), zero.reshape(n3, -1).all(axis=0)
    kept_total = 0
    for sl, gp, kp in _pools(g, n, form, k):
        need = kp < len(gp) and int(np.count_nonzero(gp)) > kp
        s, z = same[sl], zero[sl]
        if not need:
            assert s.all(), f"{what}: a group was written although nothing is to be dropped"
            continue
        pos = gp > 0
        assert (s | z)[pos].all(), f"{what}: a group is neither kept bit for bit nor all +0"
        assert z[~pos].all(), f"{what}: a zero group was not written +0"
        keep = s & pos
        card_exact.check_card_output(gp, np.where(keep, gp, TF(0)).astype(TF), kp)
        assert np.array_equal(keep, R.kept(gp, kp)), what
        assert int(keep.sum()) == kp
        kept_total += kp
    return kept_total


# ---- 1. the selection is exact on the device's own key -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("op,n,form", CS.CASES)
def test_selection_is_exact_on_the_device_key(sipx, TF, op, n, form):
    x, v = _xv(sipx, op, n, TF)
    g = sipx.tv_group_norms(x, _grid(sipx, n), op, joint=form == "joint")
    ng = R.ngroups(n, op, form)
    assert g.dtype == TF and g.shape == (ng if form == "joint" else int(np.prod(n)),)
    assert 0 < int(np.count_nonzero(g == 0)) < len(g), "the input has no zero group"
    for k in CS.ks(ng):
        y = _P(sipx, op, n, form, TF, k)(v.copy())
        _check_selection(v, y, g, k, op, n, form, f"{op} {n} {form} k {k}")
    if form == "joint":                                   # the small route by the size of these cases: the search route too
        with _route(sipx, SEARCH):
            y = _P(sipx, op, n, form, TF, ng // 3)(v.copy())
        _check_selection(v, y, g, ng // 3, op, n, form, f"{op} {n} joint, search route")


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("op,n,form", [c for c in CS.CASES if int(np.prod(c[1])) <= 3000])
def test_selection_on_vectors_that_are_no_gradients(sipx, TF, op, n, form):
    v = CS.mixed_input(op, n, form, TF)
    g = R.norms(v, n, op, form, TF)                       # (the device's key, by section 2)
    ng = R.ngroups(n, op, form)
    for k in CS.ks(ng):
        y = _P(sipx, op, n, form, TF, k)(v.copy())
        _check_selection(v, y, g, k, op, n, form, f"{op} {n} {form} k {k}")
        assert l1_exact.same_bits(y, R.project(v, n, op, form, k))


def test_frames_with_a_vector_of_budgets_and_a_single_frame(sipx):
    """One entry >= L: that frame must stay unwritten, -0.0 included; n3 = 1 is a 2-D grid to the front end, which has no TV_xy: the
    per-frame set of one frame is ("l20", "TV") on the plane."""
    for TF in PRECISIONS:
        for n in [(8, 6, 3), (72, 64, 3)]:
            L = n[0] * n[1]
            v = CS.mixed_input("TV_xy", n, "frames", TF)
            g = R.norms(v, n, "TV_xy", "frames", TF)
            k = np.array([3, L, L // 2])
            y = _P(sipx, "TV_xy", n, "frames", TF, k)(v.copy())
            _check_selection(v, y, g, k, "TV_xy", n, "frames", f"frames {n} k-vector")
            assert l1_exact.same_bits(y, R.project(v, n, "TV_xy", "frames", k))
            G = R.members(n, "TV_xy")[L:2 * L]
            rows = G[G >= 0]
            assert np.signbit(v[rows]).any() and l1_exact.same_bits(y[rows], v[rows]), "the frame with k >= L was written"
    with pytest.raises(sipx.SipxError) as e:
        _P(sipx, "TV_xy", (8, 6, 1), "frames", np.float32, 3)
    assert str(e.value) == sipx.host.TV_XY_NEEDS_3D


# ---- 2. the key is right -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("op,n,form", [c for c in CS.CASES if c[2] != "joint"])
def test_key_is_the_float64_sum_of_squares_rounded_once(sipx, TF, op, n, form):
    x, v = _xv(sipx, op, n, TF)
    g = sipx.tv_group_norms(x, _grid(sipx, n), op)
    assert l1_exact.same_bits(g, R.norms(v, n, op, "whole", TF)), "the key is not (T)sqrt of the float64 sum of squares in block order"
    gt = sipx.tv_group_norms(torch.from_numpy(x.copy()).cuda(), _grid(sipx, n), op)
    assert gt.is_cuda and l1_exact.same_bits(gt.cpu().numpy(), g)
    ref = sipx.l21_norm(x, _grid(sipx, n), op)
    s = float(np.sum(g.astype(l1_exact._WIDE)))
    assert abs(float(ref) - s) <= 2 * float(np.finfo(TF).eps) * s, "sum(tv_group_norms) and l21_norm disagree"


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("op,n,form", CS.JOINT)
def test_joint_key_is_within_the_bound_of_the_joint_ball(sipx, TF, op, n, form):
    x, v = _xv(sipx, op, n, TF)
    g = sipx.tv_group_norms(x, _grid(sipx, n), "TV_xy", joint=True)
    exact = l21_joint_ref.exact_norms(v, n)
    eps = float(np.finfo(TF).eps)
    worst = float(np.max(np.abs(g.astype(np.float64) - exact) / np.maximum(exact, np.finfo(np.float64).tiny)) / eps)
    print(f"l20 joint key {n} {np.dtype(TF).name}: worst |g - exact| = {worst:.3f} eps g (bound {joint_bound(n, TF)}); "
          f"bits of the chunked reference: {l1_exact.same_bits(g, l21_joint_ref.norms(v, n, TF))}")
    assert np.all(np.abs(g.astype(np.float64) - exact) <= joint_bound(n, TF) * eps * exact)
    assert np.array_equal(g == 0, exact == 0)
    ref = sipx.l21_joint_norm(x, _grid(sipx, n))
    s = float(np.sum(g.astype(l1_exact._WIDE)))
    assert abs(float(ref) - s) <= 2 * eps * s


# ---- 3. ties ---------------------------------------------------------------------------------------------------------------------------------------
def _tie_vector(n, op, TF, strong=(), weak=()):
    """Exact integers whose different members give equal norm bits: every group has norm 5 -- (3, 4), (5, 0), (0, 5), (4, 3) in turn, a
    group of one member 5, of three (0, 3, 4) -- but the groups `strong` (norm 10: (6, 8)) and `weak` (norm 3)."""
    G = R.members(n, op)
    v = np.zeros(R.rows(n, op), TF)
    pats = [(3, 4), (5, 0), (0, 5), (4, 3)]
    for p in range(G.shape[0]):
        idx = G[p][G[p] >= 0]
        if len(idx) == 0:
            continue
        a = pats[p % 4]
        vals = {1: (5,), 2: a, 3: (0,) + a}[len(idx)]
        if p in strong:
            vals = {1: (10,), 2: (6, 8), 3: (0, 6, 8)}[len(idx)]
        if p in weak:
            vals = {1: (3,), 2: (0, 3), 3: (3, 0, 0)}[len(idx)]
        v[idx] = np.array(vals, TF) * (-1 if p % 3 == 0 else 1)
    return v


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("n,routes", [((8, 6), (SMALL, SEARCH)), ((32, 32), (SMALL, SEARCH)), ((41, 25), (0, SEARCH)), ((8, 4, 6), (SMALL, SEARCH))])
def test_a_tie_group_across_the_kth_place_on_both_routes(sipx, TF, n, routes):
    N = int(np.prod(n))
    v = _tie_vector(n, "TV", TF, strong=(4, 9, 17), weak=(2, 11, 30))
    g = R.norms(v, n, "TV", "whole", TF)
    assert set(np.unique(g)) == {0.0, 3.0, 5.0, 10.0}
    outs = []
    for k in (3, 4, N // 2, N - 5):
        assert k <= 3 or card_exact.straddles(g, k)[0]
        for route in routes:
            with _route(sipx, route):
                y = _P(sipx, "TV", n, "whole", TF, k)(v.copy())
            _check_selection(v, y, g, k, "TV", n, "whole", f"ties {n} k {k} route {route}")
            outs.append(y)
        assert l1_exact.same_bits(outs[-1], outs[-2]), "the routes differ"


@pytest.mark.parametrize("TF", PRECISIONS)
def test_a_tie_group_above_the_gather_capacity_keeps_the_lowest_indices(sipx, TF):
    op, n, form = CS.BIG_TIE
    v = _tie_vector(n, op, TF)
    g = R.norms(v, n, op, form, TF)
    assert int((g == 5).sum()) == 96 * 96 - 1 > CS.CARD_CAP
    y = _P(sipx, op, n, form, TF, 100)(v.copy())
    _check_selection(v, y, g, 100, op, n, form, "big tie")
    G = R.members(n, op)
    kept = [p for p in range(len(g)) if np.any(y[G[p][G[p] >= 0]] != 0)]
    assert kept == list(range(100)), "the lowest indices must stay"


@pytest.mark.parametrize("TF", PRECISIONS)
def test_a_tie_group_across_the_cut_of_a_streamed_frame(sipx, TF):
    n = (96, 96, 3)                                       # 9216 keys a frame: streamed in both precisions
    L = 96 * 96
    v = _tie_vector(n, "TV_xy", TF, strong=(5, L + 7, 2 * L + 1), weak=(8, L + 3))
    g = R.norms(v, n, "TV_xy", "frames", TF)
    for k in (np.array([100, 5000, L]), 2, L - 2):
        y = _P(sipx, "TV_xy", n, "frames", TF, k)(v.copy())
        _check_selection(v, y, g, k, "TV_xy", n, "frames", f"streamed ties k {k}")
        assert l1_exact.same_bits(y, R.project(v, n, "TV_xy", "frames", k))


# ---- 4. nothing to do means nothing written ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("op,n,form", [("TV", (8, 6), "whole"), ("TV", (30, 12, 8), "whole"), ("TV_xy", (8, 4, 67), "joint"),
                                        ("TV_xy", (8, 6, 3), "frames"), ("TV_xy", (96, 96, 3), "frames")])
def test_nothing_to_drop_means_nothing_written(sipx, TF, op, n, form):
    ng = R.ngroups(n, op, form)
    G = R.members(n, op)
    rng = np.random.default_rng(3)
    v = np.zeros(R.rows(n, op), TF)
    v[:] = TF(-0.0)
    few = rng.choice(ng, 4, replace=False)                # four non-zero groups (per frame: in every frame; joint: pixels)
    pts = few if form == "whole" else np.concatenate([few + f * ng for f in range(n[2])])
    for p in pts:
        idx = G[p][G[p] >= 0]
        v[idx] = TF(1 + p % 7)
    nz = int(np.count_nonzero(R.norms(v, n, op, form, TF)[:ng] if form == "frames" else R.norms(v, n, op, form, TF)))
    assert 1 <= nz <= 4
    for k in (nz, ng - 1, ng, ng + 3, 2 ** 24 + 1):
        y = _P(sipx, op, n, form, TF, k)(v.copy())
        assert l1_exact.same_bits(y, v), f"k = {k}: v was written"
    if nz > 1:
        y = _P(sipx, op, n, form, TF, nz - 1)(v.copy())
        assert not l1_exact.same_bits(y, v) and not np.signbit(y[y == 0]).all()


def test_k_at_least_the_number_of_groups_launches_nothing(sipx):
    TF, n, h = np.float32, (16, 12, 4), (1.0, 1.0, 1.0)
    m = np.random.default_rng(1).standard_normal(int(np.prod(n))).astype(TF)
    names = {"k_l21_norms", "k_l21j_norms", "k_l21j_finish", "k_cardg_rank", "k_card_*", "k_l20_frames", "k_l20_zero"}
    for big in (True, False):
        g = sipx.compgrid(h, n)
        k = (lambda ng: ng if big else ng // 4)
        c = [sipx.set_definitions("bounds", "identity", -1.0, 1.0, ("tensor", "")), sipx.set_definitions("l20", "TV", 0, k(16 * 12 * 4), ("tensor", "")),
             sipx.set_definitions("l20", "TV_xy", 0, k(16 * 12), ("slice", "z")), sipx.set_definitions("l20_joint", "TV_xy", 0, k(16 * 12), ("tensor", ""))]
        opt = sipx.PARSDMM_options(FL=TF, maxit=8, evol_rel_tol=0.0, feas_tol=0.0, obj_tol=0.0)
        P, A, prop = sipx.setup_constraints(c, g, TF)
        A, AtA, _, _ = sipx.PARSDMM_precompute_distribute(A, prop, g, opt)
        ctx = sipx.host.build_context(m, AtA, A, prop, P, g, opt)
        try:
            ctx.parsdmm_begin(opt)
            ctx.kernel_stats_all(2)
            ctx.parsdmm_steps(4)
            st = ctx.kernel_stats_all(0)
            ran = {q["name"] for q in st["kernels"] if q["launches"] > 0} & names
            row = st["l20"]
            assert row["calls"] > 0 and row["groups"] in (16 * 12, 16 * 12 * 4)
            if big:
                assert not ran, f"k >= the number of groups, and {sorted(ran)} ran"
                assert row["small"] == row["search"] == row["frames"] == 0
            else:
                assert {"k_l21_norms", "k_l21j_norms", "k_cardg_rank", "k_l20_frames", "k_l20_zero"} <= ran
                assert row["small"] > 0 and row["frames"] > 0 and row["small"] + row["search"] + row["frames"] == row["calls"]
        finally:
            ctx.close()


# ---- 5. stability and equivalence ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("op,n,form", [("TV", (8, 6), "whole"), ("TV", (30, 12, 8), "whole"), ("TV_xy", (8, 4, 67), "joint"),
                                        ("TV_xy", (72, 64, 3), "frames")])
def test_projection_is_idempotent_and_repeatable(sipx, TF, op, n, form):
    v = CS.mixed_input(op, n, form, TF) if int(np.prod(n)) <= 3000 else _xv(sipx, op, n, TF)[1]
    k = R.ngroups(n, op, form) // 3
    P = _P(sipx, op, n, form, TF, k)
    y = P(v.copy())
    assert not l1_exact.same_bits(y, v)
    assert l1_exact.same_bits(P(v.copy()), y), "two calls differ"
    assert l1_exact.same_bits(P(y.copy()), y), "P(P(v)) != P(v)"
    if form != "frames":
        outs = []
        for route in ((SMALL, SEARCH) if R.ngroups(n, op, form) <= CS.SMALL_MAX else (0, SEARCH)):
            with _route(sipx, route):
                outs.append(_P(sipx, op, n, form, TF, k)(v.copy()))
        assert l1_exact.same_bits(outs[0], outs[1]) and l1_exact.same_bits(outs[0], y), "the routes differ"


SOLVE_CASES = [("l20-tv-2d", (32, 24), (25.0, 25.0)), ("l20-frames", (16, 12, 4), (25.0, 25.0, 6.0)), ("l20-joint", (16, 12, 4), (25.0, 25.0, 6.0))]


def _solve_model(name, n, TF, seed):
    """(m, k): a piecewise-constant model inside the bounds but for one block, small noise, and k = its number of edge groups."""
    rng = np.random.default_rng(20261021 + seed)
    m = np.full(n, 2000.0)
    if len(n) == 2:
        m[8:20, 6:15] = 3000.0
        m[22:, :] = 4300.0                                # (above the upper bound)
    elif name == "l20-joint":
        for f in range(n[2]):                             # one common edge set, its contrast differs from frame to frame
            m[4:11, 3:9, f] = 2600.0 + 250.0 * f
        m[13:, :, :] = 4300.0
    else:
        for f in range(n[2]):                             # the block moves from frame to frame
            m[3 + f:9 + f, 2 + f:8 + f, f] = 3100.0
        m[13:, :, :] = 4300.0
    flat = m.copy()
    m += 0.5 * rng.standard_normal(n)
    op = "TV" if len(n) == 2 else "TV_xy"
    form = {"l20-tv-2d": "whole", "l20-frames": "frames", "l20-joint": "joint"}[name]
    h = dict((c[0], c[2]) for c in SOLVE_CASES)[name]
    A = O.get_TD_operator(O.compgrid(h, n), "TV", np.float64)[0] if len(n) == 2 else _stacked(n, h, np.float64)
    g = R.norms(np.asarray(A @ flat.reshape(-1, order="F")), n, op, form, np.float64)
    if form == "frames":
        L = n[0] * n[1]
        k = np.array([int(np.count_nonzero(g[f * L:(f + 1) * L])) for f in range(n[2])])
    else:
        k = int(np.count_nonzero(g))
    return m.astype(TF).reshape(-1, order="F"), k, op, form


def _solve_problem(mod, name, n, h, TF, m, k, op, form, opt_kw, gaps=None):
    """{bounds, the l2,0 set of `name`} for module `mod`.  The oracle is set up with a cardinality set on the operator (TV_xy: its own D_y
    and D_x stacked, as a custom operator), so that ncvx agrees, its projector then replaced by the reference, which also records the gap
    between the k-th and the (k+1)-th key of every call."""
    g = mod.compgrid(h, n)
    opt = mod.PARSDMM_options(FL=TF, **opt_kw)
    whole = ("matrix", "") if len(n) == 2 else ("tensor", "")
    c = [mod.set_definitions("bounds", "identity", 1600.0, 3900.0, whole)]
    if mod is O:
        def proj(x):
            if gaps is not None:
                key = R.norms(x, n, op, form, TF)
                gaps.extend(R.gap(gp, kp) for _, gp, kp in _pools(key, n, form, k))
            return _in_place(lambda a: R.project(a, n, op, form, k), x)
        kk = int(np.max(k))
        if op == "TV":
            c.append(mod.set_definitions("cardinality", "TV", 0, kk, whole))
        else:
            c.append(mod.set_definitions("cardinality", "identity", 0, kk, whole, (_stacked(n, h, TF), False)))
    else:
        c.append(mod.set_definitions("l20_joint" if form == "joint" else "l20", op, 0, k, _mode(n, form)))
    P, A, prop = mod.setup_constraints(c, g, TF)
    if mod is O:
        P[1] = proj
    A, AtA, l, y = mod.PARSDMM_precompute_distribute(A, prop, g, opt)
    return g, opt, P, A, prop, AtA


def _fresh(sipx, args, m):
    AtA, A, prop, P, g, opt = args
    ctx = sipx.host.build_context(m, AtA, A, prop, P, g, opt)
    try:
        log, _ = ctx.parsdmm(opt)
        x, l, y = ctx.download()
    finally:
        ctx.close()
    return x, l, y, log


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("case", [0, 1])
def test_two_solves_and_a_reset_give_the_bits_of_a_new_context(sipx, TF, case):
    name, n, h = SOLVE_CASES[case]
    m, k, op, form = _solve_model(name, n, TF, 5)
    g, opt, Ps, A, prop, AtA = _solve_problem(sipx, name, n, h, TF, m, k, op, form, dict(maxit=12))
    args = (AtA, A, prop, Ps, g, opt)
    want = _fresh(sipx, args, m)
    with sipx.Solver(*args, TF) as S:
        for _ in range(2):                                # the second solve is a reset of the same context
            x, log, l, y = S(m.copy())
            _assert_same((x, l, y, log), want)
        assert log.context_reused
        st = S.ctx.kernel_stats_all(-1)["l20"]
        assert st["calls"] >= 2 and st["small" if form == "whole" else "frames"] == st["calls"]
        if form == "whole":
            with pytest.raises(sipx.SipxError) as e:
                S.set_data(1, ub=np.ones(4, TF))
            assert str(e.value) == "set_data: " + sipx.host.L20_NO_SET_DATA
    if form != "frames":
        return
    # set_data with a new vector of budgets equals a new context built with it
    k2 = np.maximum(k // 2, 1)
    with sipx.Solver(*args, TF) as S:
        S(m.copy())
        S.set_data(1, ub=k2.astype(TF))
        x, log, l, y = S(m.copy())
        for bad, text in [(np.array([1, 0.5, 2, 2], TF), sipx.host.L20_BAD_K), (np.array([1, 0, 2, 2], TF), sipx.host.L20_BAD_K)]:
            with pytest.raises(sipx.SipxError) as e:
                S.set_data(1, ub=bad)
            assert str(e.value) == text
        with pytest.raises(sipx.SipxError) as e:
            S.set_data(1, lb=k2.astype(TF))
        assert str(e.value) == "set_data: " + sipx.host.L20_SET_DATA_UB
    g2, opt2, P2, A2, prop2, AtA2 = _solve_problem(sipx, name, n, h, TF, m, k2, op, form, dict(maxit=12))
    _assert_same((x, l, y, log), _fresh(sipx, (AtA2, A2, prop2, P2, g2, opt2), m))
    assert not np.array_equal(x, want[0]), "the new budgets changed nothing: the comparison shows nothing"


# ---- 6. whole solves against the oracle (rules and tolerances of tests/test_gpu_card_groups.py, test_solve_matches_oracle) -----------------------
@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("name,n,h", SOLVE_CASES)
def test_solve_matches_oracle(sipx, TF, name, n, h):
    """Smallest gap between the k-th and the (k+1)-th key over the oracle's projections, measured on the CPU: see DESIGN.md 7m."""
    m, k, op, form = _solve_model(name, n, TF, seed=1)
    kw = dict(maxit=60)
    gaps = []
    go, oo, Po, Ao, propo, AtAo = _solve_problem(O, name, n, h, TF, m, k, op, form, kw, gaps)
    gs, os_, Ps, As, props, AtAs = _solve_problem(sipx, name, n, h, TF, m, k, op, form, kw)
    assert props.ncvx == propo.ncvx and props.ncvx[1]
    xo, lo, l_o, y_o = O.PARSDMM(m.copy(), AtAo, Ao, propo, Po, go, oo)
    # the condition of the comparison, checked on the oracle alone: no projection of its run was within MIN_GAP of another selection
    assert gaps and min(gaps) >= MIN_GAP, f"{name}: the k-th and the (k+1)-th key came within {min(gaps):.2e} of each other in the oracle's run"
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
    sep = next((q for q in range(Kc) if ls.cg_it[q] != lo.cg_it[q] or not np.allclose(ls.rho[q], lo.rho[q], rtol=sep_rt)), None)
    upto = Kc if sep is None else sep
    for f in ("obj", "r_pri_total", "rho", "gamma"):
        a, b = np.asarray(getattr(ls, f))[:upto], np.asarray(getattr(lo, f))[:upto]
        assert np.allclose(a, b, rtol=(5e-4 if TF == np.float32 else 1e-6), atol=1e-12), (f, upto)
    tol = 5e-4 if TF == np.float32 else 1e-6
    print(f"{name} {n} {np.dtype(TF).name}: iterations {len(ls.obj)} / {len(lo.obj)}, separation {sep}, rel diff {err:.3e}, "
          f"smallest gap {min(gaps):.3e} over {len(gaps)} projections")
    if sep is not None or len(ls.obj) != len(lo.obj):
        # after a separation: the oracle again with the engine's rho / gamma history forced on it
        gr, orr, Pr, Ar, propr, AtAr = _solve_problem(O, name, n, h, TF, m, k, op, form, dict(kw, maxit=len(ls.obj)))
        xr, lr, _, _ = O.PARSDMM(m.copy(), AtAr, Ar, propr, Pr, gr, orr, replay=(ls.rho, ls.gamma))
        err_replay = np.linalg.norm(xs.astype(np.float64) - xr) / np.linalg.norm(xr)
        assert err_replay < tol, (name, "replayed", sep, err_replay)
        tol = max(tol, 5e-4)
        assert _julia_max(ls.set_feasibility[-1]) <= max(_julia_max(lo.set_feasibility[-1]), float(os_.feas_tol))
    assert err < tol, (name, sep, err)
    assert ls.r_pri.shape == (len(ls.obj), 3) and ls.set_feasibility.shape[1] == 2
    assert len(y_s) == 3 and [len(q) for q in y_s] == [len(q) for q in y_o]
    assert len(ls.obj) > 6, "the solve stopped before anything was compared"


# ---- 7. the device-resident solve, the refusals through the C ABI -----------------------------------------------------------------------------------
def test_device_form_gives_the_bits_of_the_host_form(sipx):
    TF, (name, n, h) = np.float32, SOLVE_CASES[2]
    m, k, op, form = _solve_model(name, n, TF, seed=3)
    g, opt, P, A, prop, AtA = _solve_problem(sipx, name, n, h, TF, m, k, op, form, dict(maxit=30))
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


def _desc(sipx, op, proj=21, mode=0, dir=0, k=3.0, lb=None, ub=None, count=0, transform=0, component=0):
    d = sipx.host._SetDesc()
    d.op, d.proj, d.pmin, d.pmax, d.mode, d.dir, d.transform, d.component = op, proj, 0.0, k, mode, dir, transform, component
    d.lb = None if lb is None else lb.ctypes.data_as(C.c_void_p)
    d.ub = None if ub is None else ub.ctypes.data_as(C.c_void_p)
    d.reserved, d.ncvx = count, 1
    return d


def _refused(sipx, ctx, d):
    rc = sipx.lib().sipx_add_set(ctx.h, C.byref(d), None, None, 0)
    assert rc < 0, "the engine took the set"
    return sipx.lib().sipx_last_error().decode()


def test_engine_refusals(sipx):
    TF, H = np.float32, sipx.host
    OPS = H.OPS
    n = (16, 12, 8)
    g = sipx.compgrid((1.0, 1.0, 1.0), n)
    w = np.ones(16 * 12 * 8, TF)
    kv = np.full(8, 3.0, TF)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    ctx = sipx.Context(g, TF)
    try:
        for op in ("identity", "D_x", "D_z"):
            assert _refused(sipx, ctx, _desc(sipx, OPS[op])) == H.L20_NEEDS_TV
        for op in ("TV", "identity"):
            assert _refused(sipx, ctx, _desc(sipx, OPS[op], proj=22)) == H.L20_JOINT_ROUTE
        assert _refused(sipx, ctx, _desc(sipx, OPS["TV_xy"], proj=22, mode=2, dir=2)) == H.L20_JOINT_ROUTE
        import scipy.sparse as sp
        A = sp.identity(16 * 12 * 8, format="csc", dtype=TF)      # a custom operator: valid CSC arrays, so that the set's own refusal is reached
        cp, ri, nz = np.ascontiguousarray(A.indptr, np.int64), np.ascontiguousarray(A.indices, np.int64), np.ascontiguousarray(A.data, TF)
        d = _desc(sipx, OPS["custom"])
        d.csc_colptr, d.csc_rowval, d.csc_nzval, d.csc_rows = cp.ctypes.data, ri.ctypes.data, nz.ctypes.data, 16 * 12 * 8
        assert _refused(sipx, ctx, d) == H.L20_NEEDS_TV
        for tr in (1, 2):
            assert _refused(sipx, ctx, _desc(sipx, OPS["TV"], transform=tr)) == H.L20_NO_TRANSFORM
            assert _refused(sipx, ctx, _desc(sipx, OPS["TV_xy"], proj=22, transform=tr)) == H.L20_NO_TRANSFORM
        assert _refused(sipx, ctx, _desc(sipx, OPS["TV"], component=1)) == H.L20_NO_MINKOWSKI
        for mode, dir in ((1, 2), (1, 0), (2, 0), (2, 1)):
            assert _refused(sipx, ctx, _desc(sipx, OPS["TV_xy"], mode=mode, dir=dir)) == H.L20_MODES
        assert _refused(sipx, ctx, _desc(sipx, OPS["TV"], mode=2, dir=2)) == H.L20_MODES
        assert _refused(sipx, ctx, _desc(sipx, OPS["TV"], lb=w, count=len(w))) == H.L20_NO_WEIGHTS
        assert _refused(sipx, ctx, _desc(sipx, OPS["TV_xy"], mode=2, dir=2, lb=kv)) == H.L20_NO_WEIGHTS
        assert _refused(sipx, ctx, _desc(sipx, OPS["TV"], ub=kv)) == H.L20_K_VECTOR
        assert _refused(sipx, ctx, _desc(sipx, OPS["TV_xy"], proj=22, ub=kv)) == H.L20_K_VECTOR
        for k in (0.0, -1.0, 2.5, float("nan"), float("inf")):
            assert _refused(sipx, ctx, _desc(sipx, OPS["TV"], k=k)) == H.L20_BAD_K
            assert _refused(sipx, ctx, _desc(sipx, OPS["TV_xy"], proj=22, k=k)) == H.L20_BAD_K
            assert _refused(sipx, ctx, _desc(sipx, OPS["TV_xy"], mode=2, dir=2, k=k)) == H.L20_BAD_K
        assert _refused(sipx, ctx, _desc(sipx, OPS["TV_xy"], mode=2, dir=2, ub=np.array([3, 3, 0.5, 3, 3, 3, 3, 3], TF))) == H.L20_BAD_K
        # what the engine takes -- pmin is ignored -- and what such sets refuse afterwards
        d = _desc(sipx, OPS["TV"], k=5.0)
        d.pmin = -7.0
        assert sipx.lib().sipx_add_set(ctx.h, C.byref(d), None, None, 0) == 0
        assert sipx.lib().sipx_add_set(ctx.h, C.byref(_desc(sipx, OPS["TV_xy"], mode=2, dir=2, k=1e9)), None, None, 0) == 1
        assert sipx.lib().sipx_add_set(ctx.h, C.byref(_desc(sipx, OPS["TV_xy"], mode=2, dir=2, ub=kv)), None, None, 0) == 2
        assert sipx.lib().sipx_add_set(ctx.h, C.byref(_desc(sipx, OPS["TV_xy"], proj=22, k=7.0)), None, None, 0) == 3
        for i in (0, 1, 3):
            assert sipx.lib().sipx_set_data(ctx.h, i, None, p(kv)) != 0
            assert sipx.lib().sipx_last_error().decode() == "sipx_set_data: " + H.L20_NO_SET_DATA
        assert sipx.lib().sipx_set_data(ctx.h, 2, p(kv), None) != 0
        assert sipx.lib().sipx_last_error().decode() == "sipx_set_data: " + H.L20_SET_DATA_UB
        assert sipx.lib().sipx_set_data(ctx.h, 2, None, p(np.array([3, 3, 0, 3, 3, 3, 3, 3], TF))) != 0
        assert sipx.lib().sipx_last_error().decode() == H.L20_BAD_K
        assert sipx.lib().sipx_set_data(ctx.h, 2, None, p(kv)) == 0
        # the stand-alone observer refuses what the set refuses
        out, x, cnt = np.zeros(16 * 12 * 8, TF), np.zeros(16 * 12 * 8, TF), C.c_int64()
        assert sipx.lib().sipx_tv_group_norms(ctx.h, OPS["D_z"], 0, p(x), p(out), C.byref(cnt)) != 0
        assert sipx.lib().sipx_last_error().decode() == H.L20_NEEDS_TV
        assert sipx.lib().sipx_tv_group_norms(ctx.h, OPS["TV"], 1, p(x), p(out), C.byref(cnt)) != 0
        assert sipx.lib().sipx_last_error().decode() == H.L20_JOINT_ROUTE
        assert sipx.lib().sipx_tv_group_norms(ctx.h, OPS["TV"], 0, None, None, C.byref(cnt)) == 0 and cnt.value == 16 * 12 * 8
        assert sipx.lib().sipx_tv_group_norms(ctx.h, OPS["TV_xy"], 1, None, None, C.byref(cnt)) == 0 and cnt.value == 16 * 12
    finally:
        ctx.close()
    # k below the number of groups that Float32 cannot hold: 2^26 points, 2^25 pixels
    big = sipx.compgrid((1.0, 1.0, 1.0), (8192, 4096, 2))
    for T_, want in ((np.float32, H.L20_K_INEXACT), (np.float64, None)):
        ctx = sipx.Context(big, T_)
        try:
            for d in (_desc(sipx, OPS["TV"], k=2.0 ** 24 + 1), _desc(sipx, OPS["TV_xy"], proj=22, k=2.0 ** 24 + 1)):
                if want:
                    assert _refused(sipx, ctx, d) == want
                else:
                    assert sipx.lib().sipx_add_set(ctx.h, C.byref(d), None, None, 0) >= 0
        finally:
            ctx.close()
    # a slab-decomposed or owned context
    ctx = sipx.Context(g, TF)
    try:
        ctx.set_decomp("slab")
        assert _refused(sipx, ctx, _desc(sipx, OPS["TV"])) == H.L20_SHARDED
    finally:
        ctx.close()
    for shard in (lambda c: c.set_decomp("slab"), lambda c: c.set_owned([1, 1])):
        ctx = sipx.Context(g, TF)
        try:
            ctx.add_set(sipx.TDOperator("TV", g, TF), _P(sipx, "TV", n, "whole", TF, 3), True)
            shard(ctx)
            with pytest.raises(sipx.SipxError) as e:
                ctx.finalize(np.ones(16 * 12 * 8, TF), [10.0], 1.0)
            assert H.L20_SHARDED in str(e.value)
        finally:
            ctx.close()
    # the projector itself: a vector of another length
    with pytest.raises(sipx.SipxError, match="the l2,0 set projects a vector of the TV range: 4192 entries on this grid, 7 given"):
        _P(sipx, "TV", n, "whole", TF, 3)(np.ones(7, TF))
