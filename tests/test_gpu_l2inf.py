"""The l2,inf ball on the GPU -- every group norm at most c_p (csrc/l2inf.h; csrc/ext_group.hip: k_l2inf_clip, k_l2infs_clip,
k_l2inf_scale and the observer's two-stage maximum behind L2InfProj): the projector alone through sipx.Projector / sipx_project against
tests/l2inf_ref.py, the bits it must leave, feasibility of the output to the header's bound, set_data, whole solves against the oracle
with its projector swapped for the reference (the way tests/test_gpu_l21.py runs its solves, with its iteration counts and tolerances:
the comparison is that of tests/test_gpu_l21_stacked.py, which copies it), the caller-supplied two-block operator that reproduces
("l2inf", "TV"), and the engine's refusals through the C ABI.

SIZES.  The clip kernels launch min(ceil(N / (256 VW)), 2048) workgroups of 256 threads, VW = 4 (Float32) or 2 (Float64) points per
thread when n1 % 4 == 0 (16 bytes per access) and one otherwise; one trip of the grid-stride loop covers 2048 * 256 thread-iterations.
(2048, 1025) is the smallest 2-D grid with n1 = 2048 whose N / 4 exceeds that, (2047, 1025) beside it takes the narrow path into its
fifth trip.  The stacked sizes are those of tests/test_gpu_l21_stacked.py.

A 3-D grid with n3 = 1 is a 2-D grid to the engine and the front end (host._grid): TV_xy does not exist there and the sets on it are
refused with the operator's own words (test_one_frame_is_a_2d_grid); the joint and TV_xy cases start at n3 = 2."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch      # (before libsipx.so is loaded: one HIP runtime in the process)

from oracle import parsdmm_oracle as O
from tests import l1_exact, l21_joint_ref
from tests import l2inf_ref as R
from tests import test_gpu_l21 as T21
from tests import test_gpu_l21_frames as TFR
from tests import test_gpu_l21_stacked as TS

pytestmark = pytest.mark.gpu

PRECISIONS = [np.float32, np.float64]
FRACS = [0.9, 0.5, 0.05]
TV_GRIDS = [(5, 4), (12, 9), (13, 7), (256, 5), (257, 4), (8, 6, 5), (7, 5, 3), (4, 3, 2)]
TVXY_GRIDS = [(8, 6, 2), (7, 5, 3)]
BIG_GRIDS = [(2048, 1025), (2047, 1025)]
JOINT_GRIDS = [(8, 6, 2), (8, 6, 5), (12, 9, 64), (4, 3, 16)]      # (4, 3, 16): l21_joint_plan cuts it into two chunks
BLOCKS = [1, 2, 3, 6, 8]
SMALL_G = [1, 3, 4, 255, 256, 257, 1028]
_cache = {}
_worst = {}


def _mode(n):
    return ("matrix", "") if len(n) == 2 else ("tensor", "")


def _grid(sipx, n):
    return sipx.compgrid(tuple(1.0 for _ in n), n)


class Case:
    """One layout: its groups (tests/l2inf_ref.py), an input, and the projector of a bound c."""

    def __init__(self, kind, n=None, B=None, G=None):
        self.kind, self.n, self.B, self.G = kind, n, B, G
        self.jn = n if kind == "joint" else None
        if kind == "tv":
            self.idx = R.layout_tv(n)
        elif kind == "tv_xy":
            self.idx = R.layout_tv_xy(n)
        elif kind == "joint":
            self.idx = R.layout_joint(n)
        else:
            self.idx = R.layout_stacked(B * G, B)
        self.groups, self.m = self.idx.shape

    def input(self, TF):
        """Heavy-tailed randn * exp(randn) as the make_input of the l2,1 tests builds it, with an all-zero group and a group of -0.0;
        computed once, handed out as a copy."""
        key = ("in", self.kind, self.n, self.B, self.G, np.dtype(TF).name)
        if key not in _cache:
            if self.kind == "tv":
                v = T21.make_input(self.n, TF)[0]
            elif self.kind == "stacked":
                v = TS.make_input(self.B, self.G, TF)[0]
            else:
                v = TFR.make_input(self.n, TF)[0]
            if self.kind != "stacked" and self.groups >= 6:
                for p, z in ((self.groups // 2, 0.0), (self.groups // 3, -0.0)):
                    mem = self.idx[p][self.idx[p] >= 0]
                    v[mem] = z
            v.setflags(write=False)
            _cache[key] = v
        return _cache[key].copy()

    def norms(self, v, TF):
        return R.norms(v, self.idx, TF, self.jn)

    def P(self, sipx, TF, c, small=True):
        if self.kind == "stacked":
            M = self.B * self.G
            if small:
                grid, A = sipx.compgrid((1.0, 1.0), (M, 1)), sp.identity(M, format="csc", dtype=TF)
            else:
                grid, A = sipx.compgrid((1.0, 1.0), (4, 3)), sp.csc_matrix((M, 12), dtype=TF)
            sd = sipx.set_definitions("l2inf_stacked", "custom", 0, c, ("matrix", ""), custom_TD_OP=(A, False), blocks=self.B)
            return sipx.Projector(sd, grid, TF)
        st, op = {"tv": ("l2inf", "TV"), "tv_xy": ("l2inf", "TV_xy"), "joint": ("l2inf_joint", "TV_xy")}[self.kind]
        return sipx.Projector(sipx.set_definitions(st, op, 0, c, _mode(self.n)), _grid(sipx, self.n), TF)


def _vector_bound(case, v, TF, seed):
    """c = u (.) g with u drawn from {0, 0.5, 1, 2, +inf}; where g = 0 the product with inf is taken as 0."""
    g = case.norms(v, TF)
    u = np.random.default_rng(seed).choice([0.0, 0.5, 1.0, 2.0, np.inf], case.groups)
    with np.errstate(invalid="ignore"):
        c = (u * g.astype(np.float64)).astype(TF)
    c[np.isnan(c)] = TF(0)
    return c


def _check(sipx, case, TF, c, label, small=True):
    """|y - ref| <= 4 eps |v| per entry, two calls give the same bits, unclipped groups keep their bits; returns the worst error in eps |v|."""
    v = case.input(TF)
    ref = R.project(v, case.idx, c, case.jn)
    P = case.P(sipx, TF, c, small)
    y = P(v.copy())
    eps = float(np.finfo(TF).eps)
    v64 = np.abs(v.astype(np.float64))
    err = np.abs(y.astype(np.float64) - np.asarray(ref, np.float64))
    worst = float(np.max(err / np.maximum(v64, np.finfo(np.float64).tiny)) / eps)
    key = (case.kind, np.dtype(TF).name)
    _worst[key] = max(_worst.get(key, 0.0), worst)
    print(f"l2inf {case.kind} n {case.n} B {case.B} G {case.G} {np.dtype(TF).name} {label}: worst error {worst:.3f} eps |v| "
          f"(worst so far for {key}: {_worst[key]:.3f})")
    assert np.all(err <= 4 * eps * v64), f"worst error {worst:.3f} eps |v|"
    assert l1_exact.same_bits(P(v.copy()), y), "two calls differ"
    keep = ~(case.norms(v, TF) > R.bounds(c, case.groups, TF))
    for q in range(case.m):
        has = (case.idx[:, q] >= 0) & keep
        assert l1_exact.same_bits(y[case.idx[has, q]], v[case.idx[has, q]]), "an unclipped group was changed"
    return worst


def _all_bounds(sipx, case, TF, small=True):
    v = case.input(TF)
    gmax = float(case.norms(v, TF).max())
    for frac in FRACS:
        _check(sipx, case, TF, TF(frac * gmax), f"scalar {frac}", small)
    _check(sipx, case, TF, _vector_bound(case, v, TF, 7 + case.groups), "vector", small)


# ---- the projector alone ------------------------------------------------------------------------------------------------------------------------
def test_the_large_grids_need_a_second_trip():
    a, b = BIG_GRIDS
    assert a[0] % 4 == 0 and a[0] * a[1] // 4 > 2048 * 256 and a[0] * (a[1] - 1) // 4 <= 2048 * 256
    assert b[0] % 4 != 0 and b[0] * b[1] > 2048 * 256
    assert l21_joint_ref.plan(12, 16, 4)[0] == 2 and l21_joint_ref.plan(12, 16, 8)[0] == 2, "(4, 3, 16) is chunked"
    assert l21_joint_ref.plan(108, 64, 4)[0] > 1


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("n", TV_GRIDS)
def test_tv_projector_matches_the_reference(sipx, TF, n):
    _all_bounds(sipx, Case("tv", n), TF)


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("n", TVXY_GRIDS)
def test_tv_xy_projector_matches_the_reference(sipx, TF, n):
    _all_bounds(sipx, Case("tv_xy", n), TF)


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("n", BIG_GRIDS)
def test_tv_projector_matches_the_reference_beyond_one_trip(sipx, TF, n):
    case = Case("tv", n)
    v = case.input(TF)
    _check(sipx, case, TF, TF(0.5 * float(case.norms(v, TF).max())), "scalar 0.5")
    _check(sipx, case, TF, _vector_bound(case, v, TF, 3), "vector")


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("G", SMALL_G)
@pytest.mark.parametrize("B", BLOCKS)
def test_stacked_projector_matches_the_reference(sipx, TF, B, G):
    _all_bounds(sipx, Case("stacked", B=B, G=G), TF)


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("odd", [0, 1])
@pytest.mark.parametrize("B", BLOCKS)
def test_stacked_projector_matches_the_reference_beyond_one_trip(sipx, TF, B, odd):
    case = Case("stacked", B=B, G=TS.g_trip(TF) + odd)
    v = case.input(TF)
    _check(sipx, case, TF, TF(0.5 * float(case.norms(v, TF).max())), "scalar 0.5", small=False)
    if B == 3:
        _check(sipx, case, TF, _vector_bound(case, v, TF, 5), "vector", small=False)


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("n", JOINT_GRIDS)
def test_joint_projector_matches_the_reference(sipx, TF, n):
    _all_bounds(sipx, Case("joint", n), TF)


def test_one_frame_is_a_2d_grid(sipx):
    g = sipx.compgrid((1.0, 1.0, 1.0), (8, 6, 1))
    for st in ("l2inf", "l2inf_joint"):
        with pytest.raises(sipx.SipxError) as e:
            sipx.Projector(sipx.set_definitions(st, "TV_xy", 0, 1.0, ("tensor", "")), g, np.float32)
        assert str(e.value) == sipx.host.TV_XY_NEEDS_3D
    case = Case("tv", (8, 6))
    v = case.input(np.float32)
    c = np.float32(0.5 * float(case.norms(v, np.float32).max()))
    y = sipx.Projector(sipx.set_definitions("l2inf", "TV", 0, c, ("tensor", "")), g, np.float32)(v.copy())
    assert l1_exact.same_bits(y, case.P(sipx, np.float32, c)(v.copy()))


# ---- bits that must stay -----------------------------------------------------------------------------------------------------------------------
def _x_case(sipx, which, TF):
    """(grid, x, TD_OP / joint / blocks of l2inf_norm, the set, A x and its Case) of one example in x-space."""
    if which == "tv2":
        n, args, sd = (33, 20), dict(TD_OP="TV"), ("l2inf", "TV")
    elif which == "tv3":
        n, args, sd = (8, 6, 5), dict(TD_OP="TV"), ("l2inf", "TV")
    elif which == "tv_xy":
        n, args, sd = (8, 6, 5), dict(TD_OP="TV_xy"), ("l2inf", "TV_xy")
    elif which == "joint":
        n, args, sd = (4, 3, 16), dict(TD_OP="TV_xy", joint=True), ("l2inf_joint", "TV_xy")
    else:
        n, args, sd = ((12, 9) if which == "hessian2" else (8, 6, 5)), dict(TD_OP="Hessian"), ("l2inf", "Hessian")
    g = sipx.compgrid(tuple(3.0 + a for a in range(len(n))), n)
    x = np.random.default_rng(5 + sum(n)).standard_normal(int(np.prod(n))).astype(TF)
    if which.startswith("hessian"):
        A = sipx.get_TD_operator(g, "Hessian", TF)[0]
        B = 3 if len(n) == 2 else 6
        case = Case("stacked", B=B, G=int(np.prod(n)))
    else:
        A = sipx.TDOperator(sd[1], g, TF)
        case = Case({"tv2": "tv", "tv3": "tv"}.get(which, which), n)
    return g, x, args, sd, np.asarray(A @ x, TF), case, n


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("which", ["tv2", "tv3", "tv_xy", "joint", "hessian2", "hessian3"])
def test_observed_bound_leaves_the_point_unwritten(sipx, TF, which):
    """c = sipx.l2inf_norm(x): A x comes back bit for bit; a little below it, it does not.  The observer equals the reference's maximum
    of the TF norms of the engine's own A x, and the device form gives the bits of the host form."""
    g, x, args, sd, v, case, n = _x_case(sipx, which, TF)
    c = sipx.l2inf_norm(x, g, **args)
    assert isinstance(c, TF)
    if not which.startswith("hessian"):      # (A x of the built-in operators is the front end's, bit for bit; the Hessian's on the device sums four terms a row)
        assert c == R.max_norm(v, case.idx, TF, case.jn)
    else:
        assert abs(float(c) - float(R.max_norm(v, case.idx, TF))) <= 8 * float(np.finfo(TF).eps) * float(c)
    mk = lambda b: sipx.Projector(sipx.set_definitions(sd[0], sd[1], 0, b, _mode(n)), g, TF)
    if not which.startswith("hessian"):
        assert l1_exact.same_bits(mk(float(c))(v.copy()), v), "v was written although its bound was observed on it"
        assert not l1_exact.same_bits(mk(float(c) * 0.999)(v.copy()), v)
    td = sipx.l2inf_norm(torch.from_numpy(x).cuda(), g, **args)
    assert td.is_cuda and td.shape == (1,) and l1_exact.same_bits(td.cpu().numpy(), np.array([c], TF))
    # in a solve: x is feasible for the bound observed on it, and comes back exactly
    opt = sipx.PARSDMM_options(FL=TF, maxit=20)
    P, A, prop = sipx.setup_constraints([sipx.set_definitions(sd[0], sd[1], 0, float(c), _mode(n))], g, TF)
    A, AtA, l, y = sipx.PARSDMM_precompute_distribute(A, prop, g, opt)
    xs, log, _, _ = sipx.PARSDMM(x.copy(), AtA, A, prop, P, g, opt)
    assert l1_exact.same_bits(xs, x), "a model feasible for its observed bound was changed"


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("kind,n", [("tv", (33, 20)), ("tv", (32, 12, 8)), ("tv_xy", (8, 6, 5)), ("joint", (4, 3, 16)), ("joint", (8, 6, 5))])
def test_every_group_on_its_bound_comes_back_bit_for_bit(sipx, TF, kind, n):
    case = Case(kind, n)
    v = case.input(TF)
    v[::7] = -0.0
    g = case.norms(v, TF)
    assert np.any(np.signbit(v) & (v == 0))
    assert l1_exact.same_bits(case.P(sipx, TF, g)(v.copy()), v)
    z = np.zeros_like(v)
    z[::2] = -0.0
    assert l1_exact.same_bits(case.P(sipx, TF, TF(1.0))(z.copy()), z)
    assert l1_exact.same_bits(case.P(sipx, TF, np.zeros(case.groups, TF))(z.copy()), z)


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("B,G", [(3, 256), (6, 1028), (8, 4), (2, 257)])
def test_stacked_groups_on_their_bound_come_back_bit_for_bit(sipx, TF, B, G):
    case = Case("stacked", B=B, G=G)
    v = case.input(TF)
    g = case.norms(v, TF)
    assert l1_exact.same_bits(case.P(sipx, TF, g)(v.copy()), v)
    assert l1_exact.same_bits(case.P(sipx, TF, TF(g.max()))(v.copy()), v)


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("kind,n,B,G", [("tv", (256, 5), None, None), ("tv", (8, 6, 5), None, None), ("tv_xy", (8, 6, 2), None, None),
                                        ("joint", (8, 6, 5), None, None), ("stacked", None, 3, 256), ("stacked", None, 8, 1028)])
def test_unclipped_groups_keep_their_bits_beside_clipped_ones(sipx, TF, kind, n, B, G):
    """Every second group gets half its norm as the bound, the others twice theirs: in every 16-byte vector clipped and unclipped groups
    lie side by side.  The unclipped ones keep their bits, -0.0 included; the clipped ones change."""
    case = Case(kind, n, B, G)
    v = case.input(TF)
    v[::5] = -0.0
    g = case.norms(v, TF)
    c = np.where(np.arange(case.groups) % 2 == 0, TF(0.5) * g, TF(2) * g).astype(TF)
    y = case.P(sipx, TF, c)(v.copy())
    changed = np.zeros(case.groups, bool)
    for q in range(case.m):
        has = case.idx[:, q] >= 0
        same = y[case.idx[has, q]].view(np.uint8).reshape(-1, v.itemsize) == v[case.idx[has, q]].view(np.uint8).reshape(-1, v.itemsize)
        changed[has] |= ~same.all(axis=1)
    odd = np.arange(case.groups) % 2 == 1
    assert not changed[odd].any(), "an unclipped group was written with other bits"
    assert changed[~odd & (g > 0)].all(), "a clipped group was left alone"


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("op,n", [("TV", (12, 9)), ("TV", (13, 7)), ("TV", (8, 6, 5)), ("TV_xy", (8, 6, 5))])
def test_pad_rows_are_untouched(sipx, TF, op, n):
    """The set inside a context whose y of that set is pre-filled is out of reach of the public calls; what they reach: the rows the
    blocks do not have never enter the norm -- so the result of sipx_project does not depend on what a neighbouring row holds -- and
    the projected M-vector has exactly the rows of the operator, each written from its own group."""
    case = Case("tv" if op == "TV" else "tv_xy", n)
    v = case.input(TF)
    c = TF(0.5 * float(case.norms(v, TF).max()))
    d = sipx.host._SetDesc()
    d.op, d.proj, d.pmin, d.pmax = sipx.host.OPS[op], sipx.host.PROJ["l2inf"], 0.0, float(c)
    ctx = sipx.Context(_grid(sipx, n), TF)
    try:
        w = v.copy()
        assert sipx.lib().sipx_project(ctx.h, C.byref(d), w.ctypes.data_as(C.c_void_p), C.c_int64(len(w))) == 0
        sentinel = np.full(len(v) + 8, TF(-7777.0))
        sentinel[4:-4] = v
        inner = sentinel[4:-4]
        assert sipx.lib().sipx_project(ctx.h, C.byref(d), inner.ctypes.data_as(C.c_void_p), C.c_int64(len(v))) == 0
    finally:
        ctx.close()
    assert l1_exact.same_bits(inner, w) and np.all(sentinel[:4] == TF(-7777.0)) and np.all(sentinel[-4:] == TF(-7777.0))
    ref = R.project(v, case.idx, c)
    assert np.all(np.abs(w.astype(np.float64) - ref) <= 4 * float(np.finfo(TF).eps) * np.abs(v.astype(np.float64)))


# ---- feasibility of the output, to the header's bound ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("which", ["tv2", "tv3", "tv_xy", "joint"])
def test_projected_vector_is_feasible_to_the_headers_bound(sipx, TF, which):
    """The norms the reference observes, in TF, on the projector's output are within l2inf_excess_units(m) (eps / 2) c of c, and the
    observer sipx.l2inf_norm of a projected x-space example -- the solve's result -- is within that bound and the solve's tolerance."""
    g, x, args, sd, v, case, n = _x_case(sipx, which, TF)
    u = float(np.finfo(TF).eps) / 2
    c = TF(0.3 * float(case.norms(v, TF).max()))
    y = sipx.Projector(sipx.set_definitions(sd[0], sd[1], 0, c, _mode(n)), g, TF)(v.copy())
    gy = case.norms(y, TF).astype(np.float64)
    worst = float((gy.max() / float(c) - 1) / u)
    print(f"feasibility {which} {np.dtype(TF).name}: the observed norm exceeds c by {worst:.3f} u c, the header allows {R.excess_units(TF, case.m):.2f}")
    assert np.all(gy <= float(c) * (1 + R.excess_units(TF, case.m) * u))
    opt = sipx.PARSDMM_options(FL=TF, maxit=200)
    P, A, prop = sipx.setup_constraints([sipx.set_definitions(sd[0], sd[1], 0, float(c), _mode(n))], g, TF)
    A, AtA, l, yy = sipx.PARSDMM_precompute_distribute(A, prop, g, opt)
    xs, log, _, _ = sipx.PARSDMM(x.copy(), AtA, A, prop, P, g, opt)
    seen = float(sipx.l2inf_norm(xs, g, **args))
    print(f"  solve: l2inf_norm(x) / c = {seen / float(c):.6f} after {len(log.obj)} iterations, feasibility {log.set_feasibility[-1]}")
    assert seen <= float(c) * (1 + R.excess_units(TF, case.m) * u) * (1 + 10 * float(opt.feas_tol))


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("B,G", [(2, 257), (3, 1028), (6, 256), (8, 1028)])
def test_observer_sees_a_projected_vector_within_the_headers_bound(sipx, TF, B, G):
    """On the identity as a stacked operator x is A x itself: sipx.l2inf_norm of the projector's output, observed by the device, is
    within l2inf_excess_units(B) (eps / 2) c of c -- no other slack."""
    case = Case("stacked", B=B, G=G)
    v = case.input(TF)
    M = B * G
    grid, A = sipx.compgrid((1.0, 1.0), (M, 1)), sp.identity(M, format="csc", dtype=TF)
    u = float(np.finfo(TF).eps) / 2
    top = float(sipx.l2inf_norm(v, grid, A, blocks=B))
    assert top == float(case.norms(v, TF).max())
    for frac in FRACS:
        c = TF(frac * top)
        y = case.P(sipx, TF, c)(v.copy())
        seen = float(sipx.l2inf_norm(y, grid, A, blocks=B))
        print(f"observer B {B} G {G} {np.dtype(TF).name} frac {frac}: exceeds c by {(seen / float(c) - 1) / u:.3f} u c, allowed {R.excess_units(TF, B):.2f}")
        assert seen <= float(c) * (1 + R.excess_units(TF, B) * u)
        assert seen >= float(c) * (1 - R.excess_units(TF, B) * u), "the largest group was clipped onto its bound"


# ---- set_data ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("which", ["tv2", "joint", "hessian2"])
def test_set_data_gives_the_bits_of_a_new_context(sipx, TF, which):
    g, x, args, sd, v, case, n = _x_case(sipx, which, TF)
    gn = case.norms(v, TF)
    c1 = np.maximum(TF(0.8) * gn, TF(0.1) * gn.max()).astype(TF)
    c2 = np.maximum(TF(0.4) * gn, TF(0.05) * gn.max()).astype(TF)
    opt = sipx.PARSDMM_options(FL=TF, maxit=25)

    def solver(c):
        cons = [sipx.set_definitions("bounds", "identity", -10.0, 10.0, _mode(n)), sipx.set_definitions(sd[0], sd[1], 0, c, _mode(n))]
        P, A, prop = sipx.setup_constraints(cons, g, TF)
        A, AtA, l, y = sipx.PARSDMM_precompute_distribute(A, prop, g, opt)
        return sipx.Solver(AtA, A, prop, P, g, opt, TF)
    S = solver(c1)
    try:
        x1 = S(x.copy())[0].copy()
        S.set_data(1, ub=c2)
        x2 = S(x.copy())[0].copy()
        with pytest.raises(sipx.SipxError, match="entries"):
            S.set_data(1, ub=c2[:-1])
        with pytest.raises(sipx.SipxError, match="takes no weights"):
            S.set_data(1, lb=c2)
        with pytest.raises(sipx.SipxError, match="negative or NaN"):
            S.set_data(1, ub=np.r_[c2[:3], TF(-1), c2[4:]].astype(TF))
    finally:
        S.close()
    S = solver(c2)
    try:
        x2_new = S(x.copy())[0].copy()
    finally:
        S.close()
    assert l1_exact.same_bits(x2, x2_new), "set_data then reset differs from a new context"
    assert not l1_exact.same_bits(x1, x2)
    S = solver(float(gn.max()) * 0.5)
    try:
        with pytest.raises(sipx.SipxError, match="scalar bound"):
            S.set_data(1, ub=c2)
    finally:
        S.close()


# ---- whole solves against the oracle ----------------------------------------------------------------------------------------------------------
SOLVE_SETS = {"l2inf-TV": ["l2inf"], "l1-TV+l2inf-TV": ["l1", "l2inf"], "l2inf-joint": ["joint"], "l2inf-Hessian": ["hessian"]}
SOLVE_GRIDS = [((12, 9), (25.0, 6.0)), ((16, 16), (1.0, 1.0)), ((8, 6, 5), (25.0, 25.0, 25.0)), ((8, 8, 4), (1.0, 2.0, 3.0))]
SOLVE_CASES = [(name, n, h) for name in SOLVE_SETS for n, h in SOLVE_GRIDS if name != "l2inf-joint" or len(n) == 3]


def _solve_problem(mod, sipx, name, n, h, TF, m, opt_kw, scale=0.5):
    """{bounds, the sets of SOLVE_SETS[name]} for module `mod`; c = scale times the largest group norm of A m from the reference.  The
    oracle takes the l1 ball on the same operator (TV_xy and the Hessian as caller-supplied operators), whose projector is then
    replaced by the reference's."""
    g = mod.compgrid(h, n)
    opt = mod.PARSDMM_options(FL=TF, **opt_kw)
    c = [mod.set_definitions("bounds", "identity", 1600.0, 3900.0, _mode(n))]
    swaps = []
    for kind in SOLVE_SETS[name]:
        if kind == "l1":
            s = np.asarray(O.get_TD_operator(O.compgrid(h, n), "TV", TF)[0] @ m, TF)
            c.append(mod.set_definitions("l1", "TV", 0.0, float(TF(0.5 * np.abs(s.astype(np.float64)).sum())), _mode(n)))
            continue
        if kind == "l2inf":
            A, idx, jn, sd = O.get_TD_operator(O.compgrid(h, n), "TV", TF)[0], R.layout_tv(n), None, ("l2inf", "TV")
        elif kind == "joint":
            A, idx, jn, sd = TFR._stacked(n, h, TF), R.layout_joint(n), n, ("l2inf_joint", "TV_xy")
        else:
            A = sipx.get_TD_operator(sipx.compgrid(h, n), "Hessian", TF)[0].A
            idx, jn, sd = R.layout_stacked(A.shape[0], 3 if len(n) == 2 else 6), None, ("l2inf", "Hessian")
        r = TF(scale * float(R.max_norm(np.asarray(A @ m, TF), idx, TF, jn)))
        if mod is O:
            swaps.append((len(c), lambda x, r=r, idx=idx, jn=jn: TS._in_place(lambda t: R.project(t, idx, r, jn), x)))
            if kind == "l2inf":
                c.append(mod.set_definitions("l1", "TV", 0.0, float(r), _mode(n)))
            else:
                c.append(mod.set_definitions("l1", "identity", 0.0, float(r), _mode(n), (A, False)))
        else:
            c.append(mod.set_definitions(sd[0], sd[1], 0, float(r), _mode(n)))
    P, A, prop = mod.setup_constraints(c, g, TF)
    for i, f in swaps:
        P[i] = f
    A, AtA, l, y = mod.PARSDMM_precompute_distribute(A, prop, g, opt)
    return g, opt, P, A, prop, AtA


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("name,n,h", SOLVE_CASES)
def test_solve_matches_oracle(sipx, TF, name, n, h):
    m = TS._model(n, TF, seed=1 + len(SOLVE_SETS[name]))
    kw = dict(maxit=60)
    go, oo, Po, Ao, propo, AtAo = _solve_problem(O, sipx, name, n, h, TF, m, kw)
    gs, os_, Ps, As, props, AtAs = _solve_problem(sipx, sipx, name, n, h, TF, m, kw)
    assert props.ncvx == propo.ncvx
    xo, lo, l_o, y_o = O.PARSDMM(m.copy(), AtAo, Ao, propo, Po, go, oo)
    xs, ls, l_s, y_s = sipx.PARSDMM(m.copy(), AtAs, As, props, Ps, gs, os_)

    def replay(maxit, hist):
        gr, orr, Pr, Ar, propr, AtAr = _solve_problem(O, sipx, name, n, h, TF, m, dict(kw, maxit=maxit))
        return O.PARSDMM(m.copy(), AtAr, Ar, propr, Pr, gr, orr, replay=hist)[0]
    TS._compare(name, n, TF, ls, lo, xs, xo, os_, replay)
    p = len(SOLVE_SETS[name]) + 2
    assert ls.r_pri.shape == (len(ls.obj), p) and ls.set_feasibility.shape[1] == p - 1
    assert len(y_s) == p and [len(q) for q in y_s] == [len(q) for q in y_o]


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("name,n,h", [("l2inf-TV", (12, 9), (25.0, 6.0)), ("l2inf-joint", (8, 6, 5), (25.0, 25.0, 25.0)),
                                      ("l2inf-Hessian", (16, 16), (1.0, 1.0))])
def test_feasible_model_comes_back_exactly(sipx, TF, name, n, h):
    m = TS._model(n, TF, seed=4)
    kw = dict(maxit=60)
    go, oo, Po, Ao, propo, AtAo = _solve_problem(O, sipx, name, n, h, TF, m, kw, scale=2.0)
    gs, os_, Ps, As, props, AtAs = _solve_problem(sipx, sipx, name, n, h, TF, m, kw, scale=2.0)
    xo, lo, _, _ = O.PARSDMM(m.copy(), AtAo, Ao, propo, Po, go, oo)
    xs, ls, _, _ = sipx.PARSDMM(m.copy(), AtAs, As, props, Ps, gs, os_)
    assert np.array_equal(xo, m.astype(xo.dtype)) and l1_exact.same_bits(xs, m)
    assert len(ls.obj) == len(lo.obj), "both take the feasible-input exit"


# ---- the caller-supplied two-block operator [D_x; D_z], zero-padded to N rows each: the groups of ("l2inf", "TV") --------------------------------
@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("form", ["scalar", "vector"])
def test_two_block_gradient_reproduces_l2inf_on_tv(sipx, TF, form):
    """The tolerance is the one the twin test of the stacked l2,1 ball is held to (tests/test_gpu_l21_stacked.py,
    test_two_block_gradient_reproduces_isotropic_tv): 5e-4 in Float32, 1e-6 in Float64, relative in x."""
    n, h = (12, 9), (25.0, 6.0)
    m = TS._model(n, TF, seed=5)
    g = sipx.compgrid(h, n)
    opt = sipx.PARSDMM_options(FL=TF, maxit=60)
    TV = O.get_TD_operator(O.compgrid(h, n), "TV", TF)[0]
    gn = R.norms(np.asarray(TV @ m, TF), R.layout_tv(n), TF)
    c = float(TF(0.5 * gn.max())) if form == "scalar" else np.maximum(TF(0.5) * gn, TF(0.05) * gn.max()).astype(TF)
    A2 = TS._padded_gradient(n, h, TF)
    assert np.array_equal(R.norms(A2 @ m, R.layout_stacked(216, 2), TF), gn) or \
        np.allclose(R.norms(A2 @ m, R.layout_stacked(216, 2), TF), gn, rtol=4 * float(np.finfo(TF).eps)), "the same groups"
    xs = {}
    for which in ("tv", "stacked"):
        cons = [sipx.set_definitions("bounds", "identity", 1600.0, 3900.0, ("matrix", ""))]
        if which == "tv":
            cons.append(sipx.set_definitions("l2inf", "TV", 0, c, ("matrix", "")))
        else:
            cons.append(sipx.set_definitions("l2inf_stacked", "gradient", 0, c, ("matrix", ""), custom_TD_OP=(A2, False), blocks=2))
        P, A, prop = sipx.setup_constraints(cons, g, TF)
        A, AtA, l, y = sipx.PARSDMM_precompute_distribute(A, prop, g, opt)
        x, log, l, y = sipx.PARSDMM(m.copy(), AtA, A, prop, P, g, opt)
        assert len(log.obj) > 6
        xs[which] = (x.astype(np.float64), log)
    err = np.linalg.norm(xs["stacked"][0] - xs["tv"][0]) / np.linalg.norm(xs["tv"][0])
    print(f"two-block gradient {form} {np.dtype(TF).name}: iterations {len(xs['stacked'][1].obj)} / {len(xs['tv'][1].obj)}, rel diff {err:.3e}")
    assert err < (5e-4 if TF == np.float32 else 1e-6), err


# ---- the engine's refusals through the C ABI ---------------------------------------------------------------------------------------------------
def _desc(sipx, proj, op, A=None, blocks=0, pmin=0.0, pmax=1.0, mode=0, dir=0, transform=0, component=0, lb=None, ub=None, reserved=0):
    d = sipx.host._SetDesc()
    d.op, d.proj, d.pmin, d.pmax, d.mode, d.dir, d.transform, d.component, d.blocks = op, proj, pmin, pmax, mode, dir, transform, component, blocks
    keep = [lb, ub]
    d.reserved = reserved
    if lb is not None:
        d.lb = lb.ctypes.data
    if ub is not None:
        d.ub = ub.ctypes.data
    if A is not None:
        cp, ri, nz = (np.ascontiguousarray(A.indptr, np.int64), np.ascontiguousarray(A.indices, np.int64), np.ascontiguousarray(A.data))
        d.csc_colptr, d.csc_rowval, d.csc_nzval, d.csc_rows = cp.ctypes.data, ri.ctypes.data, nz.ctypes.data, A.shape[0]
        keep += [cp, ri, nz]
    return d, keep


def _refused(sipx, ctx, dk):
    rc = sipx.lib().sipx_add_set(ctx.h, C.byref(dk[0]), None, None, 0)
    assert rc < 0, "the engine took the set"
    return sipx.lib().sipx_last_error().decode()


def test_engine_refusals(sipx):
    TF = np.float32
    Hm = sipx.host
    TV, XY, CSC = Hm.OPS["TV"], Hm.OPS["TV_xy"], Hm.OPS["custom"]
    g2, g3 = sipx.compgrid((1.0, 1.0), (12, 9)), sipx.compgrid((1.0, 1.0, 1.0), (8, 6, 5))
    H = sipx.get_TD_operator(g2, "Hessian", TF)[0].A
    ones = lambda k: np.ones(k, TF)
    ctx = sipx.Context(g2, TF)
    try:
        D = lambda **kw: _desc(sipx, 24, TV, **kw)
        S = lambda **kw: _desc(sipx, 26, CSC, A=H, blocks=3, **kw)
        assert _refused(sipx, ctx, D(pmin=0.5)) == Hm.L2INF_MIN
        for c in (0.0, -2.0, float("nan")):
            assert _refused(sipx, ctx, D(pmax=c)) == Hm.L2INF_BAD_C
            assert _refused(sipx, ctx, S(pmax=c)) == Hm.L2INF_BAD_C
        bad = ones(108)
        bad[5] = -1
        assert _refused(sipx, ctx, D(ub=bad, reserved=108)) == Hm.l2inf_bad_entry(5)
        bad[5] = np.nan
        assert _refused(sipx, ctx, S(ub=bad, reserved=108)) == Hm.l2inf_bad_entry(5)
        assert _refused(sipx, ctx, D(ub=ones(107), reserved=107)) == Hm.l2inf_bad_length(107, 108)
        assert _refused(sipx, ctx, S(ub=ones(324), reserved=324)) == Hm.l2inf_bad_length(324, 108)
        assert _refused(sipx, ctx, D(mode=1)) == Hm.L2INF_MODES
        assert _refused(sipx, ctx, S(mode=2)) == Hm.L2INF_MODES
        assert _refused(sipx, ctx, D(transform=1)) == Hm.L2INF_NO_TRANSFORM
        assert _refused(sipx, ctx, D(lb=ones(108), reserved=108)) == Hm.L2INF_NO_WEIGHTS
        assert _refused(sipx, ctx, D(component=1)) == Hm.L2INF_NO_MINKOWSKI
        assert _refused(sipx, ctx, _desc(sipx, 24, Hm.OPS["D_z"])) == Hm.L2INF_NEEDS_TV
        assert _refused(sipx, ctx, _desc(sipx, 24, CSC, A=H, blocks=3)) == Hm.L2INF_NEEDS_TV
        assert _refused(sipx, ctx, _desc(sipx, 26, TV, blocks=2)) == Hm.L2INF_STACKED_NEEDS_CSC
        assert _refused(sipx, ctx, _desc(sipx, 26, CSC, A=H, blocks=5)) == Hm.l2inf_bad_rows(324, 5)
        assert _refused(sipx, ctx, _desc(sipx, 26, CSC, A=H, blocks=9)) == Hm.l2inf_bad_blocks(9)
        # sets the engine takes; set_data: a scalar set holds nothing to replace, a vector set refuses lb and a bad entry
        d0, d1 = D(), D(ub=ones(108), reserved=108)
        assert sipx.lib().sipx_add_set(ctx.h, C.byref(d0[0]), None, None, 0) == 0
        assert sipx.lib().sipx_add_set(ctx.h, C.byref(d1[0]), None, None, 0) == 1
        ub = ones(108)
        err = lambda: sipx.lib().sipx_last_error().decode()
        assert sipx.lib().sipx_set_data(ctx.h, 0, None, ub.ctypes.data_as(C.c_void_p)) != 0 and Hm.L2INF_NO_SET_DATA in err()
        assert sipx.lib().sipx_set_data(ctx.h, 1, ub.ctypes.data_as(C.c_void_p), None) != 0 and Hm.L2INF_NO_WEIGHTS in err()
        ub[9] = -3
        assert sipx.lib().sipx_set_data(ctx.h, 1, None, ub.ctypes.data_as(C.c_void_p)) != 0 and Hm.l2inf_bad_entry(9) in err()
        ub[9], ub[107] = 3, -3      # (the last corner has no member)
        assert sipx.lib().sipx_set_data(ctx.h, 1, None, ub.ctypes.data_as(C.c_void_p)) == 0
        # sipx_project: the length of the M-vector
        v = np.zeros(108, TF)
        assert sipx.lib().sipx_project(ctx.h, C.byref(d0[0]), v.ctypes.data_as(C.c_void_p), C.c_int64(len(v))) != 0
        assert "the TV range: 195 entries on this grid, 108 given" in err()
        s0 = _desc(sipx, 26, CSC, blocks=3)
        v = np.zeros(325, TF)
        assert sipx.lib().sipx_project(ctx.h, C.byref(s0[0]), v.ctypes.data_as(C.c_void_p), C.c_int64(len(v))) != 0 and err() == Hm.l2inf_bad_rows(325, 3)
        out = np.zeros(1, TF)
        x = np.zeros(108, TF)
        bad_d = _desc(sipx, 14, TV)
        assert sipx.lib().sipx_l2inf_norm(ctx.h, C.byref(bad_d[0]), x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) != 0
        assert "SIPX_PROJ_L2INF" in err()
    finally:
        ctx.close()
    ctx = sipx.Context(g3, TF)
    try:
        assert _refused(sipx, ctx, _desc(sipx, 25, TV)) == Hm.L2INF_JOINT_ROUTE
        assert _refused(sipx, ctx, _desc(sipx, 25, XY, mode=2, dir=2)) == Hm.L2INF_MODES
        assert _refused(sipx, ctx, _desc(sipx, 24, XY, mode=2, dir=2)) == Hm.L2INF_MODES
        assert _refused(sipx, ctx, _desc(sipx, 25, XY, ub=ones(240), reserved=240)) == Hm.l2inf_bad_length(240, 48)
        assert sipx.lib().sipx_add_set(ctx.h, C.byref(_desc(sipx, 25, XY, ub=ones(48), reserved=48)[0]), None, None, 0) == 0
    finally:
        ctx.close()
    ctx = sipx.Context(g2, TF)
    try:
        ctx.set_decomp("slab")
        assert _refused(sipx, ctx, _desc(sipx, 24, TV)) == Hm.L2INF_SHARDED
        assert _refused(sipx, ctx, _desc(sipx, 26, CSC, A=H, blocks=3)) == Hm.L2INF_SHARDED
    finally:
        ctx.close()
    P = sipx.Projector(sipx.set_definitions("l2inf", "TV", 0, 1.0, ("matrix", "")), g2, TF)
    for late in ("slab", "owned"):
        ctx = sipx.Context(g2, TF)
        try:
            ctx.add_set(sipx.TDOperator("TV", g2, TF), P)
            if late == "slab":
                ctx.set_decomp("slab")
            else:
                ctx.set_owned([1, 1])
            with pytest.raises(sipx.SipxError, match="takes single-process contexts only"):
                ctx.finalize(np.ones(108, TF), [10.0], 1.0)
        finally:
            ctx.close()
