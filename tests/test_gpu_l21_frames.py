"""Per-frame isotropic total variation on the GPU: the TV_xy operator and the ("l21", "TV_xy") sets, whole array and per z-slice
(csrc/l21_seg.h, csrc/ext_group.hip), against tests/l21_frames_ref.py: the operator against the stacked D_y, D_x, the projector with
per-frame and scalar radii, exact ties with a different threshold in every frame, inputs it must not write, observed radii
(sipx.l21_norm), new radii in a live context, whole solves against the oracle on the same operator given as custom_TD_OP with its
projector swapped for the reference, and the engine's refusals through the C ABI.

GRIDS and the path each takes (l21_seg_plan: a frame of L = n1 n2 group norms stays in LDS when L sizeof(T) <= SEGN_LDS_BYTES = 32768;
the norms / scale kernels take 16 bytes per thread when n1 % 4 == 0 and launch min(ceil(points / (256 VW)), 2048) workgroups):
  (4, 3, 2), (5, 4, 3)   every boundary class; one point per thread; LDS in both precisions
  (33, 20, 3)            odd n1, one point per thread, more than one workgroup; L = 660: LDS in both precisions
  (32, 12, 8)            16-byte path; L = 384: LDS in both precisions; more frames than any other grid
  (96, 86, 3)            L = 8256 entries = 33 024 bytes in Float32, the smallest n2 at n1 = 96 beyond the budget (96 * 85 * 4 = 32 640
                         fits): streaming in Float32 and hence in Float64
  (1024, 1028, 2)        2 105 344 points > 2048 * 256 * 4 = 2 097 152: a second, partial grid-stride sweep of the norms / scale kernels
                         in both precisions; streaming frames of 1 052 672 entries
Worst |y - ref| / (eps |v|) observed on an MI355X: see DESIGN.md section 7e."""
import ctypes as C

import numpy as np
import pytest
import torch      # (before libsipx.so is loaded: one HIP runtime in the process)

from oracle import parsdmm_oracle as O
from tests import l1_exact, l21_frames_ref as R
from tests.test_gpu_set_data import _assert_same, _rho_gamma

pytestmark = pytest.mark.gpu

SEGN_LDS_BYTES = 32 * 1024
GRIDS = [(4, 3, 2), (5, 4, 3), (33, 20, 3), (32, 12, 8), (96, 86, 3), (1024, 1028, 2)]
FRACS = [0.9, 2.0, 0.05, 0.5]             # of the frame's own norm, rotated by the pattern number: every call has a frame inside its ball
PRECISIONS = [np.float32, np.float64]
_inputs, _refs = {}, {}


def _grid(sipx, n):
    return sipx.compgrid(tuple(1.0 for _ in n), n)


def _P(sipx, n, TF, tau, mode=("slice", "z")):
    return sipx.Projector(sipx.set_definitions("l21", "TV_xy", 0.0, tau if np.ndim(tau) else float(tau), mode), _grid(sipx, n), TF)


def make_input(n, TF):
    """(v, per-frame norms): heavy-tailed randn * exp(randn) on every row of the M-vector, the frames scaled apart; computed once,
    handed out as a copy."""
    key = (n, np.dtype(TF).name)
    if key not in _inputs:
        rng = np.random.default_rng(20250601 + sum(n))
        M = R.rows(n)
        v = rng.standard_normal(M) * np.exp(rng.standard_normal(M))
        for k in range(n[2]):
            v[R.frame_rows(n, k)] *= 1.0 + 0.75 * k
        v = v.astype(TF)
        _inputs[key] = (v, R.frame_norms(v, n))
    v, nrm = _inputs[key]
    return v.copy(), nrm.copy()


def _radii(n, TF, nrm, pattern):
    fr = np.array([FRACS[(k + pattern) % 4] for k in range(n[2])])
    return (fr * nrm).astype(TF), fr


def _reference(n, TF, pattern):
    key = (n, np.dtype(TF).name, pattern)
    if key not in _refs:
        v, nrm = make_input(n, TF)
        b, fr = _radii(n, TF, nrm, pattern)
        ref = R.project(v, n, b)
        ref.setflags(write=False)
        _refs[key] = (b, fr, ref, R.inside(v, n, b))
    return _refs[key]


def test_the_grids_take_the_paths_the_docstring_names():
    assert 96 * 86 * 4 > SEGN_LDS_BYTES >= 96 * 85 * 4 and 96 % 4 == 0, "the streaming grid is the first beyond the budget in Float32"
    for n in GRIDS[:4]:
        assert n[0] * n[1] * 8 <= SEGN_LDS_BYTES
    n = GRIDS[-1]
    assert n[0] % 4 == 0 and int(np.prod(n)) // 4 > 2048 * 256 and int(np.prod(n)) // 2 > 2048 * 256, "a second sweep in both precisions"
    assert (1024 * 1024 * 2) // 4 <= 2048 * 256


# ---- 1. the operator -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("n", [(5, 4, 3), (32, 12, 8)])
def test_operator_equals_the_stacked_Dy_Dx(sipx, TF, n):
    g = sipx.compgrid((25.0, 10.0, 6.0), n)
    rng = np.random.default_rng(7)
    x = rng.standard_normal(int(np.prod(n))).astype(TF)
    A = sipx.TDOperator("TV_xy", g, TF)
    Dy, Dx = sipx.TDOperator("D_y", g, TF), sipx.TDOperator("D_x", g, TF)
    assert l1_exact.same_bits(A @ x, np.concatenate([Dy @ x, Dx @ x]))
    # the adjoint: a column of vcat(D_y, D_x) is added up in ascending row order, D_y's rows first -- the sparse product of the stack
    w = rng.standard_normal(A.shape[0]).astype(TF)
    my = Dy.shape[0]
    got = A.T @ w
    M = _stacked(n, (25.0, 10.0, 6.0), TF)
    M.sort_indices()
    assert got.dtype == TF and l1_exact.same_bits(got, np.asarray(M.T @ w, TF))
    # ... and D_y' w_y + D_x' w_x of the existing operators up to the order of the four terms of a column: at most three roundings of
    # half an ulp of a partial sum on either side
    a, b = Dy.T @ w[:my], Dx.T @ w[my:]
    terms = np.asarray(abs(M).T @ np.abs(w), np.float64)
    assert np.all(np.abs(got - (a.astype(np.float64) + b)) <= 3 * float(np.finfo(TF).eps) * terms)


# ---- 2. the projector against the reference ------------------------------------------------------------------------------------------
def _check(v, y, ref, n, TF, inside, tag):
    eps = float(np.finfo(TF).eps)
    a = np.abs(v.astype(np.float64))
    err = np.abs(y.astype(np.float64) - ref)
    worst = float(np.max(err / np.maximum(a, np.finfo(np.float64).tiny)) / eps)
    print(f"l21 frames {tag} {n} {np.dtype(TF).name}: worst error {worst:.3f} eps |v|")
    assert np.all(err <= 4 * eps * a), f"worst error {worst:.3f} eps |v|"
    for k in np.nonzero(inside > 0)[0]:
        mem = R.frame_rows(n, k)
        assert l1_exact.same_bits(y[mem], v[mem]), f"frame {k} lies inside its ball and was written"
    return worst


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("pattern", [0, 1])
@pytest.mark.parametrize("n", GRIDS)
def test_projector_matches_the_reference_with_per_frame_radii(sipx, TF, pattern, n):
    if n == GRIDS[-1] and pattern:
        pattern = 3                                   # (one more pattern on the large grid: both frames outside, 0.5 and 0.9)
    v, nrm = make_input(n, TF)
    b, fr, ref, inside = _reference(n, TF, pattern)
    assert np.array_equal(inside, np.where(fr > 1, 1, -1)), "a frame too close to its radius to call"
    assert pattern == 3 or (inside > 0).any()
    P = _P(sipx, n, TF, b)
    y = P(v.copy())
    _check(v, y, ref, n, TF, inside, f"pattern {pattern}")
    assert l1_exact.same_bits(P(v.copy()), y), "two calls differ"


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("n", GRIDS[:5])
def test_projector_matches_the_reference_with_a_scalar_radius(sipx, TF, n):
    v, nrm = make_input(n, TF)
    b = TF(0.5 * (nrm.min() + nrm.max())) if n[2] > 2 else TF(0.7 * nrm.max())      # the lightest frame inside, the heaviest outside
    inside = R.inside(v, n, b)
    assert (inside != 0).all() and (inside < 0).any() and ((inside > 0).any() or n[2] <= 2)
    ref = R.project(v, n, b)
    P = _P(sipx, n, TF, b)
    y = P(v.copy())
    _check(v, y, ref, n, TF, inside, "scalar")
    assert l1_exact.same_bits(P(v.copy()), y), "two calls differ"
    # a vector whose entries all equal the scalar gives the same bits
    assert l1_exact.same_bits(_P(sipx, n, TF, np.full(n[2], b, TF))(v.copy()), y)


# ---- 3. the whole-array set on TV_xy ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("frac", [0.9, 0.5, 0.05])
@pytest.mark.parametrize("n", [(5, 4, 3), (32, 12, 8)])
def test_whole_array_set_matches_the_reference(sipx, TF, frac, n):
    v, nrm = make_input(n, TF)
    b = TF(frac * R.norm21(v, n))
    ref = R.project_whole(v, n, b)
    assert ref is not v
    P = _P(sipx, n, TF, b, ("tensor", ""))
    y = P(v.copy())
    _check(v, y, ref, n, TF, np.array([-1]), f"whole frac {frac}")
    assert l1_exact.same_bits(P(v.copy()), y)
    big = TF(2 * R.norm21(v, n))
    assert l1_exact.same_bits(_P(sipx, n, TF, big, ("tensor", ""))(v.copy()), v)
    tau = sipx.l21_norm(np.zeros(int(np.prod(n)), TF), _grid(sipx, n), "TV_xy")
    assert isinstance(tau, TF) and tau == 0


# ---- 4. ties: integer components, exact norms, a different exact threshold in every frame --------------------------------------------------
def _tie_input(n, TF):
    """Frame k holds 4 groups of norm 7 k', 9 of norm 5 k' (3-4-5 and axis-aligned), the rest norm k' or none, k' = k + 1: radius 8 k'
    puts theta_k = 5 k' exactly."""
    G = R.groups(n).reshape(n[0] * n[1], n[2], 2, order="F")
    v = np.zeros(R.rows(n), TF)
    kind = np.zeros((n[0] * n[1], n[2]), int)
    sevens = [(7, 0), (0, 7), (-7, 0), (0, -7)]
    fives = [(3, 4), (5, 0), (4, -3), (0, 5), (-3, 4), (-5, 0), (4, 3), (0, -5), (3, -4)]
    for k in range(n[2]):
        s = k + 1
        full = np.nonzero((G[:, k, :] >= 0).all(axis=1))[0]
        pick = np.random.default_rng(41 + k).permutation(full)
        for p in range(G.shape[0]):
            mem = G[p, k][G[p, k] >= 0]
            if len(mem):
                v[mem[p % len(mem)]] = -s if p % 3 == 0 else s
                kind[p, k] = 1
        for p, comp in zip(pick, sevens + fives):
            v[G[p, k]] = np.array(comp) * s
            kind[p, k] = 7 if 7 in np.abs(comp) else 5
    return v, G, kind


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("n", [(8, 6, 5), (9, 7, 3)])
def test_groups_on_their_frames_threshold_are_zeroed(sipx, TF, n):
    v, G, kind = _tie_input(n, TF)
    g = R.norms(v, n, TF)
    scale = np.arange(1, n[2] + 1)
    assert np.array_equal(g, (kind * scale[None, :]).astype(TF)) and np.all((kind == 7).sum(axis=0) == 4) and np.all((kind == 5).sum(axis=0) == 9)
    b = (8.0 * scale).astype(TF)
    for k in range(n[2]):
        assert l1_exact.exact_theta(g[:, k].astype(np.float64), b[k])[0] == 5.0 * scale[k]
    y = _P(sipx, n, TF, b)(v.copy())
    for k in range(n[2]):
        for kk in (5, 1):
            mem = G[kind[:, k] == kk, k]
            assert np.all(y[mem[mem >= 0]] == 0), f"frame {k}: a group of norm {kk * scale[k]} survived"
        mem = G[kind[:, k] == 7, k]
        mem = mem[mem >= 0]
        want = v[mem].astype(np.float64) * (2.0 / 7.0)
        assert np.all(np.abs(y[mem] - want) <= 4 * float(np.finfo(TF).eps) * np.abs(v[mem])), f"frame {k} took a neighbour's threshold"
    assert np.count_nonzero(y) == 4 * n[2]


# ---- 5. inputs the projector must not write ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("n", [(33, 20, 3), (32, 12, 8)])
def test_feasible_and_zero_inputs_come_back_bit_for_bit(sipx, TF, n):
    v, _ = make_input(n, TF)
    v[::7] = -0.0
    v[3::11] = 0.0
    b = (2 * R.frame_norms(v, n)).astype(TF)
    assert (R.inside(v, n, b) > 0).all() and np.any(np.signbit(v) & (v == 0))
    assert l1_exact.same_bits(_P(sipx, n, TF, b)(v.copy()), v)
    assert l1_exact.same_bits(_P(sipx, n, TF, float(b.max()))(v.copy()), v)
    z = np.zeros_like(v)
    z[::2] = -0.0
    assert l1_exact.same_bits(_P(sipx, n, TF, b)(z.copy()), z)
    assert l1_exact.same_bits(_P(sipx, n, TF, float(b.min()), ("tensor", ""))(z.copy()), z)


# ---- 6. observed radii -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("n", [(33, 20, 3), (32, 12, 8), (96, 86, 3)])
def test_observed_radii_leave_the_point_unwritten(sipx, TF, n):
    g = sipx.compgrid((3.0, 4.0, 5.0), n)
    x = np.random.default_rng(5 + sum(n)).standard_normal(n)
    x *= (1.0 + np.arange(n[2]))[None, None, :]
    x = x.reshape(-1, order="F").astype(TF)
    v = sipx.TDOperator("TV_xy", g, TF) @ x
    eps = float(np.finfo(TF).eps)
    tau = sipx.l21_norm(x, g, "TV_xy", ("slice", "z"))
    assert isinstance(tau, np.ndarray) and tau.dtype == TF and tau.shape == (n[2],)
    ref = R.frame_norms(v, n, TF)
    assert np.all(np.abs(tau.astype(np.float64) - ref) <= 2 * eps * ref)
    P = sipx.Projector(sipx.set_definitions("l21", "TV_xy", 0.0, tau, ("slice", "z")), g, TF)
    assert l1_exact.same_bits(P(v.copy()), v), "TV_xy x was written although its radii were observed on x"
    td = sipx.l21_norm(torch.from_numpy(x).cuda(), g, "TV_xy", ("slice", "z"))
    assert td.is_cuda and td.shape == (n[2],) and l1_exact.same_bits(td.cpu().numpy(), tau)
    y = sipx.Projector(sipx.set_definitions("l21", "TV_xy", 0.0, (tau * TF(0.999)).astype(TF), ("slice", "z")), g, TF)(v.copy())
    for k in range(n[2]):
        mem = R.frame_rows(n, k)
        assert not l1_exact.same_bits(y[mem], v[mem]), f"frame {k} was not projected"
    # the scalar form
    t1 = sipx.l21_norm(x, g, "TV_xy")
    assert isinstance(t1, TF) and abs(float(t1) - ref.sum()) <= 2 * eps * ref.sum()
    P1 = sipx.Projector(sipx.set_definitions("l21", "TV_xy", 0.0, float(t1), ("tensor", "")), g, TF)
    assert l1_exact.same_bits(P1(v.copy()), v)
    assert not l1_exact.same_bits(sipx.Projector(sipx.set_definitions("l21", "TV_xy", 0.0, float(t1) * 0.999, ("tensor", "")), g, TF)(v.copy()), v)
    t1d = sipx.l21_norm(torch.from_numpy(x).cuda(), g, "TV_xy")
    assert t1d.is_cuda and t1d.shape == (1,) and l1_exact.same_bits(t1d.cpu().numpy(), np.array([t1], TF))
    assert l1_exact.same_bits(sipx.l21_norm(x, g, "TV_xy", ("tensor", "")), t1)


# ---- whole solves ---------------------------------------------------------------------------------------------------------------------------
def _model(n, TF, seed):
    rng = np.random.default_rng(20240601 + seed)
    z = np.linspace(0, 1, n[-1]).reshape((1,) * (len(n) - 1) + (-1,))
    return (1500 + 2500 * z + 150 * rng.standard_normal(n)).astype(TF).reshape(-1, order="F")


def _julia_max(v):
    v = np.asarray(v, np.float64)
    return float("nan") if np.isnan(v).any() else float(v.max())


def _stacked(n, h, TF):
    import scipy.sparse as sp
    g = O.compgrid(h, n)
    return sp.vstack([O.get_TD_operator(g, "D_y", TF)[0], O.get_TD_operator(g, "D_x", TF)[0]]).tocsc()


def _in_place(f, x, *a):
    y = f(x, *a)
    if y is not x:
        x[:] = y
    return x


# ---- 7. new radii in a live context ----------------------------------------------------------------------------------------------------------
KW = dict(maxit=30, evol_rel_tol=0.0, feas_tol=0.0, obj_tol=0.0)      # every iteration runs
LIVE_N, LIVE_H = (24, 20, 6), (25.0, 25.0, 25.0)


def _live_setup(sipx, TF, k):
    m = (_model(LIVE_N, TF, seed=40 + k) * TF(1.0 - 0.03 * k)).astype(TF)
    g = sipx.compgrid(LIVE_H, LIVE_N)
    opt = sipx.PARSDMM_options(FL=TF, **KW)
    nrm = R.frame_norms(np.asarray(_stacked(LIVE_N, LIVE_H, TF) @ m, TF), LIVE_N)
    r = (nrm * (0.4 + 0.1 * k) * (1.0 + 0.5 * np.arange(len(nrm)) / len(nrm))).astype(TF)
    c = [sipx.set_definitions("bounds", "identity", 1600.0, 3900.0, ("tensor", "")),
         sipx.set_definitions("l21", "TV_xy", 0.0, r, ("slice", "z"))]
    P, A, prop = sipx.setup_constraints(c, g, TF)
    A, AtA, _, _ = sipx.PARSDMM_precompute_distribute(A, prop, g, opt)
    return (AtA, A, prop, P, g, opt), m, r


def _fresh(sipx, TF, k):
    (AtA, A, prop, P, g, opt), m, _ = _live_setup(sipx, TF, k)
    ctx = sipx.host.build_context(m, AtA, A, prop, P, g, opt)
    try:
        log, _ = ctx.parsdmm(opt)
        x, l, y = ctx.download()
    finally:
        ctx.close()
    return x, l, y, log


@pytest.mark.parametrize("TF", PRECISIONS, ids=["f32", "f64"])
def test_set_data_with_new_radii_then_reset_gives_the_bits_of_a_new_context(sipx, TF):
    args1, m1, r1 = _live_setup(sipx, TF, 1)
    _, m2, r2 = _live_setup(sipx, TF, 2)
    want1, want2 = _fresh(sipx, TF, 1), _fresh(sipx, TF, 2)
    assert not np.array_equal(want1[0], want2[0])
    AtA, A, prop, P, g, opt = args1
    assert [p.data_len(a) for p, a in zip(P, A)][:2] == [None, LIVE_N[2]]
    rho, gamma = _rho_gamma(opt, TF)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ctx = sipx.host.build_context(m1, AtA, A, prop, P, g, opt)
    try:
        log, _ = ctx.parsdmm(opt)
        _assert_same(ctx.download() + (log,), want1)
        before = ctx.device_bytes()["context"]
        with pytest.raises(sipx.SipxError, match="Radius of L1 ball is negative"):
            ctx.set_data(1, ub=np.where(np.arange(len(r2)) == 2, 0, r2).astype(TF))
        with pytest.raises(sipx.SipxError, match="only the annulus has inner radii"):
            ctx.set_data(1, lb=r2)
        ctx.set_data(1, ub=r2)
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
        S.set_data(1, ub=t(r2))
        x, log, l, y = S(t(m2))
        assert log.context_reused and S.ctx.io_bytes() == io
        _assert_same((x, l, y, log), want2)
    # a set built with a scalar holds no replaceable vectors
    c = [sipx.set_definitions("l21", "TV_xy", 0.0, float(r1.mean()), ("slice", "z"))]
    Ps, As, props = sipx.setup_constraints(c, g, TF)
    As, AtAs, _, _ = sipx.PARSDMM_precompute_distribute(As, props, g, opt)
    with sipx.Solver(AtAs, As, props, Ps, g, opt, TF) as S:
        with pytest.raises(sipx.SipxError, match=r"holds no replaceable vectors.*build a new Solver"):
            S.set_data(0, ub=r2)


def test_a_radius_from_device_memory_that_is_not_positive_zeroes_its_frame(sipx):
    """The host refuses such a vector; from device memory it cannot be looked at (csrc/seg_norm.h RADII): the frame's TV_xy range is set
    to zero -- the frame of x becomes constant, its mean -- and the other frames are projected as usual."""
    TF, n = np.float64, (10, 8, 5)
    g = _grid(sipx, n)
    opt = sipx.PARSDMM_options(FL=TF, maxit=2000, feas_tol=1e-10, obj_tol=1e-10, evol_rel_tol=1e-12)
    m = np.random.default_rng(17).standard_normal(int(np.prod(n)))
    A = _stacked(n, (1.0, 1.0, 1.0), TF)
    good = 0.5 * R.frame_norms(np.asarray(A @ m, TF), n)
    r = good.copy()
    bad = {1: 0.0, 3: float("nan")}
    for k, val in bad.items():
        r[k] = val
    P, Aop, prop = sipx.setup_constraints([sipx.set_definitions("l21", "TV_xy", 0.0, good, ("slice", "z"))], g, TF)
    Aop, AtA, _, _ = sipx.PARSDMM_precompute_distribute(Aop, prop, g, opt)
    with sipx.Solver(AtA, Aop, prop, P, g, opt, TF) as S:
        with pytest.raises(sipx.SipxError, match="Radius of L1 ball is negative"):
            S.set_data(0, ub=r)
    with sipx.Solver(AtA, Aop, prop, P, g, opt, TF) as S:
        S.set_data(0, ub=torch.from_numpy(r).cuda())
        x, log, _, _ = S(m.copy())
    X, M = x.reshape(n, order="F"), m.reshape(n, order="F")
    assert np.all(np.isfinite(x))
    for k in bad:
        assert np.abs(X[:, :, k] - M[:, :, k].mean()).max() <= 1e-6
    tv = R.frame_norms(np.asarray(A @ x, TF), n)
    for k in (0, 2, 4):
        assert abs(tv[k] - good[k]) <= 1e-6 * good[k]


# ---- 1b / 8. whole solves against the oracle (rules and tolerances of tests/test_gpu_l21.py, test_l21_solve_matches_oracle) ------------------
SOLVE_SETS = {"l1-TVxy": [("l1", "TV_xy", ("tensor", ""))],
              "l21-frames": [("l21", "TV_xy", ("slice", "z"))],
              "l21-frames+l1-Dz": [("l21", "TV_xy", ("slice", "z")), ("l1", "D_z", ("tensor", ""))]}
SOLVE_N, SOLVE_H = (16, 12, 8), (25.0, 25.0, 25.0)


def _solve_problem(mod, name, TF, m, opt_kw):
    """{bounds, the sets of SOLVE_SETS[name]} for module `mod`; radii: half the (frame's) norm of A m from the reference.  The oracle is
    given TV_xy as a custom operator -- its own D_y and D_x stacked -- with the l1 ball, whose projector is replaced by the reference for
    the l2,1 sets."""
    n, h = SOLVE_N, SOLVE_H
    g = mod.compgrid(h, n)
    opt = mod.PARSDMM_options(FL=TF, **opt_kw)
    c = [mod.set_definitions("bounds", "identity", 1600.0, 3900.0, ("tensor", ""))]
    swaps = []
    for st, opn, mode in SOLVE_SETS[name]:
        A = _stacked(n, h, TF) if opn == "TV_xy" else O.get_TD_operator(O.compgrid(h, n), opn, TF)[0]
        s = np.asarray(A @ m, TF)
        if st == "l21":
            r = (0.5 * R.frame_norms(s, n)).astype(TF)
            swaps.append((len(c), lambda x, r=r: _in_place(R.project, x, n, r)))
        else:
            r = TF(0.5 * np.abs(s.astype(np.float64)).sum())
        if mod is O:
            c.append(mod.set_definitions("l1", "identity" if opn == "TV_xy" else opn, 0.0, float(np.mean(r)), ("tensor", ""),
                                         (A, False) if opn == "TV_xy" else ((), False)))
        else:
            c.append(mod.set_definitions(st, opn, 0.0, r if np.ndim(r) else float(r), mode))
    P, A, prop = mod.setup_constraints(c, g, TF)
    if mod is O:
        for i, f in swaps:
            P[i] = f
    A, AtA, l, y = mod.PARSDMM_precompute_distribute(A, prop, g, opt)
    return g, opt, P, A, prop, AtA


@pytest.mark.parametrize("TF", PRECISIONS)
@pytest.mark.parametrize("name", list(SOLVE_SETS))
def test_solve_matches_oracle(sipx, TF, name):
    m = _model(SOLVE_N, TF, seed=1 + len(SOLVE_SETS[name]))
    kw = dict(maxit=60)
    go, oo, Po, Ao, propo, AtAo = _solve_problem(O, name, TF, m, kw)
    gs, os_, Ps, As, props, AtAs = _solve_problem(sipx, name, TF, m, kw)
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
    print(f"{name} {SOLVE_N} {np.dtype(TF).name}: iterations {len(ls.obj)} / {len(lo.obj)}, separation {sep}, rel diff {err:.3e}")
    if sep is not None or len(ls.obj) != len(lo.obj):
        # after a separation: the oracle again with the engine's rho / gamma history forced on it
        gr, orr, Pr, Ar, propr, AtAr = _solve_problem(O, name, TF, m, dict(kw, maxit=len(ls.obj)))
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


LOG_FIELDS = ("set_feasibility", "r_dual", "r_pri", "r_dual_total", "r_pri_total", "obj", "evol_x", "rho", "gamma", "cg_it", "cg_relres")


def test_device_form_gives_the_bits_of_the_host_form(sipx):
    TF = np.float32
    m = _model(SOLVE_N, TF, seed=3)
    g, opt, P, A, prop, AtA = _solve_problem(sipx, "l21-frames+l1-Dz", TF, m, dict(maxit=30))
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


# ---- 9. the engine's refusals through the C ABI -----------------------------------------------------------------------------------------------
def _desc(sipx, op, proj=14, mode=0, pmax=1.0, transform=0, dir=0, component=0):
    d = sipx.host._SetDesc()
    d.op, d.proj, d.pmin, d.pmax, d.mode, d.dir, d.transform, d.component = op, proj, 0.0, pmax, mode, dir, transform, component
    return d


def _refused(sipx, ctx, d):
    rc = sipx.lib().sipx_add_set(ctx.h, C.byref(d), None, None, 0)
    assert rc < 0, "the engine took the set"
    return sipx.lib().sipx_last_error().decode()


def test_engine_refusals(sipx):
    TF = np.float32
    XY, TV = sipx.host.OPS["TV_xy"], sipx.host.OPS["TV"]
    assert XY == 6
    L = sipx.lib()
    n = (16, 12, 8)
    g = _grid(sipx, n)
    ctx = sipx.Context(g, TF)
    try:
        # frames run along z; every existing refusal keeps its text
        for mode, dr in ((2, 0), (2, 1), (1, 0), (1, 1), (1, 2)):
            assert "frames run along z" in _refused(sipx, ctx, _desc(sipx, XY, mode=mode, dir=dr))
        assert "fiber / slice modes need an operator with one block" in _refused(sipx, ctx, _desc(sipx, TV, mode=2, dir=2))
        for proj in ("l1", "l2", "annulus", "cardinality"):
            assert "fiber / slice modes need an operator with one block" in _refused(sipx, ctx, _desc(sipx, XY, sipx.host.PROJ[proj], mode=2, dir=2))
        for op in ("identity", "D_x", "D_z"):
            assert "the l2,1 ball acts on the range of the TV operator: TD_OP must be TV" in _refused(sipx, ctx, _desc(sipx, sipx.host.OPS[op], mode=2, dir=2))
        assert "this projector needs an operator with one block" in _refused(sipx, ctx, _desc(sipx, XY, sipx.host.PROJ["rank"]))
        for r in (0.0, -2.0, float("nan")):
            assert _refused(sipx, ctx, _desc(sipx, XY, pmax=r)) == "Radius of L1 ball is negative"
            assert _refused(sipx, ctx, _desc(sipx, XY, pmax=r, mode=2, dir=2)) == "Radius of L1 ball is negative"
        ub = np.ones(n[2], TF)
        ub[5] = 0
        d = _desc(sipx, XY, mode=2, dir=2)
        d.ub = ub.ctypes.data
        assert "Radius of L1 ball is negative" in _refused(sipx, ctx, d)
        assert "the TV_xy operator takes no Minkowski component" in _refused(sipx, ctx, _desc(sipx, XY, sipx.host.PROJ["l1"], component=1))
        assert "sets behind the DCT act in their own domain" in _refused(sipx, ctx, _desc(sipx, XY, transform=1))
        # sets the engine takes: scalar (no replaceable vectors) and vector radii; sipx_project refuses any other length
        assert L.sipx_add_set(ctx.h, C.byref(_desc(sipx, XY, mode=2, dir=2)), None, None, 0) == 0
        ub[5] = 1
        assert L.sipx_add_set(ctx.h, C.byref(d), None, None, 0) == 1
        assert L.sipx_add_set(ctx.h, C.byref(_desc(sipx, XY)), None, None, 0) == 2
        assert L.sipx_set_data(ctx.h, 0, None, ub.ctypes.data_as(C.c_void_p)) != 0
        assert "holds no replaceable vectors" in L.sipx_last_error().decode()
        assert L.sipx_set_data(ctx.h, 1, None, ub.ctypes.data_as(C.c_void_p)) == 0
        ub[0] = -1
        assert L.sipx_set_data(ctx.h, 1, None, ub.ctypes.data_as(C.c_void_p)) != 0
        assert "Radius of L1 ball is negative" in L.sipx_last_error().decode()
        v = np.zeros(int(np.prod(n)), TF)
        for dd in (_desc(sipx, XY, mode=2, dir=2), _desc(sipx, XY)):
            assert L.sipx_project(ctx.h, C.byref(dd), v.ctypes.data_as(C.c_void_p), C.c_int64(len(v))) != 0
            assert f"TV_xy range: {R.rows(n)} entries on this grid, {len(v)} given" in L.sipx_last_error().decode()
        ns = C.c_int64()
        assert L.sipx_l21_norms(ctx.h, XY, 2, 2, None, None, C.byref(ns)) == 0 and ns.value == n[2]
        assert L.sipx_l21_norms(ctx.h, XY, 0, 0, None, None, C.byref(ns)) == 0 and ns.value == 1
        assert L.sipx_l21_norms(ctx.h, XY, 2, 1, None, None, C.byref(ns)) != 0 and "frames run along z" in L.sipx_last_error().decode()
        assert L.sipx_l21_norms(ctx.h, TV, 2, 2, None, None, C.byref(ns)) != 0
        assert "fiber / slice modes need an operator with one block" in L.sipx_last_error().decode()
        assert L.sipx_l21_norms(ctx.h, 1, 0, 0, None, None, C.byref(ns)) != 0 and "TD_OP must be TV" in L.sipx_last_error().decode()
    finally:
        ctx.close()
    # a 2-D grid: TV is in-plane already
    ctx = sipx.Context(_grid(sipx, (16, 12)), TF)
    try:
        for d in (_desc(sipx, XY), _desc(sipx, XY, sipx.host.PROJ["l1"])):
            msg = _refused(sipx, ctx, d)
            assert "provided an unknown transform domain operator" in msg and "TV_xy" in msg
    finally:
        ctx.close()
    # a context with a slab decomposition or set ownership: at sipx_add_set, or at sipx_finalize when it came later -- the operator
    # itself, with any set
    msg = "the TV_xy operator takes single-process contexts only"
    for proj, kw in (("l21", dict(mode=2, dir=2)), ("l21", {}), ("l1", {}), ("bounds", {})):
        ctx = sipx.Context(g, TF)
        try:
            ctx.set_decomp("slab")
            assert msg in _refused(sipx, ctx, _desc(sipx, XY, sipx.host.PROJ[proj], **kw))
        finally:
            ctx.close()
        for late in ("slab", "owned"):
            ctx = sipx.Context(g, TF)
            try:
                assert L.sipx_add_set(ctx.h, C.byref(_desc(sipx, XY, sipx.host.PROJ[proj], **kw)), None, None, 0) == 0
                if late == "slab":
                    ctx.set_decomp("slab")
                else:
                    ctx.set_owned([1, 1])
                with pytest.raises(sipx.SipxError, match=msg):
                    ctx.finalize(np.ones(int(np.prod(n)), TF), [10.0], 1.0)
            finally:
                ctx.close()
