"""Matrix-free terms of Q: caller-supplied sparse operators passed without their A'A (SIPX_OP_CSC, ata_R = NULL), whose
products go through csrc/kernels_sparse.hip instead of CDS bands.  The oracle handles any sparse operator through mat2CDS,
however many diagonals, and is the reference of the solves; the products are checked against a float64 evaluation.

Operators (tests/matrix_free_ops.py): `ragged` (23 x 17 grid, 300 rows: empty rows, an empty column, rows on both sides of
every lane-group size, 777 diagonals in A'A), `tall` (M > N), `blur` (the reference's deblurring example on 64 x 40: the taps
0 and 2 .. 25 as the example builds them, which gives 51 diagonals, 312 empty rows), `dxz` (nine diagonals: both routes
exist), `ragged` on two 3-D grids next to TV's seven bands, and `rowsL` (every row L long: one operator per lane-group size)."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import parsdmm_oracle as O
from tests import matrix_free_ops as MF

pytestmark = pytest.mark.gpu

BIG = 1.0e9
LOG_FIELDS = ("obj", "evol_x", "r_pri", "r_dual", "rho", "gamma", "cg_it", "cg_relres", "set_feasibility")


def _operator(name, TF):
    """-> (grid, spacing, A)"""
    if name == "ragged":
        return (23, 17), (1.0, 1.0), MF.ragged((23, 17))
    if name == "tall":
        return (23, 17), (1.0, 1.0), MF.tall((23, 17))
    if name == "blur":
        return (64, 40), (1.0, 1.0), MF.blur()
    if name == "dxz":
        return (30, 22), (25.0, 6.0), MF.dxz((30, 22), (25.0, 6.0), TF)
    if name == "ragged975":
        return (9, 7, 5), (1.0, 2.0, 4.0), MF.ragged((9, 7, 5))
    if name == "ragged16128":
        return (16, 12, 8), (1.0, 2.0, 4.0), MF.ragged((16, 12, 8))
    if name.startswith("rows"):
        return (23, 17), (1.0, 1.0), MF.uniform_rows((23, 17), int(name[4:]))
    raise KeyError(name)


def _same_logs(a, b):
    for f in LOG_FIELDS:
        assert np.array_equal(np.asarray(getattr(a, f)), np.asarray(getattr(b, f)), equal_nan=True), f


def _same_state(a, b):
    assert np.array_equal(a[0], b[0])
    for u, v in zip(a[1], b[1]):
        assert np.array_equal(u, v)
    for u, v in zip(a[2], b[2]):
        assert np.array_equal(u, v)


# ---- 1. the product -----------------------------------------------------------------------------------------------------------------
OPERATORS = ["ragged", "tall", "blur", "dxz", "ragged975", "ragged16128"] + ["rows%d" % L for L in (1, 2, 3, 6, 12, 24, 48, 100)]


@pytest.mark.parametrize("TF", [np.float32, np.float64])
@pytest.mark.parametrize("name", OPERATORS)
def test_product_with_a_matrix_free_term(sipx, TF, name):
    """apply_Q(x) against sum_i rho_i A_i'A_i x evaluated in float64 from the TF-rounded entries and TF rho.  Element-wise
    bound c eps(TF) (sum_i rho_i |A_i|'|A_i| |x|), c = longest row + longest column + bands of the CDS part + 8: the
    gamma-bound of the two nested sums (any summation order) plus the scalings by rho and the accumulation over the terms."""
    n, h, A = _operator(name, TF)
    A = sp.csc_matrix(A, dtype=TF)
    three_d = len(n) == 3
    m = MF.model(n, TF)
    c = [sipx.set_definitions("l1", "TV", 0.0, BIG, ("matrix", ""))] if three_d else [sipx.set_definitions("bounds", "identity", -BIG, BIG, ("matrix", ""))]
    c.append(MF.custom_set(sipx, "bounds", A, -BIG, BIG))
    rho = [1.5, 0.7, 2.25]
    g, opt, P, ops, prop, AtA = MF.setup(sipx, TF, n, h, c, dict(rho_ini=rho), banded={1: False})
    assert AtA[1] is None and len(prop.AtA_offsets[1]) == 0
    ctx = sipx.host.build_context(m, AtA, ops, prop, P, g, opt)
    try:
        bands, free = ctx.q_terms()
        assert free == 1 and bands == (7 if three_d else 1)
        first = O.get_TD_operator(O.compgrid(h, n), "TV" if three_d else "identity", TF)[0]
        mats = [sp.csc_matrix(M, dtype=TF).astype(np.float64) for M in (first, A, sp.identity(m.size, format="csc"))]
        absm = [abs(M) for M in mats]
        x = np.random.default_rng(3).standard_normal(m.size).astype(TF)
        x64 = x.astype(np.float64)
        Acsr = A.tocsr()
        cst = int(np.diff(Acsr.indptr).max()) + int(np.diff(A.indptr).max()) + bands + 8
        eps = float(np.finfo(TF).eps)

        def check(r):
            r64 = [float(TF(v)) for v in r]
            want = sum(ri * (M.T @ (M @ x64)) for ri, M in zip(r64, mats))
            scale = sum(ri * (M.T @ (M @ np.abs(x64))) for ri, M in zip(r64, absm))
            got = ctx.apply_Q(x).astype(np.float64)
            bad = np.abs(got - want) > cst * eps * scale
            assert not bad.any(), (name, int(bad.sum()), float((np.abs(got - want) / np.maximum(cst * eps * scale, 1e-300)).max()))
        check(rho)
        new = [0.4, 3.5, 2.25]                     # the matrix-free term and a banded one change, the distance term keeps its rho
        ctx.q_update(new, rho)
        check(new)                                 # (a stale rho of the matrix-free term shows here)
        assert ctx.q_terms() == (bands, 1)
        Q, off = ctx.get_Q()                       # the banded part only
        assert Q.shape == (m.size, bands)
    finally:
        ctx.close()


# ---- 2. the two routes of an operator whose A'A is banded ---------------------------------------------------------------------------
def _dxz_problem(mod, TF, banded=None):
    n, h = (30, 22), (25.0, 6.0)
    m = MF.model(n, TF, seed=6)
    A = MF.dxz(n, h, TF)
    s = A @ m
    c = [mod.set_definitions("bounds", "identity", 1600.0, 3900.0, ("matrix", "")),
         MF.custom_set(mod, "l1", A, 0.0, float(0.4 * np.abs(s).sum()))]
    return (m,) + MF.setup(mod, TF, n, h, c, dict(maxit=40), banded=banded)


@pytest.mark.parametrize("TF", [np.float32, np.float64])
def test_routes_of_a_banded_operator_agree(sipx, TF):
    tol = 1e-3 if TF == np.float32 else 1e-5
    m, go, oo, Po, Ao, propo, AtAo = _dxz_problem(O, TF)
    xo = O.PARSDMM(m.copy(), AtAo, Ao, propo, Po, go, oo)[0].astype(np.float64)
    xs = {}
    for route, banded in (("cds", None), ("free", {1: False})):
        m, g, opt, P, A, prop, AtA = _dxz_problem(sipx, TF, banded)
        ctx = sipx.host.build_context(m, AtA, A, prop, P, g, opt)
        try:
            if route == "cds":
                assert len(prop.AtA_offsets[1]) == 9 and AtA[1].shape == (m.size, 9) and ctx.q_terms() == (9, 0)
            else:
                assert len(prop.AtA_offsets[1]) == 0 and AtA[1] is None and ctx.q_terms() == (1, 1)
            ctx.parsdmm(opt)
            xs[route] = ctx.download()[0].astype(np.float64)
        finally:
            ctx.close()
    nrm = np.linalg.norm(xo)
    d = {k: float(np.linalg.norm(v - xo) / nrm) for k, v in xs.items()}
    d["routes"] = float(np.linalg.norm(xs["cds"] - xs["free"]) / nrm)
    print("dxz", np.dtype(TF).name, d)
    assert max(d.values()) < tol, d


# ---- 3. solves against the oracle ------------------------------------------------------------------------------------------------
def _sipx_problem(sipx, name, TF):
    if name == "ragged":
        n, h, m, c, kw = MF.ragged_problem(sipx, TF)
    elif name == "ragged3d":
        n, h, m, c, kw = MF.ragged_problem(sipx, TF, n=(16, 12, 8), h=(1.0, 1.0, 1.0))
    elif name == "blur":
        n, h, m, c, kw = MF.blur_problem(sipx, TF)
    else:
        n, h, m, c, kw = MF.blur_problem(sipx, TF, feasibility_only=True)
    return (m,) + MF.setup(sipx, TF, n, h, c, kw)


@pytest.mark.parametrize("TF", [np.float32, np.float64])
@pytest.mark.parametrize("name", ["ragged", "blur", "ragged3d"])
def test_solve_matches_oracle(sipx, TF, name):
    """||x - x_oracle|| / ||x_oracle|| below 1e-3 (Float32) / 1e-5 (Float64), the oracle in the same precision: the bounds the
    suite holds for a route whose sums are ordered differently from the oracle's (test_gpu_parity.py, the host-mirror A'A)."""
    xo, lo = MF.oracle_solve(name, np.dtype(TF).name)
    m, g, opt, P, A, prop, AtA = _sipx_problem(sipx, name, TF)
    assert AtA[2] is None and len(prop.AtA_offsets[2]) == 0        # more diagonals than Q keeps bands: matrix-free by itself
    x, log, l, y = sipx.PARSDMM(m.copy(), AtA, A, prop, P, g, opt)
    err = float(np.linalg.norm(x.astype(np.float64) - xo) / np.linalg.norm(xo))
    print(name, np.dtype(TF).name, "iterations", len(log.obj), "oracle", len(lo.obj), "distance", err)
    assert err < (1e-3 if TF == np.float32 else 1e-5), err
    assert (np.asarray(log.set_feasibility)[-1] <= opt.feas_tol).all(), log.set_feasibility[-1]
    assert [len(v) for v in y] == [a.shape[0] for a in A]


# ---- 4. the example's shape --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("TF", [np.float32, np.float64])
def test_deblurring_example_feasibility_only(sipx, TF):
    m, g, opt, P, A, prop, AtA = _sipx_problem(sipx, "blur_feas", TF)
    assert opt.feasibility_only and opt.zero_ini_guess and len(A) == 3
    ctx = sipx.host.build_context(m, AtA, A, prop, P, g, opt)
    try:
        assert ctx.q_terms()[1] == 1
        log, input_was_feasible = ctx.parsdmm(opt)      # (the flag of the feasible-input exit, PARSDMM.jl:63-82: not taken here)
        x = ctx.download()[0]
    finally:
        ctx.close()
    # it runs and stops on feasibility (stop_PARSDMM.jl:23): before maxit, every set within feas_tol at the last check
    assert not input_was_feasible and 6 < len(log.obj) < opt.maxit
    assert (np.asarray(log.set_feasibility)[-1] <= opt.feas_tol).all(), log.set_feasibility[-1]
    B = MF.blur().astype(TF)
    d = (B @ MF.model((64, 40), TF, seed=1)).astype(TF).astype(np.float64)
    s = B.astype(np.float64) @ x.astype(np.float64)
    assert (np.abs(s - d) <= 15.0 * (1 + 1e-3)).all(), float(np.abs(s - d).max())


# ---- 5. state ----------------------------------------------------------------------------------------------------------------------
def test_state_is_reproducible(sipx):
    import torch
    TF = np.float32
    m, g, opt, P, A, prop, AtA = _sipx_problem(sipx, "ragged", TF)
    args = (AtA, A, prop, P, g, opt)
    x1, log1, l1, y1 = sipx.PARSDMM(m.copy(), *args)
    x2, log2, l2, y2 = sipx.PARSDMM(m.copy(), *args)                 # (custom operators are never cached: a fresh context)
    _same_state((x1, l1, y1), (x2, l2, y2))
    _same_logs(log1, log2)
    # sipx_reset + solve == a new context; the stepwise driver == the whole solve
    rho_ini = [float(TF(r)) for r in opt.rho_ini]
    ctx = sipx.host.build_context(m, *args)
    try:
        ctx.parsdmm(opt)
        ctx.reset(m, rho_ini, float(TF(opt.gamma_ini)))
        log3, _ = ctx.parsdmm(opt)
        _same_state((x1, l1, y1), ctx.download())
        _same_logs(log1, log3)
        ctx.reset(m, rho_ini, float(TF(opt.gamma_ini)))
        ctx.parsdmm_begin(opt)
        done, steps = False, 0
        while not done:
            done = ctx.parsdmm_steps(3 if steps % 2 else 1)
            steps += 1
            assert steps < 400
        _same_state((x1, l1, y1), ctx.download())
        _same_logs(log1, ctx.parsdmm_log())
    finally:
        ctx.close()
    # device-resident call
    xd, logd, ld, yd = sipx.PARSDMM_device(torch.from_numpy(m.copy()).cuda(), *args)
    _same_state((x1, l1, y1), (xd.cpu().numpy(), [v.cpu().numpy() for v in ld], [v.cpu().numpy() for v in yd]))
    _same_logs(log1, logd)


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------
def _small(sipx, TF=np.float32, **opt):
    n, h = (23, 17), (1.0, 1.0)
    m = MF.model(n, TF)
    A = MF.ragged(n).astype(TF)
    c = [sipx.set_definitions("bounds", "identity", 1600.0, 3900.0, ("matrix", "")), MF.custom_set(sipx, "bounds", A, -BIG, BIG)]
    return (m,) + MF.setup(sipx, TF, n, h, c, opt)


def test_refused_with_stencil_q(sipx):
    m, g, opt, P, A, prop, AtA = _small(sipx)
    opt.Q_mode = "stencil"
    with pytest.raises(sipx.SipxError, match=r"custom sparse operator.*stencil"):
        sipx.host.build_context(m, AtA, A, prop, P, g, opt)


def test_refused_with_a_communicator(sipx):
    import torch

    class OneRank:           # what TorchComm asks of torch.distributed; the refusal comes before any collective is called
        @staticmethod
        def get_world_size():
            return 1

        @staticmethod
        def get_rank():
            return 0

        @staticmethod
        def get_backend():
            return "gloo"
    from sipx import sharded
    m, g, opt, P, A, prop, AtA = _small(sipx)
    keep = []
    with pytest.raises(sipx.SipxError, match=r"custom sparse operator.*sharded"):
        sipx.host.build_context(m, AtA, A, prop, P, g, opt,
                                attach=lambda ctx: keep.append(sharded.attach_comm(ctx, OneRank, torch.device("cuda", 0), mode="torch")))


def test_refused_with_a_minkowski_component(sipx):
    m, g, opt, P, A, prop, AtA = _small(sipx)
    A[1].component = 1
    try:
        with pytest.raises(sipx.SipxError, match=r"custom sparse operator.*Minkowski"):
            sipx.host.build_context(m, AtA, A, prop, P, g, opt)
    finally:
        del A[1].component


def test_refused_beyond_32_bit_indices(sipx):
    """A unit-sized fake: one stored entry in a matrix that claims 2^31 rows.  Refused when the set is added; nothing of that
    size is ever allocated."""
    TF = np.float32
    n = (4, 3)
    g = sipx.compgrid((1.0, 1.0), n)
    A = sp.csc_matrix((np.ones(1, TF), (np.zeros(1, np.int64), np.zeros(1, np.int64))), shape=(2 ** 31, 12))
    op = sipx.host.CustomOperator(A, g, TF)
    proj = sipx.host.Projector(sipx.set_definitions("bounds", "identity", -1.0, 1.0, ("matrix", "")), g, TF)
    ctx = sipx.Context(g, TF)
    try:
        with pytest.raises(sipx.SipxError, match=r"32-bit indices.*2\^31"):
            ctx.add_set(op, proj)
        B = sp.csc_matrix((np.ones(1, TF), (np.zeros(1, np.int64), np.zeros(1, np.int64))), shape=(2 ** 31 - 1, 12))
        assert ctx.add_set(sipx.host.CustomOperator(B, g, TF), proj) == 0      # the largest row count the indices hold (never finalized)
    finally:
        ctx.close()
