"""Device memory of a context (csrc/device_memory.h): an error return frees its buffers, a context gives back what it took, and
sipx_reset still zero-fills every array that carries state from one solve to the next."""
import ctypes as C
import time

import numpy as np
import pytest

from tests import matrix_free_ops as MF
from tests.test_gpu_parity import _minkowski_problem, _problem, model
from tests.test_gpu_round5 import _same_logs

pytestmark = pytest.mark.gpu

H3 = (25.0, 25.0, 25.0)
KW = dict(evol_rel_tol=0.0, feas_tol=0.0, obj_tol=0.0)


def _vectors_mfree_rank(sipx, TF, m, kw):
    """per-element bounds vectors, a caller-supplied CSC operator handed over without A'A (a matrix-free term of Q) and a
    slice-rank set"""
    n = (32, 32, 16)
    A = MF.ragged(n).astype(TF)
    lo = np.linspace(1600.0, 2200.0, m.size).astype(TF)
    c = [sipx.set_definitions("bounds", "identity", lo, (lo + 1500).astype(TF), ("matrix", "")),
         MF.custom_set(sipx, "l2", A, 0.0, float(0.7 * np.linalg.norm((A @ m).astype(np.float64)))),
         sipx.set_definitions("rank", "identity", 0, 6, ("slice", "z"))]
    g, opt, P, TD, prop, AtA = MF.setup(sipx, TF, n, H3, c, kw)
    assert AtA[1] is None and len(prop.AtA_offsets[1]) == 0
    return g, opt, P, TD, prop, AtA


# name -> (grid, precision, maker(sipx, m, opt_kw) -> g, opt, P, TD_OP, prop, AtA)
LISTS = {
    "l1-pair-f32": ((48, 40, 32), np.float32, lambda sipx, m, kw: _problem(sipx, (48, 40, 32), H3, np.float32, ["bounds", "l1:D_x", "l1:D_z"], m, kw)),
    "l1-pair-f64": ((48, 40, 32), np.float64, lambda sipx, m, kw: _problem(sipx, (48, 40, 32), H3, np.float64, ["bounds", "l1:D_x", "l1:D_z"], m, kw)),
    "vectors-mfree-rank": ((32, 32, 16), np.float32, lambda sipx, m, kw: _vectors_mfree_rank(sipx, np.float32, m, kw)),
    "minkowski": ((32, 24), np.float32, None),
}


def _make(sipx, name, m, maxit):
    n, TF, maker = LISTS[name]
    if name == "minkowski":
        g, opt, P, TD, prop, AtA = _minkowski_problem(sipx, n, (25.0, 6.0), TF, m, maxit=maxit)
        opt.evol_rel_tol = opt.feas_tol = opt.obj_tol = 0.0
        return g, opt, P, TD, prop, AtA
    return maker(sipx, m, dict(KW, maxit=maxit))


def _rho_gamma(opt, TF):
    TFt = np.dtype(TF).type
    return [float(TFt(r)) for r in opt.rho_ini], float(TFt(opt.gamma_ini))


@pytest.fixture()
def probe(sipx):
    """-> device_used(): the runtime's figure for the card, read through a context that holds nothing itself; skips the test when
    another process moves it"""
    ctx = sipx.host.Context(sipx.compgrid((1.0, 1.0), (8, 8)), np.float32)

    def device_used():
        return ctx.device_bytes()["device_used"]
    a = device_used()
    time.sleep(0.2)
    b = device_used()
    if a != b:
        ctx.close()
        pytest.skip(f"device_used moves without this test doing anything ({a} -> {b}): another process is using the card")
    yield device_used
    ctx.close()


def test_error_returns_of_project_free_their_buffers(sipx, probe):
    """sipx_project allocates its buffers and then validates the descriptor: a refused descriptor must not leave them behind.
    40 refused calls on one un-finalised context; device_used may grow by one call's two vectors at the most."""
    TF, n = np.float32, 1 << 20
    host = sipx.host
    g = sipx.compgrid((1.0, 1.0), (n, 1))
    v = np.ones(n, TF)
    ball = host.Projector(sipx.set_definitions("l1", "identity", 0.0, -1.0, ("matrix", "")), g, TF).desc("identity", False)
    bounds = host.Projector(sipx.set_definitions("bounds", "identity", np.zeros(n, TF), np.ones(n, TF), ("matrix", "")), g, TF)
    no_lb = bounds.desc("identity", False)
    no_lb.lb = None
    ctx = host.Context(g, TF)
    try:
        before = probe()
        for k in range(40):
            d, why = (ball, "Radius of L1 ball is negative") if k % 2 == 0 else (no_lb, "per-element bounds need lb and ub")
            assert host.lib().sipx_project(ctx.h, C.byref(d), v.ctypes.data_as(C.c_void_p), C.c_int64(n)) != 0
            assert why in host.lib().sipx_last_error().decode()
        after = probe()
        grown = after - before
        print(f"\n[device memory] 40 refused sipx_project calls: device_used grew by {grown} bytes ({grown / (2 * n * 4):.2f} x one call's two vectors)")
        assert grown <= 2 * n * 4, grown
        assert ctx.device_bytes()["context"] == 0
    finally:
        ctx.close()


@pytest.mark.parametrize("name", list(LISTS))
def test_a_context_gives_back_what_it_took(sipx, probe, name):
    """build, three steps, sipx_reset, three steps, close -- seven times; after the seventh close device_used may exceed its value
    after the first one (the warm-up: libraries load their kernels and keep their pools) by one N-vector at the most."""
    n, TF, _ = LISTS[name]
    m = model(n, TF, seed=3)
    g, opt, P, TD, prop, AtA = _make(sipx, name, m, 20)
    rho, gamma = _rho_gamma(opt, TF)
    used = []
    for cycle in range(7):
        ctx = sipx.host.build_context(m, AtA, TD, prop, P, g, opt)
        try:
            if cycle == 0:
                print(f"\n[device memory] {name}: context bytes after sipx_finalize {ctx.device_bytes()['context']}")
            ctx.parsdmm_begin(opt)
            ctx.parsdmm_steps(3)
            ctx.reset(m, rho, gamma)
            ctx.parsdmm_begin(opt)
            ctx.parsdmm_steps(3)
        finally:
            ctx.close()
        used.append(probe())
    print(f"[device memory] {name}: device_used after each close, less the first: {[u - used[0] for u in used]}")
    assert used[6] - used[0] <= m.size * np.dtype(TF).itemsize, used


@pytest.mark.parametrize("name", ["l1-pair-f32", "vectors-mfree-rank"])
def test_reset_zeroes_what_a_solve_left_behind(sipx, name):
    """12 iterations on a new context == 12 iterations on a context that ran 7 iterations on another model and was reset: the
    same bits of x and of every y_i, l_i (and of the logs)."""
    n, TF, _ = LISTS[name]
    m1, m2 = model(n, TF, seed=11), model(n, TF, seed=12)
    m2 = (m2 * TF(0.97) + TF(40.0)).astype(TF)
    g, opt, P, TD, prop, AtA = _make(sipx, name, m1, 12)
    rho, gamma = _rho_gamma(opt, TF)
    ctx = sipx.host.build_context(m2, AtA, TD, prop, P, g, opt)
    try:
        log2, _ = ctx.parsdmm(opt)
        x2, l2, y2 = ctx.download()
    finally:
        ctx.close()
    ctx = sipx.host.build_context(m1, AtA, TD, prop, P, g, opt)
    try:
        ctx.parsdmm_begin(opt)
        ctx.parsdmm_steps(7)
        ctx.reset(m2, rho, gamma)
        log, _ = ctx.parsdmm(opt)
        xr, lr, yr = ctx.download()
    finally:
        ctx.close()
    assert len(log2.obj) == 12
    assert np.array_equal(xr, x2)
    for a, b in zip(lr + yr, l2 + y2):
        assert np.array_equal(a, b)
    _same_logs(log, log2)
