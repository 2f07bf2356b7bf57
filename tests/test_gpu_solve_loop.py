"""The native whole-solve loop (sipx_parsdmm: software pipeline, right-hand side queued ahead, sums by event or pinned word)
against the same loop kept on the host over the phase entry points (sharded.PhaseDriver), on one rank: the same context
type, the same inputs, bit for bit.  The problem is chosen so that every rho rule acts -- the clamp at once (rho_ini lies
outside it), Barzilai-Borwein steps, a feasibility doubling -- and so that rho also stays put on some iterations, where the
native loop queues the next right-hand side ahead."""
import numpy as np
import pytest

from oracle import parsdmm_oracle as O      # checker only
from tests.test_gpu_parity import _problem, model

pytestmark = pytest.mark.gpu

LOG_FIELDS = ("obj", "evol_x", "r_pri", "r_dual", "r_pri_total", "r_dual_total", "rho", "gamma", "cg_it", "cg_relres", "set_feasibility")


@pytest.mark.parametrize("stride", [None, "7"])        # 7: section marks on a sample of the iterations, the sums by pinned word
@pytest.mark.parametrize("TF", [np.float32, np.float64])
def test_native_loop_equals_phase_driver(sipx, monkeypatch, TF, stride):
    from sipx import sharded
    if stride is None:
        monkeypatch.delenv("SIPX_MARK_STRIDE", raising=False)
    else:
        monkeypatch.setenv("SIPX_MARK_STRIDE", stride)
    n, h, maxit = (16, 12, 8), (25.0, 20.0, 10.0), 45
    m = model(n, TF, seed=3)
    g, o, P, A, prop, AtA = _problem(sipx, n, h, TF, ["bounds", "l1:D_z"], m,
                                     dict(maxit=maxit, rho_ini=[1e5], rho_update_frequency=2, adjust_feasibility_rho=True,
                                          evol_rel_tol=0.0, feas_tol=0.0, obj_tol=0.0))
    # the loop on the host
    ctx = sipx.host.build_context(m, AtA, A, prop, P, g, o)
    try:
        drv = sharded.PhaseDriver(ctx, o, any(prop.ncvx[:len(P)]))
        doublings = []                                 # (iteration, rho of the least feasible set: as the Barzilai-Borwein rule left it, as logged)
        while not drv.step():
            i = drv.i
            if i in (20, 30, 40) and drv.adjust_feas_rho:          # (the switches as the rho rules of iteration i saw them)
                # the Barzilai-Borwein rule alone, once more, from the sums of iteration i that the context still holds
                rho_bb = drv.log.rho[i - 1].copy()
                if (drv.adjust_rho or drv.adjust_gamma) and i % 2 == 0:
                    rho_bb, _ = ctx.adapt_rho_gamma(drv.adjust_rho, drv.adjust_gamma, drv.log.rho[i - 1], drv.log.gamma[i - 1])
                k = O._julia_argmax(drv.log.set_feasibility[drv.counter - 2])
                doublings.append((i, float(TF(rho_bb[k])), float(drv.rho[k])))
        log_p = drv.result_log()
        x_p, l_p, y_p = ctx.download()
    finally:
        ctx.close()
    # its record shows every rule at work (row k of log.rho: the rho of iteration k + 1, i.e. what the rules of iteration k left)
    rho = np.asarray(log_p.rho)
    assert len(rho) == maxit
    assert (rho[0] == 1e5).all() and (rho[1] == 1e4).all()                                    # the clamp acted after iteration 1
    changed = [bool((rho[k] != rho[k - 1]).any()) for k in range(1, maxit)]                   # changed[k - 1]: by the rules of iteration k
    assert any(changed[k - 1] for k in range(2, maxit) if k % 2 == 0 and k % 10)              # a Barzilai-Borwein change, no doubling beside it
    assert any(after == 2 * bb and after < 1e4 for _, bb, after in doublings), doublings         # a feasibility doubling, not clamped away
    assert any(not c for c in changed[1:])                                                    # rho unchanged: the right-hand side was queued ahead
    # the native loop
    ctx = sipx.host.build_context(m, AtA, A, prop, P, g, o)
    try:
        log_n, feasible = ctx.parsdmm(o)
        x_n, l_n, y_n = ctx.download()
    finally:
        ctx.close()
    assert not feasible and not drv.stopped_feasible
    for f in LOG_FIELDS:
        a, b = np.asarray(getattr(log_n, f)), np.asarray(getattr(log_p, f))
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), f
    assert np.array_equal(x_n, x_p)
    assert len(y_n) == len(y_p) == len(l_n) == len(l_p) == 3
    for k in range(3):
        assert np.array_equal(y_n[k], y_p[k]) and np.array_equal(l_n[k], l_p[k]), k
