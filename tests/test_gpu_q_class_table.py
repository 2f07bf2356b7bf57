"""The class table of Q: the z-marching products take the coefficients of the 7-band matrix from 4 x 27 values (one per stored
band and boundary class of a row) instead of the four stored bands, and a planned Q update touches the table only.  The
products, the solve and Q read back must keep every bit of the band path (SIPX_Q_TABLE=0) and of the oracle."""
import numpy as np
import pytest

from oracle import parsdmm_oracle as O      # checker only
from tests import march_geometry as MG
from tests.test_gpu_parity import _problem, model

pytestmark = pytest.mark.gpu

LOG_FIELDS = ("obj", "cg_it", "rho", "gamma", "r_pri", "r_dual", "set_feasibility")


def _q_table(ctx):
    return ctx.kernel_stats_all(-1)["q_table"]


def _same_log(la, lb):
    for k in LOG_FIELDS:
        a, b = np.asarray(getattr(la, k)), np.asarray(getattr(lb, k))
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), k


@pytest.mark.parametrize("TF", [np.float32, np.float64])
@pytest.mark.parametrize("n,kinds", [((40, 24, 20), ["bounds", "l1:D_x", "l1:D_y", "l1:D_z"]),      # band order 0, -1, +1, -n1, +n1, -n1n2, +n1n2
                                     ((36, 20, 9), ["bounds", "l1:TV"]),                              # band order 0, -n1n2, -n1, -1, +1, +n1, +n1n2
                                     ((264, 10, 7), ["bounds", "l1:D_x", "l1:D_y", "l1:D_z"]),       # two tiles along x (Float32), ragged rows
                                     ((40, 24, 3), ["bounds", "l1:D_x", "l1:D_y", "l1:D_z"])])       # fewer planes than a chunk
def test_table_products_keep_the_bits_of_the_bands(sipx, monkeypatch, TF, n, kinds):
    """apply_Q before and after q_update, Q read back after several rho changes, and a 30-iteration solve: the same bits with
    the table on and off (on small grids in chunks of 4 planes, so that chunk and tile edges run), and apply_Q on the table
    equals the oracle's Ax_CDS."""
    h = (25.0, 20.0, 10.0)
    m = model(n, TF, seed=4)
    go, oo, Po, Ao, propo, AtAo = _problem(O, n, h, TF, kinds, m)
    p = len(Ao)
    rho = list(np.linspace(0.5, 11.0, p))
    x = np.random.default_rng(9).standard_normal(m.size).astype(TF)
    Qo, offo = O.assemble_Q(AtAo, propo.AtA_offsets, np.array(rho, TF), TF)
    want = O.Ax_CDS(x, Qo, offo)
    monkeypatch.setenv("SIPX_CDS_MARCH", "2")
    monkeypatch.setenv("SIPX_CDS_MARCH_ZCHUNK", "4")
    out = {}
    for tab in ("1", "0"):
        monkeypatch.setenv("SIPX_Q_TABLE", tab)
        gs, os_, Ps, As, props, AtAs = _problem(sipx, n, h, TF, kinds, m, dict(maxit=30))
        os_.rho_ini = rho
        ctx = sipx.host.build_context(m, AtAs, As, props, Ps, gs, os_)
        try:
            state = _q_table(ctx)
            before = MG.routes(ctx)
            y0 = ctx.apply_Q(x)
            rho2 = [r * (1.5 if i % 2 else 0.75) for i, r in enumerate(rho)]
            ctx.q_update(rho2, rho)
            y1 = ctx.apply_Q(x)
            rho3 = list(rho2); rho3[0] = 0.0625; rho3[-1] = 17.5
            ctx.q_update(rho3, rho2)
            rho4 = [r * 1.25 for r in rho3]
            ctx.q_update(rho4, rho3)
            Q4, _ = ctx.get_Q()
            y4 = ctx.apply_Q(x)
            took_q = MG.ran(MG.routes(ctx), before)
            ctx.close()
            ctx = sipx.host.build_context(m, AtAs, As, props, Ps, gs, os_)
            before = MG.routes(ctx)
            log, _ = ctx.parsdmm(os_)
            took = MG.ran(MG.routes(ctx), before)
            xs, ls, ys = ctx.download()
        finally:
            ctx.close()
        # the products ran marched, on the table / on the bands as switched: the engine's own count of launches per route
        form, other = ("/table", "/bands") if tab == "1" else ("/bands", "/table")
        assert took_q == {"k_cds_march<MODE=0>" + form: 3}, f"SIPX_Q_TABLE={tab}: apply_Q did not take the march on {form[1:]} three times: {took_q}"
        MG.assert_route(took, [f"k_cds_march<MODE={k}>{form}" for k in (1, 2, 3)], MG.MARCH_ONLY + [other], f"SIPX_Q_TABLE={tab}")
        out[tab] = (state, y0, y1, Q4, y4, log, xs, ls, ys)
    on, off = out["1"], out["0"]
    assert on[0]["on"] is True and on[0]["reason"] == "", on[0]
    assert off[0]["on"] is False and off[0]["reason"] == "SIPX_Q_TABLE=0", off[0]
    assert np.array_equal(on[1], want) and np.array_equal(off[1], want)
    for k in (2, 3, 4):
        assert np.array_equal(on[k], off[k]), k
    _same_log(on[5], off[5])
    assert np.array_equal(on[6], off[6])
    for a, b in zip(on[7], off[7]):
        assert np.array_equal(a, b)
    for a, b in zip(on[8], off[8]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("TF", [np.float32, np.float64])
def test_a_q_that_is_not_class_constant_keeps_the_bands(sipx, monkeypatch, TF):
    """Explicit A'A bands with one diagonal entry changed (still symmetric, so the march applies): the table check finds the
    mismatch, the products read the bands and give the oracle's bits, and the counter says why."""
    n, h, kinds = (40, 24, 20), (25.0, 20.0, 10.0), ["bounds", "l1:D_x", "l1:D_y", "l1:D_z"]
    monkeypatch.setenv("SIPX_CDS_MARCH", "2")
    monkeypatch.setenv("SIPX_CDS_MARCH_ZCHUNK", "4")
    m = model(n, TF, seed=6)
    go, oo, Po, Ao, propo, AtAo = _problem(O, n, h, TF, kinds, m)
    gs, os_, Ps, As, props, AtAs = _problem(sipx, n, h, TF, kinds, m)
    rho = [2.0, 3.0, 5.0, 7.0, 1.5][:len(Ao)]
    x = np.random.default_rng(3).standard_normal(m.size).astype(TF)
    os_.rho_ini = rho
    # as handed over: class-constant, the table is used; an update of explicit bands has no plan -> the bands from then on
    ctx = sipx.host.build_context(m, AtAo, As, propo, Ps, gs, os_)
    try:
        assert _q_table(ctx)["on"] is True
        rho2 = [r * 1.5 for r in rho]
        ctx.q_update(rho2, rho)
        st = _q_table(ctx)
        y2 = ctx.apply_Q(x)
    finally:
        ctx.close()
    assert st["on"] is False and "without a plan" in st["reason"], st
    class L: pass
    log = L(); log.rho = np.array([rho])
    Qo, offo = O.assemble_Q(AtAo, propo.AtA_offsets, np.array(rho, TF), TF)
    Qr = O.Q_update(Qo.copy(order="F"), AtAo, propo, np.array(rho2, TF), list(range(len(rho))), log, 0, offo)
    assert np.array_equal(y2, O.Ax_CDS(x, Qr, offo))
    # one diagonal entry that differs from the rest of its class: refused at the check
    bad = [np.array(a, order="F", copy=True) for a in AtAo]
    bad[0][5, 0] += 0.125
    Qb, offb = O.assemble_Q(bad, propo.AtA_offsets, np.array(rho, TF), TF)
    ctx = sipx.host.build_context(m, bad, As, propo, Ps, gs, os_)
    try:
        st = _q_table(ctx)
        y = ctx.apply_Q(x)
        Q, _ = ctx.get_Q()
    finally:
        ctx.close()
    assert st["on"] is False and "not constant" in st["reason"], st
    assert np.array_equal(y, O.Ax_CDS(x, Qb, offb))
    assert np.array_equal(Q, Qb)


@pytest.mark.timeout(900)
def test_full_size_c3_same_bits_with_and_without_the_table(sipx, monkeypatch):
    """The headline problem at its own size (256^3 Float32, bounds + l1 on D_x, D_y, D_z): 20 iterations with the table on and
    off end on the same x and the same log, bit for bit."""
    TF, n, h = np.float32, (256, 256, 256), (25.0, 25.0, 25.0)
    kinds = ["bounds", "l1:D_x", "l1:D_y", "l1:D_z"]
    m = model(n, TF, seed=7)
    out = {}
    for tab in ("1", "0"):
        monkeypatch.setenv("SIPX_Q_TABLE", tab)
        gs, os_, Ps, As, props, AtAs = _problem(sipx, n, h, TF, kinds, m, dict(maxit=20, evol_rel_tol=0.0, feas_tol=0.0, obj_tol=0.0))
        ctx = sipx.host.build_context(m, AtAs, As, props, Ps, gs, os_)
        try:
            state = _q_table(ctx)
            log, _ = ctx.parsdmm(os_)
            xs, _, _ = ctx.download()
        finally:
            ctx.close()
        out[tab] = (state, log, xs)
    assert out["1"][0]["on"] is True and out["0"][0]["on"] is False
    assert len(out["1"][1].obj) == 20
    _same_log(out["1"][1], out["0"][1])
    assert np.array_equal(out["1"][2], out["0"][2])
