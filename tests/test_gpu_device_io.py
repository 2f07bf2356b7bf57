"""PARSDMM_device: the whole solve on tensors that already live on the GPU (sipx_finalize_dev / sipx_reset_dev /
sipx_download_dev).  The device form shares the context's state with the host form once the vectors are in, so every check
against the host form is EQUALITY: x, l, y bit for bit and every log field; no vector may cross PCIe; the call orders itself
against the caller's stream."""
import numpy as np
import pytest
import torch      # (before libsipx.so is loaded: one HIP runtime in the process, see host._check_one_hip_runtime)

from tests.test_gpu_parity import _custom_problem, _minkowski_problem, _problem, model

pytestmark = pytest.mark.gpu

LOG_FIELDS = ("set_feasibility", "r_dual", "r_pri", "r_dual_total", "r_pri_total", "obj", "evol_x", "rho", "gamma", "cg_it", "cg_relres")
C3 = ["bounds", "l1:D_x", "l1:D_y", "l1:D_z"]
H3 = (25.0, 25.0, 25.0)


def _same_logs(a, b):
    for f in LOG_FIELDS:
        x, y = np.asarray(getattr(a, f)), np.asarray(getattr(b, f))
        assert x.shape == y.shape and np.array_equal(x, y, equal_nan=True), f


def _build(sipx, name):
    """(m, (AtA, TD_OP, set_Prop, P_sub, comp_grid, options)) of a problem of the table."""
    if name in ("c3-64-f32", "c3-64-f64"):
        TF, n = (np.float32 if name.endswith("f32") else np.float64), (64, 64, 64)
        m = model(n, TF, seed=3)
        g, opt, P, A, prop, AtA = _problem(sipx, n, H3, TF, C3, m, dict(maxit=30))
    elif name == "tv-2d-odd":                 # sides that are not multiples of 4: no 16-byte path anywhere
        TF, n = np.float32, (30, 21)
        m = model(n, TF, seed=4)
        g, opt, P, A, prop, AtA = _problem(sipx, n, (2.0, 3.0), TF, ["bounds", "l1:TV"], m, dict(maxit=40))
    elif name == "rank-and-dft":              # a materialised projector (slice rank) and a transform set (l1 behind the DFT)
        TF, n = np.float32, (32, 24, 16)
        m = model(n, TF, seed=5)
        g, opt, P, A, prop, AtA = _problem(sipx, n, H3, TF, ["bounds", "rank:3", "l1dft", "l1:TV"], m, dict(maxit=20))
    elif name == "many-blocks":               # 8 terms, 40 operator blocks in l and y together: more than one launch carries (32 segments)
        TF, n = np.float32, (16, 12, 8)
        m = model(n, TF, seed=9)
        g, opt, P, A, prop, AtA = _problem(sipx, n, H3, TF, ["bounds"] + ["l1:TV"] * 6, m, dict(maxit=15))
    elif name == "minkowski":
        TF, n = np.float32, (32, 24)
        m = model(n, TF, seed=6)
        g, opt, P, A, prop, AtA = _minkowski_problem(sipx, n, (25.0, 6.0), TF, m, maxit=30)
    elif name == "feasibility-only":
        TF, n = np.float64, (24, 20, 16)
        m = model(n, TF, seed=7)
        g, opt, P, A, prop, AtA = _problem(sipx, n, H3, TF, ["bounds", "l1:TV"], m, dict(maxit=30, feasibility_only=True))
    elif name == "custom-operator":
        TF, n = np.float32, (30, 22)
        m = model(n, TF, seed=8)
        g, opt, P, A, prop, AtA, _ = _custom_problem(sipx, n, (25.0, 6.0), TF, m, "l1", maxit=30)
    else:
        raise KeyError(name)
    return m, (AtA, A, prop, P, g, opt)


PROBLEMS = ["c3-64-f32", "c3-64-f64", "tv-2d-odd", "rank-and-dft", "minkowski", "feasibility-only", "custom-operator", "many-blocks"]


def _equal_results(dev, host):
    xd, logd, ld, yd = dev
    xh, logh, lh, yh = host
    assert xd.is_cuda and np.array_equal(xd.cpu().numpy(), xh)
    assert len(ld) == len(lh) and len(yd) == len(yh)
    for a, b in zip(list(ld) + list(yd), list(lh) + list(yh)):
        assert a.is_cuda and np.array_equal(a.cpu().numpy(), b)
    _same_logs(logd, logh)


@pytest.mark.parametrize("name", PROBLEMS)
def test_device_form_gives_the_bits_of_the_host_form(sipx, name):
    """PARSDMM_device on torch.from_numpy(m).cuda() == PARSDMM on m: x, l, y with np.array_equal, every log field equal."""
    m, args = _build(sipx, name)
    sipx.clear_context_cache()
    try:
        host = sipx.PARSDMM(m.copy(), *args)
        sipx.clear_context_cache()                                   # (both forms build their own context)
        dev = sipx.PARSDMM_device(torch.from_numpy(m.copy()).cuda(), *args)
        assert not dev[1].context_reused
        _equal_results(dev, host)
        assert len(host[1].obj) > 1, "the solve stopped before it began: nothing was compared"
    finally:
        sipx.clear_context_cache()


@pytest.mark.parametrize("name", ["c3-64-f32", "tv-2d-odd", "minkowski", "many-blocks"])
def test_device_form_takes_a_warm_start(sipx, name):
    """zero_ini_guess = False with device x, l, y of a first solve == the host form given the same arrays."""
    import copy
    m, (AtA, A, prop, P, g, opt) = _build(sipx, name)
    sipx.clear_context_cache()
    try:
        x0, _, l0, y0 = sipx.PARSDMM(m.copy(), AtA, A, prop, P, g, opt)
        opt2 = copy.copy(opt)
        opt2.zero_ini_guess = False
        opt2.maxit = 12
        host = sipx.PARSDMM(m.copy(), AtA, A, prop, P, g, opt2, x0.copy(), [v.copy() for v in l0], [v.copy() for v in y0])
        assert not np.array_equal(host[0], x0)
        up = lambda v: torch.from_numpy(v.copy()).cuda()
        dev = sipx.PARSDMM_device(up(m), AtA, A, prop, P, g, opt2, up(x0), [up(v) for v in l0], [up(v) for v in y0])
        assert dev[1].context_reused                                 # (warm start through sipx_reset_dev)
        _equal_results(dev, host)
        sipx.clear_context_cache()
        dev = sipx.PARSDMM_device(up(m), AtA, A, prop, P, g, opt2, up(x0), [up(v) for v in l0], [up(v) for v in y0])
        assert not dev[1].context_reused                             # (... and through sipx_finalize_dev)
        _equal_results(dev, host)
    finally:
        sipx.clear_context_cache()


def test_device_form_reuses_its_context_and_fills_the_tensors_it_is_given(sipx, monkeypatch):
    TF, n = np.float32, (48, 40, 32)
    m1, m2 = model(n, TF, seed=1), (model(n, TF, seed=2) * TF(0.97) + TF(40.0)).astype(TF)
    g, opt, P, A, prop, AtA = _problem(sipx, n, H3, TF, ["bounds", "l1:TV", "l1:D_z"], m1, dict(maxit=40))
    sipx.clear_context_cache()
    try:
        monkeypatch.setenv("SIPX_CONTEXT_CACHE", "0")
        fresh = sipx.PARSDMM(m2.copy(), AtA, A, prop, P, g, opt)     # a fresh host call: its own context
        assert not fresh[1].context_reused
        monkeypatch.delenv("SIPX_CONTEXT_CACHE")
        _, log1, _, _ = sipx.PARSDMM_device(torch.from_numpy(m1).cuda(), AtA, A, prop, P, g, opt)
        assert not log1.context_reused
        dt = torch.float32
        bx = torch.full((m1.size,), 7.0, dtype=dt, device="cuda")
        bl = [torch.full((a.shape[0],), 7.0, dtype=dt, device="cuda") for a in A]
        by = [torch.full((a.shape[0],), 7.0, dtype=dt, device="cuda") for a in A]
        x2, log2, l2, y2 = sipx.PARSDMM_device(torch.from_numpy(m2).cuda(), AtA, A, prop, P, g, opt, out=(bx, bl, by))
        assert log2.context_reused
        assert x2 is bx and l2 is bl and y2 is by
        _equal_results((x2, log2, l2, y2), fresh)
        # x alone: l and y stay on the device, the x argument is the destination
        x3, log3, l3, y3 = sipx.PARSDMM_device(torch.from_numpy(m2).cuda(), AtA, A, prop, P, g, opt, outputs="x", out=(bx, None, None))
        assert log3.context_reused and x3 is bx and l3 is None and y3 is None
        assert np.array_equal(x3.cpu().numpy(), fresh[0])
        # the host form finds the same context
        x4, log4, _, _ = sipx.PARSDMM(m2.copy(), AtA, A, prop, P, g, opt)
        assert log4.context_reused and np.array_equal(x4, fresh[0])
    finally:
        sipx.clear_context_cache()


def test_device_form_moves_no_vector_over_pcie(sipx):
    """sipx_io_bytes around a device-form call on a cached context: 0 and 0.  Around the host form of the same problem: at least m
    in, at least x out."""
    TF, n = np.float32, (48, 40, 32)
    m = model(n, TF, seed=9)
    g, opt, P, A, prop, AtA = _problem(sipx, n, H3, TF, C3, m, dict(maxit=15))
    sipx.clear_context_cache()
    try:
        md = torch.from_numpy(m).cuda()
        sipx.PARSDMM_device(md, AtA, A, prop, P, g, opt)
        (ctx,) = sipx.host._ctx_cache.values()
        ctx.io_bytes(reset=True)
        _, log, _, _ = sipx.PARSDMM_device(md, AtA, A, prop, P, g, opt)
        assert log.context_reused and ctx.io_bytes() == (0, 0)
        opt.zero_ini_guess = False                                   # a warm start and all outputs: still nothing
        xd, log, ld, yd = sipx.PARSDMM_device(md, AtA, A, prop, P, g, opt, md.clone(), None, None)
        xd, log, ld, yd = sipx.PARSDMM_device(md, AtA, A, prop, P, g, opt, xd, ld, yd)
        assert log.context_reused and ctx.io_bytes() == (0, 0)
        opt.zero_ini_guess = True
        x, log, l, y = sipx.PARSDMM(m.copy(), AtA, A, prop, P, g, opt)
        assert log.context_reused
        h2d, d2h = ctx.io_bytes()
        assert h2d >= m.nbytes and d2h >= x.nbytes
        assert d2h == x.nbytes + sum(v.nbytes for v in l + y)
        # a context built by the device form has not uploaded a vector either
        sipx.clear_context_cache()
        sipx.PARSDMM_device(md, AtA, A, prop, P, g, opt)
        (ctx,) = sipx.host._ctx_cache.values()
        assert ctx.io_bytes() == (0, 0)
    finally:
        sipx.clear_context_cache()


def test_device_form_is_ordered_against_the_callers_stream(sipx):
    """On a stream of the caller's, with no synchronisation between the steps: m comes out of a chain of large tensor operations,
    PARSDMM_device runs, the result is reduced -- all queued on that stream.  What comes out equals the host result."""
    TF, n = np.float32, (48, 40, 32)
    N = int(np.prod(n))
    m0 = model(n, TF, seed=10)
    c1, c2, steps, tiles, pick = TF(1.0009765625), TF(1.5), 24, 512, 5
    m = m0.copy()
    for _ in range(steps):                                           # what the chain below computes, one rounding per operation
        m = (m * c1).astype(TF)
        m = (m + c2).astype(TF)
    g, opt, P, A, prop, AtA = _problem(sipx, n, H3, TF, C3, m, dict(maxit=25))
    sipx.clear_context_cache()
    try:
        xh, logh, _, _ = sipx.PARSDMM(m.copy(), AtA, A, prop, P, g, opt, outputs="x")
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            big = torch.from_numpy(np.tile(m0, tiles)).cuda()        # 126 MB: every operation of the chain is a kernel of its own
            for _ in range(steps):
                big = big * float(c1)
                big = big + float(c2)
            md = big[pick * N:(pick + 1) * N]
            xd, logd, _, _ = sipx.PARSDMM_device(md, AtA, A, prop, P, g, opt, outputs="x")
            top, bottom = xd.max(), xd.min()
            got = (top.item(), bottom.item(), xd.cpu().numpy())      # (read back on the same stream)
        assert np.array_equal(md.cpu().numpy(), m)
        assert got[0] == float(xh.max()) and got[1] == float(xh.min())
        assert np.array_equal(got[2], xh)
        _same_logs(logd, logh)
    finally:
        sipx.clear_context_cache()


def test_dev_calls_refuse_a_slab_decomposed_context(sipx):
    TF, n = np.float32, (16, 12, 8)
    m = model(n, TF, seed=2)
    g, opt, P, A, prop, AtA = _problem(sipx, n, H3, TF, ["bounds", "l1:D_z"], m, dict(maxit=5))
    md = torch.from_numpy(m).cuda()

    def context():
        ctx = sipx.Context(g, TF)
        for i in range(len(P)):
            ctx.add_set(A[i], P[i], prop.ncvx[i])
        ctx.set_decomp("slab")
        return ctx
    ctx = context()
    try:
        with pytest.raises(sipx.SipxError, match="sipx_finalize_dev takes single-process contexts only"):
            ctx.finalize_dev(md, [10.0], 1.0)
    finally:
        ctx.close()
    ctx = context()
    try:
        ctx.finalize(m, [10.0], 1.0)
        with pytest.raises(sipx.SipxError, match="sipx_reset_dev takes single-process contexts only"):
            ctx.reset_dev(md, [10.0], 1.0)
        with pytest.raises(sipx.SipxError, match="sipx_download_dev takes single-process contexts only"):
            ctx.download_dev(md.device)
    finally:
        ctx.close()
