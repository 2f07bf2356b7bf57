"""sipx_set_data / sipx_set_data_dev and host.Solver: the vectors of a data-bearing set -- element-wise or per-fiber bounds, the
relaxed histogram -- replaced in a context that stays alive, the loop of the reference's application examples
(P_sub[end] = x -> project_bounds!(x, LBD, UBD), examples/Indonesia_desaturation/image_desaturation_by_constraint_learning.jl:264).
The contract (include/sipx.h): set_data followed by reset leaves the context in the state finalize leaves a NEW context built
with that data, so everything below compares bits."""
import ctypes as C

import numpy as np
import pytest
import torch      # (before libsipx.so is loaded: one HIP runtime in the process, see host._check_one_hip_runtime)

from oracle import parsdmm_oracle as O      # checker only
from tests import matrix_free_ops as MF
from tests.test_gpu_parity import model
from tests.test_gpu_round5 import _same_logs

pytestmark = pytest.mark.gpu

PRECISIONS = [np.float32, np.float64]
KW = dict(maxit=30, evol_rel_tol=0.0, feas_tol=0.0, obj_tol=0.0)      # every iteration runs


def _op(n, h, TF, name):
    return O.get_TD_operator(O.compgrid(h, n), name, TF)[0]


def _tdn(n, h, TF, name):
    return tuple(int(v) for v in O.get_TD_operator(O.compgrid(h, n), name, TF)[3])


def _box(s, TF, k):
    """An element-wise box around s = A m that cuts (a third of the entries lie outside) without being empty; k varies it."""
    w = TF(0.4 + 0.1 * k) * TF(np.std(s.astype(np.float64)) + 1.0)
    c = (s.astype(np.float64) * 0.9 + 0.1 * np.mean(s)).astype(TF)
    return (c - w).astype(TF), (c + w).astype(TF)


def _fiber_box(s, tdn, ax, TF, k):
    """Per-fiber bounds: one pair per coordinate along ax, around the mean of s over the other dimensions."""
    S = s.astype(np.float64).reshape(tdn, order="F")
    mean = S.mean(axis=tuple(a for a in range(len(tdn)) if a != ax))
    w = (0.3 + 0.1 * k) * (S.std() + 1.0)
    return (mean - w).astype(TF), (mean + w).astype(TF)


def _hist_box(s, TF, k):
    ref = np.sort(0.5 * (s.astype(np.float64) + np.mean(s)))
    w = (0.05 + 0.02 * k) * (np.std(s.astype(np.float64)) + 1.0)
    return (ref - w).astype(TF), (ref + w).astype(TF)


# ---- the lists: name -> (n, h, constraints(mod, TF, m, k) -> (list of set_definitions, {set index: (lb, ub)}), banded) ----------
def _list_box(opname):
    def make(mod, n, h, TF, m, k):
        TV = _op(n, h, TF, "TV")
        lb, ub = _box((_op(n, h, TF, opname) @ m).astype(TF), TF, k)
        c = [mod.set_definitions("bounds", "identity", 1600.0, 3900.0, ("matrix", "")),
             mod.set_definitions("l1", "TV", 0.0, float(0.5 * np.abs(TV @ model(n, TF, seed=21)).sum()), ("matrix", "")),   # (not the image's)
             mod.set_definitions("bounds", opname, lb, ub, ("matrix", ""))]
        return c, {2: (lb, ub)}
    return make


def _list_fibers(mod, n, h, TF, m, k):
    c, data = [], {}
    for i, (opname, d) in enumerate((("identity", "x"), ("D_z", "z"), ("D_x", "y"))):
        tdn = _tdn(n, h, TF, opname)
        lb, ub = _fiber_box((_op(n, h, TF, opname) @ m).astype(TF), tdn, {"x": 0, "y": 1, "z": 2}[d], TF, k)
        c.append(mod.set_definitions("bounds", opname, lb, ub, ("fiber", d)))
        data[i] = (lb, ub)
    return c, data


def _list_hist(mod, n, h, TF, m, k):
    # (behind the identity and behind a difference operator.  sipx_add_set takes the histogram behind operators of ONE block only,
    #  test_histogram_behind_tv_is_not_a_set_the_engine_builds: D_z stands where a list on TV would)
    c = [mod.set_definitions("bounds", "identity", 1600.0, 3900.0, ("matrix", ""))]
    data = {}
    for i, opname in ((1, "identity"), (2, "D_z")):
        lb, ub = _hist_box((_op(n, h, TF, opname) @ m).astype(TF), TF, k)
        c.append(mod.set_definitions("histogram", opname, lb, ub, ("matrix", "")))
        data[i] = (lb, ub)
    return c, data


def _list_custom(mod, n, h, TF, m, k):
    A = MF.dxz(n, h, TF)
    lb, ub = _box((A @ m).astype(TF), TF, k)
    c = [mod.set_definitions("bounds", "identity", 1600.0, 3900.0, ("matrix", "")),
         MF.custom_set(mod, "bounds", A, lb, ub)]
    return c, {1: (lb, ub)}


H2, H3 = (25.0, 6.0), (25.0, 25.0, 25.0)
LISTS = {
    "2d-box-identity": ((24, 20), H2, _list_box("identity"), None),
    "2d-odd-box-identity": ((13, 11), H2, _list_box("identity"), None),          # n1 odd: one element per lane
    "2d-box-tv": ((24, 20), H2, _list_box("TV"), None),                          # one unpack segment per operator block
    "3d-fibers": ((16, 12, 6), H3, _list_fibers, None),
    "3d-odd-fibers": ((13, 11, 5), H3, _list_fibers, None),
    "2d-histograms": ((24, 20), H2, _list_hist, None),
    "2d-custom-banded": ((24, 20), (1.0, 1.0), _list_custom, {}),
    "2d-custom-matrix-free": ((24, 20), (1.0, 1.0), _list_custom, {1: False}),
}


def _setup(sipx, name, TF, m, k, **opt_kw):
    n, h, make, banded = LISTS[name]
    c, data = make(sipx, n, h, TF, m, k)
    g, opt, P, A, prop, AtA = MF.setup(sipx, TF, n, h, c, dict(KW, **opt_kw), banded)
    return (AtA, A, prop, P, g, opt), data


def _models(name, TF):
    n = LISTS[name][0]
    m1, m2 = model(n, TF, seed=21), model(n, TF, seed=22)
    return m1, (m2 * TF(0.97) + TF(40.0)).astype(TF)


_fresh_cache = {}


def _fresh(sipx, name, TF, which):
    """x, l, y and the log of a NEWLY BUILT context with the data of image `which` (1 or 2), once per session, read-only."""
    key = (name, np.dtype(TF).name, which)
    if key not in _fresh_cache:
        m = _models(name, TF)[which - 1]
        (AtA, A, prop, P, g, opt), _ = _setup(sipx, name, TF, m, which)
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


def _assert_same(got, want):
    (x, l, y, log), (xw, lw, yw, logw) = got, want
    x, l, y = _np(x), [_np(v) for v in l], [_np(v) for v in y]
    assert np.array_equal(x, xw)
    assert len(l) == len(lw) and len(y) == len(yw)
    for a, b in zip(l + y, lw + yw):
        assert np.array_equal(a, b)
    _same_logs(log, logw)


def _np(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def _rho_gamma(opt, TF):
    TFt = np.dtype(TF).type
    return [float(TFt(r)) for r in opt.rho_ini], float(TFt(opt.gamma_ini))


# ---- 1. bits ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("TF", PRECISIONS, ids=["f32", "f64"])
@pytest.mark.parametrize("name", list(LISTS))
def test_set_data_then_reset_gives_the_bits_of_a_new_context(sipx, name, TF):
    """Built with the data of image 1 and solved on it; then set_data(image 2's vectors), reset(m2), solve: x, every l_i and y_i
    and every log array equal those of a context newly built with image 2's data.  Again after a solve cut short."""
    m1, m2 = _models(name, TF)
    args1, data1 = _setup(sipx, name, TF, m1, 1)
    _, data2 = _setup(sipx, name, TF, m2, 2)
    want1, want2 = _fresh(sipx, name, TF, 1), _fresh(sipx, name, TF, 2)
    assert not np.array_equal(want1[0], want2[0])
    AtA, A, prop, P, g, opt = args1
    rho, gamma = _rho_gamma(opt, TF)
    ctx = sipx.host.build_context(m1, AtA, A, prop, P, g, opt)
    try:
        log, _ = ctx.parsdmm(opt)
        _assert_same(ctx.download() + (log,), want1)
        for i, (lb, ub) in data2.items():
            ctx.set_data(i, lb, ub)
        ctx.reset(m2, rho, gamma)
        log, _ = ctx.parsdmm(opt)
        _assert_same(ctx.download() + (log,), want2)
        # back to image 1, a solve cut short in the middle of the iteration pattern, then image 2 once more
        for i, (lb, ub) in data1.items():
            ctx.set_data(i, lb, ub)
        ctx.reset(m1, rho, gamma)
        ctx.parsdmm_begin(opt)
        ctx.parsdmm_steps(opt.maxit // 2 + 1)
        for i, (lb, ub) in data2.items():
            ctx.set_data(i, lb, ub)
        ctx.reset(m2, rho, gamma)
        log, _ = ctx.parsdmm(opt)
        _assert_same(ctx.download() + (log,), want2)
    finally:
        ctx.close()


def test_histogram_behind_tv_is_not_a_set_the_engine_builds(sipx):
    """sipx_set_data takes every operator sipx_add_set takes for its kinds; the histogram behind TV is not among them (the
    library-backed projectors act on one operator block), so the histogram list above stands on the identity and on D_z."""
    TF, n, h = np.float32, (24, 20), H2
    m = model(n, TF, seed=21)
    lb, ub = _hist_box((_op(n, h, TF, "TV") @ m).astype(TF), TF, 1)
    c = [sipx.set_definitions("histogram", "TV", lb, ub, ("matrix", ""))]
    g, opt, P, A, prop, AtA = MF.setup(sipx, TF, n, h, c, KW)
    with pytest.raises(sipx.SipxError, match="operator with one block"):
        sipx.host.build_context(m, AtA, A, prop, P, g, opt)


# ---- 2. the device form --------------------------------------------------------------------------------------------------------
def _torch(sipx):
    sipx.host._check_one_hip_runtime()
    return torch, torch.device("cuda", 0)


@pytest.mark.parametrize("TF", PRECISIONS, ids=["f32", "f64"])
@pytest.mark.parametrize("name", ["2d-box-tv", "2d-odd-box-identity", "3d-fibers", "3d-odd-fibers", "2d-histograms", "2d-custom-matrix-free"])
def test_solver_on_tensors_gives_the_bits_of_the_host_form(sipx, name, TF):
    """The same problems through Solver with torch tensors: image 1, then image 2's data by set_data (sipx_set_data_dev) and m2
    (sipx_reset_dev).  No vector crosses PCIe on the way: io_bytes stands still."""
    torch, dev = _torch(sipx)
    m1, m2 = _models(name, TF)
    args1, _ = _setup(sipx, name, TF, m1, 1)
    _, data2 = _setup(sipx, name, TF, m2, 2)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    with sipx.Solver(*args1, TF) as S:
        x, log, l, y = S(t(m1))
        assert not log.context_reused
        _assert_same((x, l, y, log), _fresh(sipx, name, TF, 1))
        before = S.ctx.io_bytes()
        for i, (lb, ub) in data2.items():
            S.set_data(i, t(lb), t(ub))
        x, log, l, y = S(t(m2))
        assert log.context_reused and x.device == dev
        assert S.ctx.io_bytes() == before
        _assert_same((x, l, y, log), _fresh(sipx, name, TF, 2))


@pytest.mark.parametrize("name", ["2d-box-tv", "3d-fibers"])
def test_bounds_computed_on_the_current_stream_are_the_bounds_of_the_solve(sipx, name):
    """lb / ub come out of a torch op queued on the current stream immediately before set_data, nothing is synchronised, and the
    buffers are overwritten right after the call: the solve uses the values the op produced (ordering by events, sipx.h)."""
    TF = np.float32
    torch, dev = _torch(sipx)
    m1, m2 = _models(name, TF)
    args1, _ = _setup(sipx, name, TF, m1, 1)
    _, data2 = _setup(sipx, name, TF, m2, 2)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    staged = {i: (t(lb) * 0.5, t(ub) * 0.5) for i, (lb, ub) in data2.items()}      # (halving and doubling are exact)
    with sipx.Solver(*args1, TF) as S:
        S(t(m1), outputs="x")
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for i, (lo, hi) in staged.items():
                lb, ub = lo * 2.0, hi * 2.0          # produced on `side`, the current stream, right before the call
                S.set_data(i, lb, ub)
                lb.fill_(float("nan")); ub.fill_(float("nan"))      # queued after the call: may reuse the buffers
            x, log, l, y = S(t(m2))
        side.synchronize()
        _assert_same((x, l, y, log), _fresh(sipx, name, TF, 2))


# ---- 3. first build from device data --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("TF", PRECISIONS, ids=["f32", "f64"])
@pytest.mark.parametrize("name", ["2d-box-tv", "3d-odd-fibers", "2d-histograms"])
def test_first_build_takes_its_data_from_device_memory(sipx, name, TF):
    """The Projectors hold placeholders of the right shape; set_data with tensors before the first call; the first call's
    sipx_finalize_dev uses them: the result of a build from the true host arrays."""
    torch, dev = _torch(sipx)
    m1, _ = _models(name, TF)
    args, data = _setup(sipx, name, TF, m1, 1)
    for i in data:
        args[3][i].lb = np.zeros_like(args[3][i].lb)
        args[3][i].ub = np.ones_like(args[3][i].ub)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    with sipx.Solver(*args, TF) as S:
        for i, (lb, ub) in data.items():
            S.set_data(i, t(lb), t(ub))
        x, log, l, y = S(t(m1))
        assert not log.context_reused
        _assert_same((x, l, y, log), _fresh(sipx, name, TF, 1))
    # ... and the host form before finalize: numpy arrays, half of them in a call of their own
    with sipx.Solver(*args, TF) as S:
        for i, (lb, ub) in data.items():
            S.set_data(i, lb=lb)
            S.set_data(i, ub=ub)
        x, log, l, y = S(m1.copy())
        _assert_same((x, l, y, log), _fresh(sipx, name, TF, 1))


# ---- 4. against the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("TF", PRECISIONS, ids=["f32", "f64"])
def test_image_sequence_matches_the_oracle(sipx, TF):
    """Three images through one Solver as the desaturation example runs them: options.zero_ini_guess = false, x_ini and the
    previous y as the start, a data-fit box per image.  The oracle's P_sub[-1] is replaced by a closure per image.
    ||x - x_oracle|| / ||x_oracle|| within the bound tests/test_gpu_parity.py holds bound and l1 lists to: 5e-4 in Float32,
    1e-6 in Float64 (the reference's own serial-vs-parallel tolerance, test/test_PARSDMM_parallel.jl:72)."""
    n, h = (24, 20), H2
    tol = 5e-4 if TF == np.float32 else 1e-6
    images = [model(n, TF, seed=31 + k) for k in range(3)]
    images = [(im * TF(1.0 - 0.02 * k) + TF(25.0 * k)).astype(TF) for k, im in enumerate(images)]
    make = _list_box("identity")
    kw = dict(maxit=60, zero_ini_guess=False)
    cs, _ = make(sipx, n, h, TF, images[0], 0)
    co, _ = make(O, n, h, TF, images[0], 0)
    gs, os_, Ps, As, props, AtAs = MF.setup(sipx, TF, n, h, cs, kw)
    go, oo, Po, Ao, propo, AtAo = MF.setup(O, TF, n, h, co, kw)
    ys = yo = None
    errs = []
    with sipx.Solver(AtAs, As, props, Ps, gs, os_, TF) as S:
        for k, im in enumerate(images):
            lb, ub = _box(im, TF, k)
            x_ini = np.clip(im, TF(1700.0), TF(3800.0)).astype(TF)
            if ys is None:                       # y = TD_OP * x_ini, the example's first start
                yo = [np.asarray(A @ x_ini, TF) for A in Ao]
                ys = [v.copy() for v in yo]
            Po[-1] = lambda v, lb=lb, ub=ub: O.project_bounds(v, lb, ub)
            S.set_data(2, lb, ub)
            xs, logs, _, ys = S(im.copy(), x_ini.copy(), None, [v.copy() for v in ys])
            xo, logo, _, yo = O.PARSDMM(im.copy(), AtAo, Ao, propo, Po, go, oo, x_ini.copy(), [], [v.copy() for v in yo])
            assert logs.context_reused == (k > 0)
            errs.append(float(np.linalg.norm(xs.astype(np.float64) - xo) / np.linalg.norm(xo)))
            print(f"set_data sequence {np.dtype(TF).name} image {k}: iterations {len(logs.obj)} (oracle {len(logo.obj)}), "
                  f"rel. distance of x {errs[-1]:.3e} (bound {tol:.0e})")
    assert all(e < tol for e in errs), errs


# ---- 5. safety and refusals ----------------------------------------------------------------------------------------------------
def test_set_data_reads_the_array_at_the_call_and_none_keeps_a_vector(sipx):
    TF, name = np.float32, "2d-box-tv"
    m1, m2 = _models(name, TF)
    args1, data1 = _setup(sipx, name, TF, m1, 1)
    _, data2 = _setup(sipx, name, TF, m2, 2)
    (lb2, ub2), want2 = data2[2], _fresh(sipx, name, TF, 2)
    with sipx.Solver(*args1, TF) as S:
        buf_lb, buf_ub = data1[2][0].copy(), data1[2][1].copy()
        S.set_data(2, buf_lb, buf_ub)
        S(m1.copy(), outputs="x")
        buf_lb[:] = lb2                          # changed in place: nothing is remembered about the array
        S.set_data(2, buf_lb, None)              # ... and None keeps image 1's ub
        buf_lb[:] = np.nan                       # (read at the call)
        x_mixed, _, _, _ = S(m2.copy(), outputs="x")
        assert not np.array_equal(x_mixed, want2[0])
        S.set_data(2, None, ub2)                 # lb of the call before is kept
        x, log, l, y = S(m2.copy())
        _assert_same((x, l, y, log), want2)
        h2d, _ = S.ctx.io_bytes(reset=True)
        S.set_data(2, lb2, ub2)
        assert S.ctx.io_bytes()[0] == 2 * lb2.nbytes      # the host form counts what it uploads


def _null_comm(sipx):
    from importlib import import_module
    SC = import_module("sipx.sharded")._SipxComm
    ok3 = SC._AR(lambda *a: 0)
    return SC(None, 1, 0, ok3, ok3, ok3, SC._HX(lambda *a: 0), SC._BC(lambda *a: 0), SC._BC(lambda *a: 0))


def test_refusals_name_the_way_out_and_leave_the_context_usable(sipx):
    TF, n, h = np.float32, (24, 20), H2
    N = n[0] * n[1]
    m1, m2 = _models("2d-box-identity", TF)
    lb, ub = _box(m1, TF, 1)
    lb2, ub2 = _box(m2, TF, 2)
    keep = (np.arange(N) % 3 != 0).astype(TF)
    t = np.linspace(0, 1, n[0])
    sub = sipx.set_definitions("subspace", "identity", 0, 0, ("fiber", "x"))
    sub.custom_TD_OP = (np.stack([np.cos(np.pi * q * t) for q in range(4)], axis=1).astype(TF), False)
    c = [sipx.set_definitions("bounds", "identity", lb, ub, ("matrix", "")),                              # 0: takes data
         sipx.set_definitions("bounds", "identity", 1600.0, 3900.0, ("matrix", "")),                      # 1: scalars
         sipx.set_definitions("bounds", "DCT", np.full(N, -1e6, TF), np.full(N, 1e6, TF), ("matrix", "")),  # 2: vectors behind the DCT
         sipx.set_definitions("bounds", "DFT", np.zeros(N, TF), keep, ("matrix", "")),                    # 3: the DFT mask
         sub]                                                                                              # 4: a subspace basis
    g, opt, P, A, prop, AtA = MF.setup(sipx, TF, n, h, c, KW)
    ctx = sipx.host.build_context(m1, AtA, A, prop, P, g, opt)
    try:
        for i in (1, 2, 3, 4):
            with pytest.raises(sipx.SipxError, match=r"holds no replaceable vectors.*build a new context"):
                ctx.set_data(i, lb, ub)
        with pytest.raises(sipx.SipxError, match=r"index 5 is the distance term"):
            ctx.set_data(5, lb, ub)
        for i in (-1, 6):
            with pytest.raises(sipx.SipxError, match=r"out of range \(5 sets\)"):
                ctx.set_data(i, lb, ub)
        with pytest.raises(sipx.SipxError, match="lb has 7 entries, 480 are needed"):
            ctx.set_data(0, np.zeros(7, TF), ub)
        # still the context it was: image 2 by set_data + reset == a new context
        ctx.set_data(0, lb2, ub2)
        rho, gamma = _rho_gamma(opt, TF)
        ctx.reset(m2, rho, gamma)
        log, _ = ctx.parsdmm(opt)
        got = ctx.download() + (log,)
    finally:
        ctx.close()
    c[0] = sipx.set_definitions("bounds", "identity", lb2, ub2, ("matrix", ""))
    g, opt, P2, A2, prop2, AtA2 = MF.setup(sipx, TF, n, h, c, KW)
    ref = sipx.host.build_context(m2, AtA2, A2, prop2, P2, g, opt)
    try:
        log, _ = ref.parsdmm(opt)
        _assert_same(got, ref.download() + (log,))
    finally:
        ref.close()

    # contexts of the class the _dev calls exclude, and Minkowski components: refused before and after finalize
    def build(prepare, minkowski=False):
        cc = [sipx.set_definitions("bounds", "identity", lb, ub, ("matrix", ""))]
        Pm, Am, propm = sipx.setup_constraints(cc, g, TF)
        ctx = sipx.Context(g, TF)
        op = sipx.TDOperator("identity", g, TF, component=1) if minkowski else Am[0]
        assert ctx.add_set(op, Pm[0]) == 0
        prepare(ctx)
        return ctx
    comm = _null_comm(sipx)
    cases = [("sharded or slab-decomposed", lambda ctx: ctx.set_decomp("slab"), False),
             ("sharded or slab-decomposed", lambda ctx: ctx.set_owned([1, 1]), False),
             ("sharded or slab-decomposed", lambda ctx: sipx.host._chk(sipx.lib().sipx_set_comm(ctx.h, C.byref(comm))), False),
             ("Minkowski", lambda ctx: None, True)]
    for msg, prepare, mk in cases:
        ctx = build(prepare, mk)
        try:
            with pytest.raises(sipx.SipxError, match=msg + r".*build a new context"):
                ctx.set_data(0, lb, ub)
        finally:
            ctx.close()
    ctx = build(lambda ctx: ctx.set_owned([1, 1]))
    try:
        ctx.finalize(m1, [10.0], 1.0)
        with pytest.raises(sipx.SipxError, match=r"sharded or slab-decomposed.*build a new context"):
            ctx.set_data(0, lb, ub)
        log, _ = ctx.parsdmm(opt)                # (usable)
        assert len(log.obj) == opt.maxit
    finally:
        ctx.close()
