"""Wavelet-domain sets on the device (TD_OP = "wavelet", sipx.h SIPX_TRANSFORM_WAVELET): the db4 transform of
kernels_dwt.hip against the float64 numpy restatement (tests/dwt_ref.py, pinned to PyWavelets by tests/test_wavelet_cpu.py)
on powers of two and on EDGE_SHAPES (plan() says which launches a grid takes; tests/test_dwt_passes_cpu.py), the projectors x -> W' P(W x) against the oracle's projectors behind the restatement, and whole solves (single level,
multilevel, two ranks sharing one GPU, full size) against the oracle with the wavelet closure substituted into P_sub."""
import functools
import os
import re

import numpy as np
import pytest

from oracle import parsdmm_oracle as O
from tests import dwt_ref as R
from tests.test_gpu_parity import model

pytestmark = pytest.mark.gpu

FEAS_TOL = 1e-4
SHAPES = [(16, 8), (32, 24), (128, 128), (8, 8, 4), (16, 16, 8), (9, 7), (64, 64, 32), (256, 128)]
# grids off the powers of two, every dimension divisible by 2^L: half-lengths that are no multiple of the run lengths RC and RS
# (the partial last run of a thread), axes shorter than the filter inside a pass kernel, levels >= 2 through the compact boxes,
# grids on which no level fits the one-workgroup kernel.  tests/test_dwt_passes_cpu.py holds the list to these paths with plan()
EDGE_SHAPES = [(202, 30), (404, 60), (200, 120), (2, 2050), (2050, 2), (6, 684), (690, 6), (34, 18, 10), (36, 20, 12),
               (72, 40, 24), (128, 128, 4), (2, 2, 1026)]
KERNELS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "setintersectionprojection.jl_amd", "csrc",
                       "kernels_dwt.hip")


@functools.lru_cache(maxsize=None)
def kernel_constants():
    """RC, RS (outputs per thread along the contiguous / a strided axis) and SMALL (the one-workgroup box), as kernels_dwt.hip
    defines them."""
    with open(KERNELS, encoding="utf-8") as f:
        src = f.read()
    return {k: int(re.search(r"^constexpr int %s = (\d+);" % k, src, re.M).group(1)) for k in ("RC", "RS", "SMALL")}


def plan(n):
    """The launches dwt_forward / dwt_inverse take on the grid n: per level ("pass" | "small", ((m, h % R), ...)) with, per axis,
    the length m of the level's box and the remainder of its half-length h = m / 2 by the run length of that axis' pass kernel.
    A level is "small" from the first box of at most SMALL entries on (first_small)."""
    k = kernel_constants()
    b, out = [int(v) for v in n], []
    for _ in range(R.levels(n)):
        kind = "small" if int(np.prod(b)) <= k["SMALL"] else "pass"
        out.append((kind, tuple((m, (m // 2) % (k["RC"] if a == 0 else k["RS"])) for a, m in enumerate(b))))
        b = [m // 2 for m in b]
    return out


def _tol(TF, scale):
    return (2e-6 if TF == np.float32 else 1e-13) * max(1.0, scale)


def _check_transform(sipx, TF, n, x, ref, inv_ref):
    """forward against the restatement, the inverse of the restatement's coefficients, the round trip, the norm, determinism"""
    N = int(np.prod(n))
    c = sipx.dwt(x, n)
    assert c.dtype == TF and c.shape == (N,)
    assert np.abs(c - ref).max() <= _tol(TF, np.abs(ref).max()), n
    xi = sipx.dwt(ref.astype(TF), n, inverse=True)
    assert np.abs(xi - inv_ref).max() <= _tol(TF, np.abs(x).max()) * 4, n
    back = sipx.dwt(c, n, inverse=True)
    assert np.abs(back.astype(np.float64) - x).max() <= _tol(TF, np.abs(x).max()) * 4, n
    nx, nc = np.linalg.norm(x.astype(np.float64)), np.linalg.norm(c.astype(np.float64))
    assert abs(nc - nx) <= (1e-6 if TF == np.float32 else 1e-13) * nx, n
    assert np.array_equal(sipx.dwt(x, n), c), n                        # deterministic: same bits
    assert np.array_equal(sipx.dwt(c, n, inverse=True), back), n


@pytest.mark.parametrize("TF", [np.float32, np.float64])
def test_dwt_matches_restatement(sipx, TF):
    rng = np.random.default_rng(5)
    for n in SHAPES:
        x = rng.standard_normal(int(np.prod(n))).astype(TF)
        ref = R.dwt_vec(x, n)
        _check_transform(sipx, TF, n, x, ref, R.dwt_vec(ref.astype(TF), n, inverse=True))


@pytest.mark.parametrize("TF", [np.float32, np.float64])
@pytest.mark.parametrize("n", EDGE_SHAPES, ids=lambda n: "x".join(map(str, n)))
def test_dwt_matches_restatement_on_edge_grids(sipx, TF, n):
    """The same checks with the same tolerances on EDGE_SHAPES: ragged runs, axes of 2, 4 and 6 inside the pass kernels, compact
    boxes with strides that differ between source and destination, grids without a one-workgroup level."""
    assert all(v % (1 << R.levels(n)) == 0 for v in n)
    x = np.random.default_rng(5 + int(np.prod(n))).standard_normal(int(np.prod(n))).astype(TF)
    ref = R.dwt_vec(x, n)
    _check_transform(sipx, TF, n, x, ref, R.dwt_vec(ref.astype(TF), n, inverse=True))


def _want(st, lo, hi, v, n):
    c = R.dwt_vec(v, n)
    if st == "l1":
        O.project_l1_Duchi(c, hi)
    elif st == "cardinality":
        O.project_cardinality(c, int(hi))
    elif st == "bounds":
        O.project_bounds(c, lo, hi)
    elif st == "l2":
        O.project_l2(c, hi)
    elif st == "annulus":
        O.project_annulus(c, lo, hi)
    return R.dwt_vec(c, n, inverse=True)


def _check_projectors(sipx, TF, n, rng):
    tol = 2e-5 if TF == np.float32 else 1e-11
    N = int(np.prod(n))
    g = sipx.compgrid((1.0,) * len(n), n)
    v = rng.standard_normal(N).astype(TF)
    c = R.dwt_vec(v, n)
    a1, a2 = float(np.abs(c).sum()), float(np.linalg.norm(c))
    for st, lo, hi in [("l1", 0.0, 0.3 * a1), ("bounds", -0.4, 0.6), ("cardinality", 0, N // 5), ("l2", 0.0, 0.5 * a2),
                       ("annulus", 1.2 * a2, 2.0 * a2)]:
        want = _want(st, lo, hi, v.astype(np.float64), n)
        got = sipx.host.Projector(sipx.set_definitions(st, "wavelet", lo, hi, ("matrix", "")), g, TF)(v.copy())
        if st == "cardinality" and TF == np.float32:
            # the k-th largest coefficient is decided on TF-rounded coefficients: allow a swap of near-equal entries
            assert np.linalg.norm(got.astype(np.float64) - want) <= 1e-3 * np.linalg.norm(want), (n, st)
        else:
            assert np.abs(got.astype(np.float64) - want).max() <= tol * max(1.0, np.abs(want).max()), (n, st)
    big = sipx.set_definitions("l1", "wavelet", 0.0, 2.0 * a1, ("matrix", ""))     # inside the ball: v bit for bit
    assert np.array_equal(sipx.host.Projector(big, g, TF)(v.copy()), v), n


@pytest.mark.parametrize("TF", [np.float32, np.float64])
def test_wavelet_domain_projectors(sipx, TF):
    rng = np.random.default_rng(23)
    for n in ((16, 16, 8), (32, 24), (64, 64, 32), (9, 7)):
        _check_projectors(sipx, TF, n, rng)


@pytest.mark.parametrize("TF", [np.float32, np.float64])
@pytest.mark.parametrize("n", [(200, 120), (72, 40, 24), (34, 18, 10), (2050, 2)], ids=lambda n: "x".join(map(str, n)))
def test_wavelet_domain_projectors_on_edge_grids(sipx, TF, n):
    """The five sets behind the transform where its passes take ragged runs; the model inside the l1 ball comes back bit for bit
    through the gated inverse of those launches."""
    _check_projectors(sipx, TF, n, np.random.default_rng(23 + int(np.prod(n))))


def _wavelet_closure(n, r, TF):
    def P(x):
        c = O.project_l1_Duchi(R.dwt_vec(x, n), r)
        x[:] = R.dwt_vec(c, n, inverse=True).astype(TF)
        return x
    return P


def _cons(mod, n, h, TF, m, wavelet_frac=0.5, dz=False, engine=True):
    c = [mod.set_definitions("bounds", "identity", 1600.0, 3900.0, ("matrix", ""))]
    if dz:
        Dz = O.get_TD_operator(O.compgrid(h, n), "D_z", TF)[0]
        c.append(mod.set_definitions("l1", "D_z", 0.0, float(0.5 * np.abs(Dz @ m).sum()), ("matrix", "")))
    r = float(wavelet_frac * np.abs(R.dwt_vec(m, n)).sum())
    c.append(mod.set_definitions("l1", "wavelet" if engine else "identity", 0.0, r, ("matrix", "")))
    return c, r


def _problems(sipx, n, h, TF, m, maxit, dz):
    cs, r = _cons(sipx, n, h, TF, m, dz=dz)
    co, _ = _cons(O, n, h, TF, m, dz=dz, engine=False)
    gs, go = sipx.compgrid(h, n), O.compgrid(h, n)
    # (feas_tol: the approximation coefficient carries most of ||W m||_2, so P(m) is within the default 5e-2 of m and the solve
    #  would stop at once -- in the oracle as here)
    os_, oo = sipx.PARSDMM_options(FL=TF, maxit=maxit, feas_tol=FEAS_TOL), O.PARSDMM_options(FL=TF, maxit=maxit, feas_tol=FEAS_TOL)
    Ps, As, props = sipx.setup_constraints(cs, gs, TF)
    As, AtAs, _, _ = sipx.PARSDMM_precompute_distribute(As, props, gs, os_)
    Po, Ao, propo = O.setup_constraints(co, go, TF)
    Po[-1] = _wavelet_closure(n, TF(r), TF)                    # the wavelet set's P_sub, as get_projector.jl builds it
    Ao, AtAo, _, _ = O.PARSDMM_precompute_distribute(Ao, propo, go, oo)
    assert Ps[-1].transform == 2
    return (gs, os_, Ps, As, props, AtAs), (go, oo, Po, Ao, propo, AtAo)


# (case, dtype) -> bound on the free-running end-point difference after a separation of the traces, as DOCUMENTED_EXCEPTIONS in
# test_gpu_parity.py: the Float64 3-D list separates at iteration 12 (a threshold flip of the Barzilai-Borwein rule on a set whose
# multiplier is rounding noise); the oracle replaying the engine's rho / gamma history agrees to 1e-6, the free-running one
# ends 1.0e-3 away after 60 iterations (measured)
SEPARATED = {("3d-32x32x16", "f64"): 2e-3}


@pytest.mark.parametrize("TF", [np.float32, np.float64])
@pytest.mark.parametrize("case", ["c1-compass-128", "3d-32x32x16", "3d-72x40x24"])
def test_wavelet_solve_matches_oracle(sipx, TF, case):
    """BASELINE config 1's compass crop (128^2, L = 7) with {bounds, l1 behind the wavelet at 0.5 ||W m||_1}, and 3-D grids
    with {bounds, l1 on D_z, l1 behind the wavelet} -- 32 x 32 x 16, and 72 x 40 x 24 (L = 3: two levels of ragged axis passes,
    the second through the compact boxes, then the one-workgroup kernel on 18 x 10 x 6): the criteria of
    test_gpu_parity.py::test_parsdmm_matches_oracle."""
    if case.startswith("c1"):
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c1_compass_128_m.npy")
        m = np.load(path).astype(TF).reshape(-1, order="F")
        n, h, dz = (128, 128), (25.0, 6.0), False
        assert m.size == 128 * 128
    else:
        n, h, dz = tuple(int(v) for v in case[3:].split("x")), (25.0, 25.0, 25.0), True
        m = model(n, TF, seed=31)
    S, Oq = _problems(sipx, n, h, TF, m, 60, dz)
    gs, os_, Ps, As, props, AtAs = S
    go, oo, Po, Ao, propo, AtAo = Oq
    xo, lo, _, _ = O.PARSDMM(m.copy(), AtAo, Ao, propo, Po, go, oo)
    xs, ls, _, _ = sipx.PARSDMM(m.copy(), AtAs, As, props, Ps, gs, os_)
    assert len(ls.obj) > 10 and len(lo.obj) > 10
    K = min(6, len(lo.obj), len(ls.obj))
    rt = 5e-4 if TF == np.float32 else 1e-8
    assert np.array_equal(ls.cg_it[:K], lo.cg_it[:K])
    for f in ("obj", "r_pri_total", "r_dual_total", "rho", "gamma"):
        a, b = np.asarray(getattr(ls, f))[:K], np.asarray(getattr(lo, f))[:K]
        assert np.allclose(a, b, rtol=rt, atol=1e-12), (f, a, b)
    assert np.allclose(ls.set_feasibility[0], lo.set_feasibility[0], rtol=rt)
    err = np.linalg.norm(xs.astype(np.float64) - xo) / np.linalg.norm(xo)
    tol = 5e-4 if TF == np.float32 else 1e-6
    Kc = min(len(ls.obj), len(lo.obj))
    sep_rt = 1e-5 if TF == np.float32 else 1e-6
    sep = next((k for k in range(Kc) if ls.cg_it[k] != lo.cg_it[k] or not np.allclose(ls.rho[k], lo.rho[k], rtol=sep_rt)), None)
    upto = Kc if sep is None else sep
    for f in ("obj", "r_pri_total", "rho", "gamma"):
        a, b = np.asarray(getattr(ls, f))[:upto], np.asarray(getattr(lo, f))[:upto]
        assert np.allclose(a, b, rtol=(5e-4 if TF == np.float32 else 1e-6), atol=1e-12), (f, upto)
    if sep is not None or len(ls.obj) != len(lo.obj):
        # a threshold flip of the Barzilai-Borwein rule: the oracle again with the engine's rho / gamma history (replay)
        _, Or = _problems(sipx, n, h, TF, m, len(ls.obj), dz)
        gr, orr, Pr, Ar, propr, AtAr = Or
        xr, _, _, _ = O.PARSDMM(m.copy(), AtAr, Ar, propr, Pr, gr, orr, replay=(ls.rho, ls.gamma))
        assert np.linalg.norm(xs.astype(np.float64) - xr) / np.linalg.norm(xr) < tol, (case, "replayed", sep)
        tol = max(tol, 5e-4, SEPARATED.get((case, "f32" if TF == np.float32 else "f64"), 0.0))
    assert err < tol, (case, sep, err)
    # the wavelet set is active at m, and the solve moved x towards it
    assert np.abs(R.dwt_vec(m, n)).sum() > float(Ps[-1].pmax)
    assert np.abs(R.dwt_vec(xs, n)).sum() < np.abs(R.dwt_vec(m, n)).sum()


def test_wavelet_multilevel_matches_oracle(sipx):
    from sipx import multilevel as ML
    TF, n, h = np.float64, (64, 64, 32), (25.0, 25.0, 25.0)
    m = model(n, TF, seed=37)
    cs, r = _cons(sipx, n, h, TF, m, dz=True)
    co, _ = _cons(O, n, h, TF, m, dz=True, engine=False)
    oo = O.PARSDMM_options(FL=TF, maxit=40, feas_tol=FEAS_TOL)
    Lo = list(O.setup_multi_level_PARSDMM(m, 3, 2, O.compgrid(h, n), co, oo))
    for lev, g in enumerate(Lo[4]):                 # the wavelet closure on every level's grid, radius as constraint2coarse scales it
        nl = tuple(int(v) for v in g.n)
        Lo[2][lev][-1] = _wavelet_closure(nl, TF(r / 8 ** lev), TF)
    xo, logo, _, _ = O.PARSDMM_multi_level(m.copy(), *Lo[:5], oo)
    os_ = sipx.PARSDMM_options(FL=TF, maxit=40, feas_tol=FEAS_TOL)
    Ls = ML.setup_multi_level_PARSDMM(m, 3, 2, sipx.compgrid(h, n), cs, os_)
    assert [tuple(g.n) for g in Ls[4]] == [tuple(g.n) for g in Lo[4]] == [(64, 64, 32), (32, 32, 16), (16, 16, 8)]
    assert all(P[-1].transform == 2 for P in Ls[2])
    assert np.allclose([P[-1].pmax for P in Ls[2]], [r / 8 ** k for k in range(3)], rtol=1e-12)
    xs, logs, _, _ = ML.PARSDMM_multi_level(m.copy(), *Ls[:5], os_)
    assert len(logs.obj) > 1
    err = np.linalg.norm(xs.astype(np.float64) - xo) / np.linalg.norm(xo)
    assert err < 1e-6, err


def _wavelet_worker(rank, world, port, out, n, decomp):
    import datetime
    import sys
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=180))
    try:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        sys.path.insert(0, root)
        from __graft_entry__ import load_package
        sipx = load_package()
        from sipx import sharded
        TF, h = np.float32, (25.0, 25.0, 25.0)
        m = model(n, TF, seed=41)
        cs, _ = _cons(sipx, n, h, TF, m, dz=True)
        g = sipx.compgrid(h, n)
        opt = sipx.PARSDMM_options(FL=TF, maxit=40, feas_tol=FEAS_TOL)
        P, A, prop = sipx.setup_constraints(cs, g, TF)
        A, AtA, _, _ = sipx.PARSDMM_precompute_distribute(A, prop, g, opt)
        x, log, l, y = sharded.PARSDMM_sharded(m.copy(), AtA, A, prop, P, g, opt, dist=dist, device=0, comm_mode="torch",
                                               decomp=decomp)
        np.savez(os.path.join(out, f"r{rank}.npz"), x=x, obj=log.obj, cg_it=log.cg_it, rho=log.rho, r_pri=log.r_pri,
                 feas=log.set_feasibility)
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(400)
@pytest.mark.parametrize("decomp", ["sets", "slab"])
def test_wavelet_two_ranks_on_one_gpu(sipx, tmp_path, decomp):
    """Two ranks sharing GPU 0 (gloo callbacks): the wavelet set takes the owner-rank route of the DCT sets under both the set
    split and the slab decomposition; the ranks agree bit for bit, x with the single-rank solve to 5e-4."""
    import torch.multiprocessing as mp
    n, world = (32, 32, 16), 2
    port = 30100 + (os.getpid() % 1500) + (0 if decomp == "sets" else 7)
    mp.spawn(_wavelet_worker, args=(world, port, str(tmp_path), n, decomp), nprocs=world, join=True)
    r0, r1 = np.load(tmp_path / "r0.npz"), np.load(tmp_path / "r1.npz")
    for k in r0.files:
        assert np.array_equal(r0[k], r1[k], equal_nan=True), k
    TF, h = np.float32, (25.0, 25.0, 25.0)
    m = model(n, TF, seed=41)
    cs, _ = _cons(sipx, n, h, TF, m, dz=True)
    g = sipx.compgrid(h, n)
    opt = sipx.PARSDMM_options(FL=TF, maxit=40, feas_tol=FEAS_TOL)
    P, A, prop = sipx.setup_constraints(cs, g, TF)
    A, AtA, _, _ = sipx.PARSDMM_precompute_distribute(A, prop, g, opt)
    xs, ls, _, _ = sipx.PARSDMM(m.copy(), AtA, A, prop, P, g, opt)
    assert len(ls.obj) > 10
    assert np.linalg.norm(r0["x"] - xs) / np.linalg.norm(xs) < 5e-4


@pytest.mark.timeout(900)
def test_wavelet_full_size_256(sipx):
    """256^3 Float32, 20 iterations of {bounds, l1 on D_z, l1 behind the wavelet}; one projector call on the engine's own
    input at full size against the float64 restatement."""
    TF, n, h = np.float32, (256, 256, 256), (25.0, 25.0, 25.0)
    m = model(n, TF, seed=43)
    cs, r = _cons(sipx, n, h, TF, m, dz=True)
    g = sipx.compgrid(h, n)
    opt = sipx.PARSDMM_options(FL=TF, maxit=20, feas_tol=1e-9, evol_rel_tol=1e-12)
    P, A, prop = sipx.setup_constraints(cs, g, TF)
    A, AtA, _, _ = sipx.PARSDMM_precompute_distribute(A, prop, g, opt)
    x, log, _, _ = sipx.PARSDMM(m.copy(), AtA, A, prop, P, g, opt)
    assert np.isfinite(x).all() and len(log.obj) == 20
    fe = np.asarray(log.set_feasibility)[:, 2]
    assert np.isfinite(fe).all() and fe[-1] < fe[0], fe
    got = P[2](m.copy())
    want = _want("l1", 0.0, float(TF(r)), m.astype(np.float64), n)
    assert np.abs(got.astype(np.float64) - want).max() <= 2e-5 * np.abs(want).max()
