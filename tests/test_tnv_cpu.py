"""Total nuclear variation without a GPU: the numpy reference (tests/tnv_ref.py), csrc/tnv.h on the CPU (tests/tnv/rule_driver.cpp,
compiled by hipcc; the program makes no HIP call) against the reference -- its singular values bit for bit against the emulation of the
contract, its output within the bound of the projection computed in extended precision --, the singular values of planted near-rank-1
pixels, the routes and refusals of csrc/set_config.h through the existing tests/set_config/config_driver.cpp, the host descriptors and
refusals, and the claims tests/test_gpu_tnv.py makes about the path each of its grids takes and about its inputs lying outside the ball."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import l1_exact, l21_joint_ref as RJ, tnv_ref as R
from tests import test_gpu_tnv as T
from tests.test_gpu_tnv import test_host_refusals_word_for_word  # noqa: F401  (host.py alone: runs here, without the gpu mark)
from tests.test_set_config_cpu import ask, req  # noqa: F401  (the fixture that builds and runs config_driver)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "setintersectionprojection.jl_amd", "csrc")
PROJ_TNV, OP_TV_XY, EXT_TNV = 17, 6, 18


def _heavy(rng, M):
    return rng.standard_normal(M) * np.exp(rng.standard_normal(M))


# ---- the reference -----------------------------------------------------------------------------------------------------------------------
def test_reference_projects_onto_the_boundary_and_aligns_the_frames():
    n, TF = (6, 5, 4), np.float64
    eps = float(np.finfo(TF).eps)
    v = _heavy(np.random.default_rng(12), R.rows(n)).astype(TF)
    nrm = R.norm(v, n)
    s1, s2, U, Rw = R.exact_svd(v, n)
    W = l1_exact._WIDE
    assert np.all(s1 >= s2) and float(np.abs((Rw[:, 0] * Rw[:, 1]).sum(1)).max()) <= 64 * float(np.finfo(W).eps) * float((s1 * s1).max())
    back = np.einsum("lji,ljk->lik", U, Rw)
    assert float(np.abs(back - R.jacobians(v, n, W)).max()) <= 64 * float(np.finfo(W).eps) * float(s1.max()), "R = U J with U orthogonal"
    assert nrm >= RJ.norm21(v, n), "the nuclear norm is at least the Frobenius norm, pixel by pixel"
    for frac in (0.9, 0.5, 0.05):
        tau = TF(frac * nrm)
        assert R.inside(v, n, tau) == -1
        y = R.project(v, n, tau)
        assert abs(R.norm(y, n) - float(tau)) <= 4 * eps * float(tau), "an infeasible point projects onto the boundary of the ball"
        t1, t2, _, _ = R.exact_svd(y, n)
        assert frac > 0.5 or np.count_nonzero(t2 <= 1e-15 * float(s1.max())) > len(t2) // 2, "small radii leave rank-1 pixels: parallel gradients"
    assert R.project(v, n, TF(2 * nrm)) is v and R.inside(v, n, TF(2 * nrm)) == 1


def test_reference_on_a_rank_one_stack_is_the_joint_reference():
    n, TF = (6, 5, 4), np.float64
    v = T._rank1(n, TF, "multiples")
    assert abs(R.norm(v, n) - RJ.norm21(v, n)) <= 1e-14 * RJ.norm21(v, n)
    tau = TF(0.5 * RJ.norm21(v, n))
    y, want = R.project(v, n, tau), RJ.project(v, n, tau)
    assert np.array_equal(y == 0, want == 0) and float(R.error(y, want, v, n).max()) <= 2 * np.finfo(TF).eps


def test_two_prod_is_exact():
    rng = np.random.default_rng(3)
    x, y = _heavy(rng, 2000), _heavy(rng, 2000)
    p, e = R._two_prod(x, y)
    W = l1_exact._WIDE
    if np.finfo(W).eps < np.finfo(np.float64).eps:
        assert np.all(np.abs((x.astype(W) * y.astype(W) - p.astype(W)) - e.astype(W)) <= np.abs(p) * 2.0 ** -63)
    assert np.all(np.abs(e) <= np.spacing(np.abs(p)) / 2) and R._two_prod(np.float64(3.0), np.float64(3.0))[1] == 0.0


# ---- csrc/tnv.h on the CPU ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    hipcc = shutil.which("hipcc") or shutil.which("hipcc", path=os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin"))
    assert hipcc, "hipcc not found"
    d = tmp_path_factory.mktemp("tnv")
    exe = str(d / "rule_driver")
    r = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                        "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "tnv", "rule_driver.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe, str(d)


def _rule(driver, n, TF, vp, thetas):
    """(s, rot, [blocks after the scaling with theta, one per theta]) of the header on the padded blocks vp."""
    exe, d = driver
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    np.ascontiguousarray(vp, TF).tofile(fin)
    line = f"{'f' if TF == np.float32 else 'd'} {n[0]} {n[1]} {n[2]} {fin} {fout} " + " ".join(float(t).hex() for t in thetas)
    r = subprocess.run([exe], input=line + "\n", capture_output=True, text=True)
    out = r.stdout.splitlines()
    assert r.returncode == 0 and out and out[-1] == "ok" and out[0] == f"done {n[0] * n[1]} {len(thetas)}", r.stdout[-2000:] + r.stderr
    assert "words 3 6" in out
    raw = np.fromfile(fout, TF)
    L, N = n[0] * n[1], n[0] * n[1] * n[2]
    assert len(raw) == 4 * L + 2 * N * len(thetas)
    return raw[:2 * L], raw[2 * L:4 * L], [raw[4 * L + 2 * N * t:4 * L + 2 * N * (t + 1)] for t in range(len(thetas))]


def _padded(v, n, pad):
    """The two padded blocks (D_y, D_x) of the M-vector v, N entries each, `pad` in the rows a block does not have; the mask of the
    rows that exist; the M-vector indices of those rows."""
    G = RJ.groups(n)
    N = G.shape[0]
    out = np.full(2 * N, pad, v.dtype)
    idx = np.full(2 * N, -1, np.int64)
    for q in range(2):
        has = G[:, q] >= 0
        out[q * N + np.nonzero(has)[0]] = v[G[has, q]]
        idx[q * N + np.nonzero(has)[0]] = G[has, q]
    return out, idx >= 0, idx


_worst = {}


@pytest.mark.parametrize("TF", T.PRECISIONS)
@pytest.mark.parametrize("n", T.GRIDS)
def test_rule_meets_the_reference_within_the_bound(driver, TF, n):
    """The measurement the bound of both test files comes from: the CPU rule against tnv_ref.project on every grid, radius and precision
    of tests/test_gpu_tnv.py.  Also: s bit for bit the emulation of the contract, pads (NaN here) neither used nor written, and the
    reference alone says every input is clearly outside its ball."""
    eps = float(np.finfo(TF).eps)
    v, nrm, pre = T._input(n, TF)
    vp, has, idx = _padded(v, n, TF(np.nan))
    taus, refs = [], []
    for frac in T.FRACS:
        tau, ref, inside = T._reference(n, TF, frac)
        assert inside == -1, (n, frac)
        taus.append(tau)
        refs.append(ref)
    thetas = [TF(l1_exact.exact_theta(pre[0].astype(np.float64), t)[0]) for t in taus]
    s, rot, outs = _rule(driver, n, TF, vp, thetas)
    assert l1_exact.same_bits(s, pre[0]), "the header's singular values are not the contract's"
    s1, s2, cs, sn = R.decompose(v, n, TF)
    assert l1_exact.same_bits(rot, np.concatenate([cs, sn]))
    assert np.all(s[:len(s) // 2] >= s[len(s) // 2:]) and s[len(s) // 2 - 1] == 0, "sigma1 >= sigma2; the last corner pixel has no member"
    for frac, ref, out in zip(T.FRACS, refs, outs):
        assert np.isnan(out[~has]).all(), "a pad row was written"
        y = np.zeros_like(v)
        y[idx[has]] = out[has]
        assert np.isfinite(y).all(), "a pad row was used"
        worst = float(R.error(y, ref, v, n).max()) / eps
        key = np.dtype(TF).name
        _worst[key] = max(_worst.get(key, 0.0), worst)
        print(f"tnv rule {n} {key} frac {frac}: worst error {worst:.3f} eps |J_p|_F (bound {R.BOUND[TF]}); so far {_worst[key]:.3f}")
        assert worst <= R.MEASURED[TF] + 0.005, "a worst error above the recorded one: tnv_ref.MEASURED and BOUND are to be set again"
    assert R.BOUND[TF] == max(4, math.ceil(2 * R.MEASURED[TF])) and R.MEASURED[np.float64] <= 8


@pytest.mark.parametrize("TF", T.PRECISIONS)
def test_sigma2_of_near_rank_one_pixels(driver, TF):
    """Planted near-rank-1 pixels: sigma2 / sigma1 about 1e-4 (Float64: 1e-9) and exactly 0.  The plain float64 evaluation of
    a b - c^2 loses sigma2 of Float64 to an error of order sqrt(eps) sigma1; in twice the working precision the sums carry a relative
    (n3 + 4) eps^2, which is an error of at most sqrt(n3 + 4) eps sigma1 in sigma2 however small it is, plus the roundings of lambda1,
    the quotient and the root (2 eps sigma2).  Float32: the float64 sums give sqrt((n3 + 4) eps64) sigma1, and half an ulp of Float32."""
    eps, e64 = float(np.finfo(TF).eps), float(np.finfo(np.float64).eps)
    for n in ((8, 4, 67), (33, 20, 3)):
        v, _, pre = T._input(n, TF)
        L = n[0] * n[1]
        vp, has, idx = _padded(v, n, TF(0))
        s, _, _ = _rule(driver, n, TF, vp, [])
        e1, e2 = pre[1][0].astype(np.float64), pre[1][1]
        p = np.arange(L)
        near = np.nonzero((RJ._members(n) >= 0).all(axis=(1, 2)) & (p % 7 == 0) & (p % 11 != 0) & (p % 13 != 0))[0]
        ratio = (e2[near] / e1[near]).astype(np.float64)
        assert len(near) and np.median(ratio) < (1e-3 if TF == np.float32 else 1e-8), "the planted pixels are nearly rank 1"
        err = np.abs(s[L:].astype(l1_exact._WIDE) - e2).astype(np.float64)
        if TF == np.float64:
            tol = (2.0 + math.sqrt(n[2] + 4)) * eps * e1
        else:
            tol = (0.5 * eps + math.sqrt((n[2] + 4) * e64)) * e1
        print(f"tnv sigma2 {n} {np.dtype(TF).name}: worst error on the planted pixels {float((err[near] / e1[near]).max()) / eps:.3e} eps sigma1, "
              f"on all pixels {float((err / np.maximum(e1, 1e-300)).max()) / eps:.3e} eps sigma1")
        assert np.all(err <= tol)
        assert np.all(np.abs(s[:L].astype(l1_exact._WIDE) - pre[1][0]).astype(np.float64) <= 2.5 * eps * e1)


def test_the_grids_of_the_gpu_test_take_the_paths_its_docstring_names():
    NB, BLOCK = 2048, 256
    want = {(4, 3, 2): (1, True), (5, 4, 3): (1, False), (33, 20, 3): (1, False), (32, 12, 8): (1, True), (8, 4, 67): (8, True),
            (4, 3, 15): (1, True), (4, 3, 16): (2, True), (1024, 1028, 2): (1, True), (1021, 515, 2): (1, False)}
    assert set(T.GRIDS) == set(want)
    for n, (nchunk, wide) in want.items():
        for eb in (4, 8):
            assert RJ.plan(n[0] * n[1], n[2], eb)[0] == nchunk, n
        assert (n[0] % 4 == 0) == wide
        assert 2 * n[0] * n[1] <= int(np.prod(n)), "the search over 2 L entries fits the N entries of scratch"
    assert RJ.plan(8 * 4, 67, 4) == (8, 9) and 67 - 7 * 9 == 4 < 9, "(8, 4, 67): a ragged last chunk, shorter than the others"
    assert 33 * 20 > BLOCK, "(33, 20, 3): more than one workgroup"
    N = 1024 * 1028 * 2
    assert N // 4 > NB * BLOCK and N // 2 > NB * BLOCK and 1024 * 1024 * 2 // 4 <= NB * BLOCK, "a second sweep of the apply kernel"
    assert 1021 * 515 > NB * BLOCK and 1021 % 4 and 1021 * 515 < 2 * NB * BLOCK, "a second, partial sweep of the Gram kernel, one pixel per thread"
    for eb in (4, 8):
        for n in T.OBSERVE_GRIDS + T.RANK1_GRIDS + T.SOLVE_GRIDS:
            assert (RJ.plan(n[0] * n[1], n[2], eb)[0] > 1) == (n in T.CHUNKED), n
    assert set(T.SOLVE_GRIDS) == {(33, 20, 3), (8, 4, 67)}


def test_exact_cases_are_what_their_comments_say():
    for entries, tau, expect in T.EXACT:
        for TF in T.PRECISIONS:
            v, want = T._exact_vector(T.EXACT_N, TF, entries), T._exact_vector(T.EXACT_N, TF, expect)
            assert abs(R.norm(v, T.EXACT_N) - float(np.abs(v).sum())) == 0 and float(np.abs(v).sum()) > tau
            assert np.array_equal(R.project(v, T.EXACT_N, TF(tau)), want.astype(np.float64))


# ---- routes and refusals of csrc/set_config.h ----------------------------------------------------------------------------------------------
N3 = (16, 12, 8)


def test_route(ask):  # noqa: F811
    for tf in ("f", "d"):
        a, joint = ask([req(N3, tf, op=OP_TV_XY, proj=PROJ_TNV, pmax=2.5), req(N3, tf, op=OP_TV_XY, proj=15, pmax=2.5)])
        assert isinstance(a, dict), a
        assert (int(a["ext_kind"]), int(a["prox"]), int(a["nblk"]), int(a["two_pass"])) == (EXT_TNV, 8, 2, 0)
        assert a["dir"] == "1,0,0" and a["spec.bdir"] == "1,0,0" and int(a["spec.nblk"]) == 2 and int(a["spec.mode"]) == 0
        assert int(a["Mtrue"]) == R.rows(N3) and int(a["Mpad"]) == 2 * int(np.prod(N3)) and int(a["needs_ext"]) == 1
        assert int(a["seg_radii"]) == 0 and int(a["nub"]) == 0 and int(a["nlb"]) == 0
        for k in ("Mtrue", "Mpad", "blk_rows", "ata_off", "spec.dims", "ih"):
            assert a[k] == joint[k], k


def test_every_refusal(ask):  # noqa: F811
    ok = dict(op=OP_TV_XY, proj=PROJ_TNV, pmax=1.0)
    lines = [req(N3, **dict(ok, op=op)) for op in (0, 1, 2, 3, 4)]                                  # wrong op
    lines += [req(N3, **dict(ok, mode=m, dir=d)) for m, d in ((1, 0), (1, 2), (2, 0), (2, 2))]     # wrong mode
    lines += [req(N3, **dict(ok, tr=t)) for t in (1, 2)]                                           # a transform
    lines += [req(N3, **dict(ok, op=5, csc="3/" + ",".join(["0"] + ["1"] * int(np.prod(N3))) + "/0"))]   # a custom operator
    for a in ask(lines):
        assert a == T.ROUTE, a
    ones = [1.0] * (N3[0] * N3[1])
    assert ask([req(N3, **dict(ok, lb=ones)), req(N3, **dict(ok, ub=ones))]) == [T.NO_WEIGHTS] * 2
    assert ask([req(N3, **dict(ok, op=4, lb=ones))]) == [T.ROUTE], "the route comes first"
    for r in (0.0, -2.0, float("nan")):
        assert ask([req(N3, **dict(ok, pmax=r))]) == [T.RADIUS]
    # the operator's own refusals, with their existing texts
    assert ask([req((16, 12), **ok), req((4, 3, 1), **ok)]) == [T.NEEDS_3D] * 2
    assert ask([req(N3, **dict(ok, comp=1))]) == ["the TV_xy operator takes no Minkowski component"]
    assert ask([req(N3, single=0, **ok)]) == [T.SHARDED]
    assert ask([req(N3, **dict(ok, op=4, single=0))]) == [T.ROUTE]
    # the joint set still answers with its own text
    assert ask([req(N3, op=4, proj=15, pmax=1.0)]) == ["the joint l2,1 ball groups the frames of TV_xy: TD_OP must be TV_xy, mode tensor"]


# ---- host side -------------------------------------------------------------------------------------------------------------------------------
def test_descriptor_and_exports(sipx):
    TF = np.float32
    g = sipx.compgrid((25.0, 10.0, 6.0), N3)
    assert sipx.host.PROJ["tnv"] == PROJ_TNV and sipx.host.PROJ["l21_groups"] == 16
    assert sipx.host.TNV_NEEDS_TV_XY == T.ROUTE and sipx.host.TNV_NO_WEIGHTS == T.NO_WEIGHTS
    P, A, prop = sipx.setup_constraints([sipx.set_definitions("tnv", "TV_xy", 0.0, 3.5, ("tensor", ""))], g, TF)
    assert prop.tag[0] == ("tnv", "TV_xy", "tensor", "") and prop.ncvx == [False] and A[0].kind == "TV_xy"
    d = P[0].desc(A[0].kind, False)
    assert (d.op, d.proj, d.mode, d.dir, d.transform, d.pmin, d.pmax, d.lb, d.ub, d.reserved) == (6, 17, 0, 0, 0, 0.0, 3.5, None, None, 0)
    assert P[0].kind == "tnv" and P[0].op == "TV_xy" and not P[0].seg_radii and not P[0].weighted and P[0].data_len(A[0]) is None
    P[0].check_rows(A[0])
    for s in ("sipx_tnv_norm", "sipx_tnv_norm_dev"):
        assert s in sipx.EXPORTED_SYMBOLS
    assert callable(sipx.tnv_norm)
    with pytest.raises(sipx.SipxError, match=f"TV_xy range: {R.rows(N3)} entries on this grid, 7 given"):
        P[0](np.zeros(7, TF))
    with pytest.raises(sipx.SipxError, match="x must be a Float32 or Float64"):
        sipx.tnv_norm(np.zeros(int(np.prod(N3)), np.int32), g)
    with pytest.raises(sipx.SipxError) as e:
        sipx.tnv_norm(np.zeros(16 * 12, TF), sipx.compgrid((25.0, 6.0), (16, 12)))
    assert str(e.value) == T.NEEDS_3D
    with pytest.raises(sipx.SipxError, match="TV_xy operator is not built for PARSDMM_multi_level"):
        sipx.setup_multi_level_PARSDMM(np.zeros(32 * 24 * 16, TF), 2, 2, sipx.compgrid((1.0, 1.0, 1.0), (32, 24, 16)),
                                       [sipx.set_definitions("tnv", "TV_xy", 0.0, 2.0, ("tensor", ""))], sipx.PARSDMM_options(FL=TF))
    opt = sipx.PARSDMM_options(FL=TF)
    A, AtA, l, y = sipx.PARSDMM_precompute_distribute(A, prop, g, opt)
    assert list(prop.AtA_offsets[0]) == [-16, -1, 0, 1, 16] and len(y[0]) == R.rows(N3)
