"""Joint isotropic total variation across frames without a GPU: the numpy reference (tests/l21_joint_ref.py), csrc/l21_joint.h on the
CPU (tests/l21_joint/rule_driver.cpp, compiled by hipcc; the program makes no HIP call) against a numpy emulation of the contract bit
for bit, the launch plan on both sides of its boundaries, the routes and refusals of csrc/set_config.h through the existing
tests/set_config/config_driver.cpp, the host descriptors and refusals, and the claims tests/test_gpu_l21_joint.py makes about the path
each of its grids takes."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import l1_exact, l21_frames_ref as RF, l21_joint_ref as R
from tests.test_set_config_cpu import ask, req  # noqa: F401  (the fixture that builds and runs config_driver)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "setintersectionprojection.jl_amd", "csrc")
JOINT = "the joint l2,1 ball groups the frames of TV_xy: TD_OP must be TV_xy, mode tensor"
UNKNOWN = r"provided an unknown transform domain operator\. check function get_TD_operator\(comp_grid,TD_type,TF\) for options.*TV_xy"
L1_RADIUS = "Radius of L1 ball is negative"
PROJ_JOINT, OP_TV_XY, EXT_L21_JOINT = 15, 6, 16


def _heavy(rng, M):
    return rng.standard_normal(M) * np.exp(rng.standard_normal(M))


# ---- the reference -----------------------------------------------------------------------------------------------------------------------
def test_reference_projects_onto_the_boundary_and_zeroes_whole_pixels():
    n, TF = (6, 5, 4), np.float64
    eps = float(np.finfo(TF).eps)
    v = _heavy(np.random.default_rng(12), R.rows(n)).astype(TF)
    G = R._members(n)
    assert G.shape == (30, 4, 2) and (G[-1] < 0).all(), "the last corner pixel has no member in any frame"
    assert sorted(G[G >= 0]) == list(range(len(v))), "every row of the operator belongs to exactly one pixel"
    nrm = R.norm21(v, n)
    for frac in (0.9, 0.5, 0.05):
        tau = TF(frac * nrm)
        assert R.inside(v, n, tau) == -1
        y = R.project(v, n, tau)
        assert abs(R.norm21(y, n) - float(tau)) <= 4 * eps * float(tau), "an infeasible point projects onto the boundary of the ball"
        gy = R.exact_norms(y, n)
        zeroed = np.nonzero(gy == 0)[0]
        assert frac > 0.5 or len(zeroed) > 1
        for p in zeroed:
            assert np.all(y[G[p][G[p] >= 0]] == 0), "a zeroed pixel is zero in every frame"
        # survivors keep their direction: one factor per pixel in all frames
        p = int(np.argmax(gy))
        mem = G[p][G[p] >= 0]
        assert np.allclose(y[mem] / v[mem], (y[mem] / v[mem])[0], rtol=1e-12)
    assert R.project(v, n, TF(2 * nrm)) is v and R.inside(v, n, TF(2 * nrm)) == 1


def test_reference_with_one_nonzero_frame_is_the_whole_array_reference():
    n, TF = (6, 5, 4), np.float64
    v = np.zeros(R.rows(n), TF)
    mem = RF.frame_rows(n, 2)
    v[mem] = _heavy(np.random.default_rng(13), len(mem))
    tau = TF(0.5 * R.norm21(v, n))
    assert abs(R.norm21(v, n) - RF.norm21(v, n)) <= 1e-12 * RF.norm21(v, n)
    # the same groups, the same exact threshold; the weights come from norms rounded once here and twice there (a float64 sum of two
    # squares, then the root): 2 eps of the weight
    y, want = R.project(v, n, tau), RF.project_whole(v, n, tau)
    assert np.array_equal(y == 0, want == 0) and np.all(np.abs(y - want) <= 2 * np.finfo(TF).eps * np.abs(v))


# ---- csrc/l21_joint.h on the CPU ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    hipcc = shutil.which("hipcc") or shutil.which("hipcc", path=os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin"))
    assert hipcc, "hipcc not found"
    exe = str(tmp_path_factory.mktemp("l21_joint") / "rule_driver")
    r = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                        "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "l21_joint", "rule_driver.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _run(driver, lines):
    r = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True)
    out = r.stdout.splitlines()
    assert r.returncode == 0 and out and out[-1] == "ok", r.stdout[-2000:] + r.stderr
    return out


def _padded(v, n, pad):
    """The two padded blocks (D_y, D_x) of the M-vector v, N entries each, `pad` in the rows a block does not have."""
    G = R.groups(n)
    N = G.shape[0]
    out = np.full(2 * N, pad, v.dtype)
    for q in range(2):
        has = G[:, q] >= 0
        out[q * N + np.nonzero(has)[0]] = v[G[has, q]]
    return out, np.concatenate([G[:, 0] >= 0, G[:, 1] >= 0])


def emulate(vp, has, n, theta, TF):
    """The contract in numpy on the padded blocks: chunked float64 sums in contract order, g, weights and scaling in TF."""
    n1, n2, n3 = n
    L, N = n1 * n2, n1 * n2 * n3
    nchunk, zc = R.plan(L, n3, np.dtype(TF).itemsize)
    sq = np.where(has, vp.astype(np.float64) ** 2, 0.0)
    sy, sx = sq[:N].reshape(L, n3, order="F"), sq[N:].reshape(L, n3, order="F")
    ss = np.zeros(L)
    for c in range(nchunk):
        sc = np.zeros(L)
        for k in range(c * zc, min((c + 1) * zc, n3)):
            sc = sc + sy[:, k]
            sc = sc + sx[:, k]
        ss = ss + sc
    g = np.sqrt(ss).astype(TF)
    t = g - TF(theta)
    t = np.where(t > 0, t, TF(0)).astype(TF)
    with np.errstate(invalid="ignore", divide="ignore"):
        f = np.where(g > 0, t / np.where(g > 0, g, TF(1)), TF(0)).astype(TF)
    w = np.tile(f, 2 * n3)
    out = np.where(has, (vp * w).astype(TF), vp)
    return g, out


RULE_GRIDS = [(4, 3, 2), (5, 4, 3), (3, 2, 15), (3, 2, 16), (4, 2, 67)]


@pytest.mark.parametrize("TF", [np.float32, np.float64])
def test_header_rule_equals_the_emulation_bit_for_bit(driver, TF):
    tag = "f" if TF == np.float32 else "d"
    cases, lines = [], []
    for i, n in enumerate(RULE_GRIDS):
        v = _heavy(np.random.default_rng(50 + i), R.rows(n)).astype(TF)
        v[::5] = -0.0
        vp, has = _padded(v, n, TF(np.nan))                  # what a pad holds is never looked at
        g = R.norms(v, n, TF)
        theta = TF(np.sort(g)[len(g) // 2])                  # half of the pixels are zeroed, one of them exactly on the threshold
        cases.append((n, v, vp, has, theta))
        lines.append(f"{tag} {n[0]} {n[1]} {n[2]} {float(theta).hex()} " + " ".join(float(x).hex() for x in vp))
    out = _run(driver, lines)
    gs = [k.split()[1:] for k in out if k.startswith("g ")]
    vs = [k.split()[1:] for k in out if k.startswith("v ")]
    assert len(gs) == len(vs) == len(cases)
    chunked = 0
    for (n, v, vp, has, theta), gw, vw in zip(cases, gs, vs):
        g_want, v_want = emulate(vp, has, n, theta, TF)
        g_got = np.array([float.fromhex(x) for x in gw]).astype(TF)
        v_got = np.array([float.fromhex(x) for x in vw]).astype(TF)
        assert l1_exact.same_bits(g_got, g_want), n
        assert l1_exact.same_bits(g_got, R.norms(v, n, TF)), "the reference's norms are the contract's"
        assert np.isnan(v_got[~has]).all(), "a pad row was written"
        assert l1_exact.same_bits(v_got[has], v_want[has]), n
        assert g_got[-1] == 0 and np.count_nonzero(v_got[has]) < np.count_nonzero(v)
        chunked += R.plan(n[0] * n[1], n[2], np.dtype(TF).itemsize)[0] > 1
    assert chunked == 2, "the grids with n3 = 16 and 67 are chunked, the others are not"


def test_launch_plan_on_both_sides_of_every_boundary(driver):
    out = _run(driver, [])
    fill, min_chunk = (int(k) for k in [k for k in out if k.startswith("constants ")][0].split()[1:])
    assert (fill, min_chunk) == (R.FILL_THREADS, R.MIN_CHUNK)
    asks = []
    for eb in (4, 8):
        per = 16 // eb
        for L, n3 in ((12, 2), (12, min_chunk - 1), (12, 2 * min_chunk - 1), (12, 2 * min_chunk), (12, 67), (12, 300),
                      (fill * per, 64), (fill * per - per, 64), (fill * per // 2, 64), (fill * per // 2 - per, 64),
                      (256 * 256, 64), (1024 * 1024, 8), (1024 * 1028, 2), (1021 * 515, 2), (1, 1), (fill * per // 8, 67)):
            asks.append((L, n3, eb))
    got = [tuple(int(x) for x in k.split()[1:]) for k in _run(driver, [f"plan {L} {n3} {eb}" for L, n3, eb in asks]) if k.startswith("plan ")]
    assert got == [R.plan(*a) for a in asks]
    plan = dict(zip(asks, got))
    for eb in (4, 8):
        per = 16 // eb
        assert plan[(12, 2 * min_chunk - 1, eb)] == (1, 2 * min_chunk - 1) and plan[(12, 2 * min_chunk, eb)] == (2, min_chunk)
        assert plan[(12, 67, eb)] == (8, 9), "8 chunks of 9 frames, the last one ragged: 4 frames"
        assert plan[(fill * per, 64, eb)] == (1, 64) and plan[(fill * per - per, 64, eb)] == (2, 32), "a frame that fills the device alone"
        assert plan[(fill * per // 2, 64, eb)] == (2, 32) and plan[(fill * per // 2 - per, 64, eb)] == (3, 22)
        assert plan[(1024 * 1028, 2, eb)] == (1, 2) and plan[(1, 1, eb)] == (1, 1)
    for (L, n3, eb), (nchunk, zc) in plan.items():
        assert (nchunk - 1) * zc < n3 <= nchunk * zc and (nchunk == 1 or zc >= min_chunk), "the chunks cover the frames, none is empty"


def test_the_grids_of_the_gpu_test_take_the_paths_its_docstring_names():
    from tests import test_gpu_l21_joint as T
    NB, BLOCK = 2048, 256
    want = {(4, 3, 2): (1, True), (5, 4, 3): (1, False), (33, 20, 3): (1, False), (32, 12, 8): (1, True), (8, 4, 67): (8, True),
            (4, 3, 15): (1, True), (4, 3, 16): (2, True), (1024, 1028, 2): (1, True), (1021, 515, 2): (1, False)}
    assert set(T.GRIDS) == set(want)
    for n, (nchunk, wide) in want.items():
        for eb in (4, 8):
            assert R.plan(n[0] * n[1], n[2], eb)[0] == nchunk, n
        assert (n[0] % 4 == 0) == wide
    assert R.plan(8 * 4, 67, 4) == (8, 9) and 67 - 7 * 9 == 4 < 9, "(8, 4, 67): a ragged last chunk, shorter than the others"
    assert 33 * 20 > BLOCK, "(33, 20, 3): more than one workgroup"
    N = 1024 * 1028 * 2
    assert N // 4 > NB * BLOCK and N // 2 > NB * BLOCK and 1024 * 1024 * 2 // 4 <= NB * BLOCK, "a second sweep of the scale kernel"
    assert 1021 * 515 > NB * BLOCK and 1021 % 4 and 1021 * 515 < 2 * NB * BLOCK, "a second, partial sweep of the norms kernel, one pixel per thread"
    for eb in (4, 8):
        for n in T.OBSERVE_GRIDS:
            assert (R.plan(n[0] * n[1], n[2], eb)[0] > 1) == (n in T.CHUNKED), n
    assert len(T.CHUNKED) == 2 and len(T.OBSERVE_GRIDS) == 4 and set(T.OBSERVE_GRIDS) <= set(T.GRIDS)


# ---- routes and refusals of csrc/set_config.h ----------------------------------------------------------------------------------------------
N3 = (16, 12, 8)


def test_route(ask):  # noqa: F811
    for tf in ("f", "d"):
        a, whole = ask([req(N3, tf, op=OP_TV_XY, proj=PROJ_JOINT, pmax=2.5), req(N3, tf, op=OP_TV_XY, proj=14, pmax=2.5)])
        assert isinstance(a, dict), a
        assert (int(a["ext_kind"]), int(a["prox"]), int(a["nblk"]), int(a["two_pass"])) == (EXT_L21_JOINT, 8, 2, 0)
        assert a["dir"] == "1,0,0" and a["spec.bdir"] == "1,0,0" and int(a["spec.nblk"]) == 2 and int(a["spec.mode"]) == 0
        assert int(a["Mtrue"]) == R.rows(N3) and int(a["Mpad"]) == 2 * int(np.prod(N3)) and int(a["needs_ext"]) == 1
        assert int(a["seg_radii"]) == 0 and int(a["nub"]) == 0 and a["ata_off"] == "-16,-1,0,1,16"
        for k in ("Mtrue", "Mpad", "blk_rows", "ata_off", "spec.dims", "ih"):
            assert a[k] == whole[k], k


def test_every_refusal(ask):  # noqa: F811
    ok = dict(op=OP_TV_XY, proj=PROJ_JOINT, pmax=1.0)
    lines = [req(N3, **dict(ok, op=op)) for op in (0, 1, 2, 3, 4)]                                  # wrong op
    lines += [req(N3, **dict(ok, mode=m, dir=d)) for m, d in ((1, 0), (1, 2), (2, 0), (2, 2))]     # wrong mode
    lines += [req(N3, **dict(ok, tr=t)) for t in (1, 2)]                                           # a transform
    lines += [req(N3, **dict(ok, op=5, csc="3/" + ",".join(["0"] + ["1"] * int(np.prod(N3))) + "/0"))]   # a custom operator
    for a in ask(lines):
        assert a == JOINT, a
    for r in (0.0, -2.0, float("nan")):
        assert ask([req(N3, **dict(ok, pmax=r))]) == [L1_RADIUS]
    # the operator's own refusals, with their existing texts
    a2 = ask([req((16, 12), **ok), req((16, 12, 1), **ok)])
    assert all("provided an unknown transform domain operator" in a and "TV_xy" in a for a in a2)
    assert ask([req(N3, **dict(ok, comp=1))]) == ["the TV_xy operator takes no Minkowski component"]
    assert "the TV_xy operator takes single-process contexts only" in ask([req(N3, single=0, **ok)])[0]
    assert ask([req(N3, **dict(ok, op=4, single=0))]) == [JOINT]
    # the texts ("l21", ...) answers with are still the pinned ones
    for m, d in ((1, 2), (2, 0), (2, 1)):
        assert "frames run along z" in ask([req(N3, op=OP_TV_XY, proj=14, pmax=1.0, mode=m, dir=d)])[0]
    for op in (0, 1, 3):
        assert "the l2,1 ball acts on the range of the TV operator: TD_OP must be TV" in ask([req(N3, op=op, proj=14, pmax=1.0)])[0]


# ---- host side -------------------------------------------------------------------------------------------------------------------------------
H3 = (25.0, 10.0, 6.0)


def test_descriptor_and_exports(sipx):
    TF = np.float32
    g = sipx.compgrid(H3, N3)
    assert sipx.host.PROJ["l21_joint"] == 15 and sipx.host.PROJ["l21"] == 14
    P, A, prop = sipx.setup_constraints([sipx.set_definitions("l21_joint", "TV_xy", 0.0, 3.5, ("tensor", ""))], g, TF)
    assert prop.tag[0] == ("l21_joint", "TV_xy", "tensor", "") and prop.ncvx == [False] and A[0].kind == "TV_xy"
    d = P[0].desc(A[0].kind, False)
    assert (d.op, d.proj, d.mode, d.dir, d.transform, d.pmin, d.pmax, d.ub) == (6, 15, 0, 0, 0, 0.0, 3.5, None)
    assert P[0].kind == "l21_joint" and P[0].op == "TV_xy" and not P[0].seg_radii and P[0].data_len(A[0]) is None
    P[0].check_rows(A[0])
    for s in ("sipx_l21_joint_norm", "sipx_l21_joint_norm_dev"):
        assert s in sipx.EXPORTED_SYMBOLS
    assert callable(sipx.l21_joint_norm)
    for kind in ("TV", "D_x", "identity"):
        with pytest.raises(sipx.SipxError, match="TD_OP must be TV_xy, mode tensor"):
            P[0].check_rows(sipx.TDOperator(kind, g, TF))
    with pytest.raises(sipx.SipxError, match=f"TV_xy range: {R.rows(N3)} entries on this grid, 7 given"):
        P[0](np.zeros(7, TF))
    opt = sipx.PARSDMM_options(FL=TF)
    A, AtA, l, y = sipx.PARSDMM_precompute_distribute(A, prop, g, opt)
    assert list(prop.AtA_offsets[0]) == [-16, -1, 0, 1, 16] and len(y[0]) == R.rows(N3)


def test_host_refusals(sipx):
    TF = np.float32
    g3, g2 = sipx.compgrid(H3, N3), sipx.compgrid((25.0, 6.0), (16, 12))

    def setup(st, op, mx, mode, g, cust=((), False)):
        return sipx.setup_constraints([sipx.set_definitions(st, op, 0.0, mx, mode, cust)], g, TF)
    for op in ("identity", "D_x", "D_z", "TV", "D3D", "DFT", "wavelet"):
        with pytest.raises(sipx.SipxError, match=JOINT):
            setup("l21_joint", op, 1.0, ("tensor", ""), g3)
    for mode in (("slice", "z"), ("slice", "x"), ("fiber", "z"), ("fiber", "y")):
        with pytest.raises(sipx.SipxError, match=JOINT):
            setup("l21_joint", "TV_xy", 1.0, mode, g3)
    import scipy.sparse as sp
    with pytest.raises(sipx.SipxError, match=JOINT):
        setup("l21_joint", "TV_xy", 1.0, ("tensor", ""), g3, (sp.identity(int(np.prod(N3)), format="csc"), False))
    for mx in (0.0, -1.0, float("nan")):
        with pytest.raises(sipx.SipxError, match=L1_RADIUS):
            setup("l21_joint", "TV_xy", mx, ("tensor", ""), g3)
    with pytest.raises(sipx.SipxError, match="takes one radius"):
        setup("l21_joint", "TV_xy", np.ones(8), ("tensor", ""), g3)
    for f in (lambda: setup("l21_joint", "TV_xy", 1.0, ("matrix", ""), g2),
              lambda: sipx.l21_joint_norm(np.zeros(16 * 12, TF), g2),
              lambda: sipx.l21_joint_norm(np.zeros(16 * 12, TF), sipx.compgrid(H3, (16, 12, 1)))):
        with pytest.raises(sipx.SipxError, match=UNKNOWN):
            f()
    with pytest.raises(sipx.SipxError, match="x must be a Float32 or Float64"):
        sipx.l21_joint_norm(np.zeros(int(np.prod(N3)), np.int32), g3)
    with pytest.raises(sipx.SipxError, match="TV_xy operator is not built for PARSDMM_multi_level"):
        sipx.setup_multi_level_PARSDMM(np.zeros(32 * 24 * 16, TF), 2, 2, sipx.compgrid((1.0, 1.0, 1.0), (32, 24, 16)),
                                       [sipx.set_definitions("l21_joint", "TV_xy", 0.0, 2.0, ("tensor", ""))], sipx.PARSDMM_options(FL=TF))
    # the pinned texts of "l21" stay what it answers
    for mode in (("slice", "x"), ("fiber", "z")):
        with pytest.raises(sipx.SipxError, match="frames run along z"):
            setup("l21", "TV_xy", 1.0, mode, g3)
    for op in ("identity", "D_x"):
        with pytest.raises(sipx.SipxError, match="the l2,1 ball acts on the range of the TV operator: TD_OP must be TV"):
            setup("l21", op, 1.0, ("tensor", ""), g3)
