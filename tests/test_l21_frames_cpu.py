"""Per-frame isotropic total variation without a GPU: the numpy reference (tests/l21_frames_ref.py) against the oracle's D_y and D_x,
csrc/l21_seg.h on the CPU (tests/l21_frames/rule_driver.cpp, compiled by hipcc; the program makes no HIP call) against a numpy
emulation of the contract bit for bit, the launch plan on each side of the LDS boundary, the host descriptors and every refusal."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import parsdmm_oracle as O
from tests import l1_exact, l21_frames_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "setintersectionprojection.jl_amd", "csrc")
UNKNOWN = r"provided an unknown transform domain operator\. check function get_TD_operator\(comp_grid,TD_type,TF\) for options.*TV_xy"


# ---- the groups and the reference ----------------------------------------------------------------------------------------------------
def test_groups_agree_with_the_oracle_operators():
    n, h, TF = (6, 4, 3), (25.0, 10.0, 6.0), np.float64
    x = np.random.default_rng(3).standard_normal(n).reshape(-1, order="F")
    g = O.compgrid(h, n)
    v = np.concatenate([np.asarray(O.get_TD_operator(g, k, TF)[0] @ x, TF) for k in ("D_y", "D_x")])
    G = R.groups(n)
    assert v.shape == (R.rows(n),) and G.shape == (x.size, 2)
    assert sorted(G[G >= 0]) == list(range(len(v))), "every row of the operator belongs to exactly one group"
    coords = np.unravel_index(np.arange(x.size), n, order="F")
    X = x.reshape(n, order="F")
    for q, d in enumerate(R.BLOCK_DIRS):
        pad = [(0, 0)] * 3
        pad[d] = (0, 1)
        diff = np.pad(np.diff(X, axis=d) / h[d], pad, constant_values=np.nan).reshape(-1, order="F")
        has = G[:, q] >= 0
        assert np.array_equal(has, coords[d] < n[d] - 1)
        assert np.allclose(v[G[has, q]], diff[has], rtol=1e-12, atol=1e-12)
    last = (coords[0] == n[0] - 1) & (coords[1] == n[1] - 1)
    assert last.sum() == n[2] and (G[last] < 0).all(), "the last corner of every frame has no member"
    for k in range(n[2]):           # no group reaches into another frame
        mem = R.frame_rows(n, k)
        assert np.array_equal(np.sort(G[coords[2] == k][G[coords[2] == k] >= 0]), mem)


def _heavy(rng, M):
    return rng.standard_normal(M) * np.exp(rng.standard_normal(M))


def test_reference_projects_every_frame_on_its_own():
    n, TF = (6, 5, 4), np.float64
    eps = float(np.finfo(TF).eps)
    v = _heavy(np.random.default_rng(12), R.rows(n)).astype(TF)
    fn = R.frame_norms(v, n)
    b = (np.array([0.9, 2.0, 0.5, 0.05]) * fn).astype(TF)
    y = R.project(v, n, b)
    assert list(R.inside(v, n, b)) == [-1, 1, -1, -1]
    got = R.frame_norms(y, n)
    for k in (0, 2, 3):
        assert abs(got[k] - float(b[k])) <= 4 * eps * float(b[k]), "an infeasible frame projects onto the boundary of its ball"
    mem = R.frame_rows(n, 1)
    assert l1_exact.same_bits(y[mem], v[mem].astype(np.float64)), "a frame inside its ball is returned untouched"
    # every frame is the projection of the whole-array reference applied to that frame alone
    for k in (0, 2, 3):
        one = np.zeros_like(v)
        mem = R.frame_rows(n, k)
        one[mem] = v[mem]
        assert np.array_equal(R.project_whole(one, n, b[k])[mem], y[mem])
    assert R.project(v, n, TF(2 * fn.max())) is v


# ---- csrc/l21_seg.h on the CPU -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    hipcc = shutil.which("hipcc") or shutil.which("hipcc", path=os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin"))
    assert hipcc, "hipcc not found"
    exe = str(tmp_path_factory.mktemp("l21_frames") / "rule_driver")
    r = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                        "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "l21_frames", "rule_driver.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _run(driver, lines):
    r = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True)
    out = r.stdout.splitlines()
    assert r.returncode == 0 and out and out[-1] == "ok", r.stdout[-2000:] + r.stderr
    return out


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def emulate_frame(g, tau, vec):
    """The contract of csrc/l21_seg.h in numpy / Python floats, sums serial in index order: (decision, (T)asum, theta, passes)."""
    TF = g.dtype.type
    a = g.astype(np.float64)
    L = len(a)
    asum = float(np.cumsum(a)[-1])
    gmin = float(a.min())
    tau = TF(tau)
    b = float(tau)
    if vec and not tau > 0:
        return (3 if asum > 0 else 0), TF(asum), TF(0), 0
    if TF(asum) <= tau:
        return 0, TF(asum), TF(0), 0
    theta, cprev, passes, done = (asum - b) / L, -1.0, 0, False
    while not done:                                               # l1_seg_start / l1_seg_step
        act = a[a > theta]
        C = float(len(act))
        S = float(np.cumsum(act)[-1]) if len(act) else 0.0
        tn = (S - b) / C if C > 0 else theta
        done = C == cprev or not C > 0
        theta = tn if tn > theta else theta
        cprev = C
        passes += 1
    if cprev >= L and L > 1:                                      # l1_seg_finish
        theta = (asum - gmin - b) / (L - 1)
    theta = TF(theta if theta > 0 else 0.0)
    if TF == np.float64:                                          # l21_theta_refined on the converged active set
        hi = lo = 0.0
        act = a[a > float(theta)]
        for x in act:
            hi, e = _two_sum(hi, float(x))
            lo += e
        C = float(len(act))
        if C > 0 and C < L:
            d, e = _two_sum(hi, -b)
            th = (d + (e + lo)) / C
            theta = TF(th if th > 0 else 0.0)
    return 1, TF(asum), theta, passes


def _frames(TF):
    """(g, tau, vec) of the frames the driver is given."""
    rng = np.random.default_rng(29)
    out = []
    for L, frac in ((12, 0.9), (60, 0.5), (660, 0.05), (660, 0.9), (1500, 0.97), (35, 0.999)):
        g = np.abs(_heavy(rng, L)).astype(TF)
        g[-1] = 0                                                  # the last corner of the frame
        out.append((g, TF(frac * float(g.astype(np.float64).sum())), 0))
    ties = np.array([7, 5, 7, 1, 5, 7, 5, 1, 7, 5, 5, 5, 5, 0], TF)                      # 4 sevens, radius 8: theta = 5 exactly
    out.append((ties, TF(8.0), 1))
    out.append((np.array([3, 3, 3, 3, 0], TF), TF(4.0), 0))                            # all equal: theta = 2, every positive entry stays
    out.append((np.zeros(40, TF), TF(1.0), 1))                                          # an all-zero frame
    g = np.abs(_heavy(rng, 50)).astype(TF)
    out.append((g, TF(2.0 * float(g.astype(np.float64).sum())), 0))                    # inside its ball
    out.append((g, TF(np.cumsum(g.astype(np.float64))[-1]), 0))                        # on its boundary: (T)asum == tau
    one = np.abs(_heavy(rng, 80)).astype(TF)
    one[17] = TF(1e3)
    out.append((one, TF(2.5), 0))                                                       # theta keeps a single group
    out.append((g, TF(0.0), 1))                                                         # device radius 0: the frame is zeroed
    out.append((g, TF(np.nan), 1))
    out.append((np.full(9, 2.0, TF), TF(3.0), 0))                                       # nothing would be zeroed: the rho + 1 < lv cap
    return out


@pytest.mark.parametrize("TF", [np.float32, np.float64])
def test_header_rule_equals_the_emulation_bit_for_bit(driver, TF):
    frames = _frames(TF)
    tag = "f" if TF == np.float32 else "d"
    lines = [f"{tag} {float(tau).hex()} {vec} {len(g)} " + " ".join(float(x).hex() for x in g) for g, tau, vec in frames]
    out = [k.split() for k in _run(driver, lines) if k.startswith("frame ")]
    assert len(out) == len(frames)
    acts, single = [], False
    for (g, tau, vec), w in zip(frames, out):
        act, asum, theta, passes = emulate_frame(g, tau, vec)
        assert int(w[1]) == act and int(w[4]) == passes, (w, act, passes)
        assert l1_exact.same_bits(np.array([float.fromhex(w[2]), float.fromhex(w[3])]).astype(TF), np.array([asum, theta], TF)), (w, asum, theta)
        acts.append(act)
        if act == 1:
            th, C, _ = l1_exact.exact_theta(g.astype(np.float64), tau)
            assert abs(float(theta) - th) <= l1_exact.theta_tol(C, float(g.astype(np.float64).sum()), tau, th, TF)
            single = single or (g > theta).sum() == 1
    assert acts[6:] == [1, 1, 0, 0, 0, 1, 3, 3, 1] and single
    assert float.fromhex(out[6][3]) == 5.0 and float.fromhex(out[7][3]) == 2.0 and float.fromhex(out[14][3]) == 1.625


def test_float64_frame_threshold_is_correctly_rounded(driver):
    """As tests/test_l21_cpu.py asks of the whole-array threshold: within 2^-52 theta* of the exact fixed point."""
    rng = np.random.default_rng(23)
    cases = []
    for L, frac in ((60, 0.9), (660, 0.9), (660, 0.05), (5000, 0.97), (5000, 0.5)):
        g = np.abs(_heavy(rng, L))
        g[-1] = 0.0
        cases.append((g, frac * float(g.sum())))
    lines = [f"d {float(b).hex()} 0 {len(g)} " + " ".join(float(x).hex() for x in g) for g, b in cases]
    out = [k.split() for k in _run(driver, lines) if k.startswith("frame ")]
    for (g, b), w in zip(cases, out):
        th = l1_exact.exact_theta(g, b)[0]
        assert int(w[1]) == 1 and abs(float.fromhex(w[3]) - th) <= 2.0 ** -52 * th, (len(g), w[3], th)


def test_launch_plan_on_each_side_of_the_lds_boundary(driver):
    out = _run(driver, [])
    budget, max_grid = (int(k) for k in [k for k in out if k.startswith("budget ")][0].split()[1:])
    assert budget == 32 * 1024
    asks, want = [], []
    for eb in (4, 8):
        Lfit = budget // eb
        for L, nf in ((Lfit, 3), (Lfit + 1, 3), (12, 2), (96 * 86, 3), (32 * 12, 8), (1024 * 1028, 2), (20, max_grid + 5)):
            asks.append(f"plan {L} {nf} {eb}")
            lds = int(L * eb <= budget)
            want.append([lds, min(nf, max_grid), L * eb if lds else 0, 1 - lds])
    got = [[int(x) for x in k.split()[1:]] for k in _run(driver, asks) if k.startswith("plan ")]
    assert got == want
    assert 96 * 86 * 4 > budget and 96 * 85 * 4 <= budget and 32 * 12 * 8 <= budget       # the grids of tests/test_gpu_l21_frames.py


# ---- host side ----------------------------------------------------------------------------------------------------------------------------
N3, H3 = (16, 12, 8), (25.0, 10.0, 6.0)


def test_operator_shapes_and_offsets(sipx):
    TF = np.float32
    g = sipx.compgrid(H3, N3)
    A = sipx.TDOperator("TV_xy", g, TF)
    n1, n2, n3 = N3
    assert sipx.host.OPS["TV_xy"] == 6 and sipx.host.OPS["TV"] == 4 and sipx.host.OPS["custom"] == 5
    assert A.shape == (R.rows(N3), n1 * n2 * n3) and A.T.shape == A.shape[::-1]
    A2, diag, dense, TD_n, banded = sipx.get_TD_operator(g, "TV_xy", TF)
    assert (A2.kind, diag, dense, TD_n, banded) == ("TV_xy", False, False, (2 * n1 - 1, 2 * n2 - 1, n3), True)
    c = [sipx.set_definitions("l1", "TV_xy", 0.0, 3.0, ("tensor", "")), sipx.set_definitions("bounds", "TV_xy", -1.0, 1.0, ("tensor", ""))]
    P, ops, prop = sipx.setup_constraints(c, g, TF)
    ops, AtA, l, y = sipx.PARSDMM_precompute_distribute(ops, prop, g, sipx.PARSDMM_options(FL=TF))
    for i in range(2):
        assert list(prop.AtA_offsets[i]) == [-n1, -1, 0, 1, n1] and AtA[i] is None and len(y[i]) == R.rows(N3)
        assert P[i].desc(ops[i].kind, False).op == 6


def test_descriptors(sipx):
    TF = np.float32
    g = sipx.compgrid(H3, N3)
    radii = np.linspace(1.0, 2.0, N3[2])
    for mode, mx, want in ((("tensor", ""), 3.5, (0, 0, None)), (("slice", "z"), 3.5, (2, 2, None)), (("slice", "z"), radii, (2, 2, N3[2]))):
        c = [sipx.set_definitions("l21", "TV_xy", 0.0, mx, mode)]
        P, A, prop = sipx.setup_constraints(c, g, TF)
        assert prop.tag[0] == ("l21", "TV_xy", mode[0], mode[1]) and prop.ncvx == [False] and prop.TD_n[0] == (31, 23, 8)
        d = P[0].desc(A[0].kind, False)
        assert (d.op, d.proj, d.mode, d.dir, d.transform, d.pmin) == (6, 14, want[0], want[1], 0, 0.0)
        assert P[0].kind == "l21" and P[0].op == "TV_xy" and P[0].seg_radii == (want[2] is not None)
        P[0].check_rows(A[0])
        assert P[0].data_len(A[0]) == want[2]
        if want[2] is None:
            assert d.ub is None and d.pmax == 3.5
        else:
            assert P[0].ub.dtype == TF and np.array_equal(P[0].ub, radii.astype(TF)) and d.ub == P[0].ub.ctypes.data
    for s in ("sipx_l21_norms", "sipx_l21_norms_dev", "sipx_l21_norm", "sipx_l21_norm_dev"):
        assert s in sipx.EXPORTED_SYMBOLS
    # check_rows: the operator the descriptor was made for, and one radius per frame
    P = sipx.Projector(sipx.set_definitions("l21", "TV_xy", 0.0, radii[:5], ("slice", "z")), g, TF)
    with pytest.raises(sipx.SipxError, match="max has 5 entries, n3 = 8 are needed"):
        P.check_rows(sipx.TDOperator("TV_xy", g, TF))
    P = sipx.Projector(sipx.set_definitions("l21", "TV_xy", 0.0, 1.0, ("slice", "z")), g, TF)
    for kind in ("TV", "D_x", "identity"):
        with pytest.raises(sipx.SipxError, match="TD_OP must be TV"):
            P.check_rows(sipx.TDOperator(kind, g, TF))
    with pytest.raises(sipx.SipxError, match="TD_OP must be TV"):
        sipx.Projector(sipx.set_definitions("l21", "TV", 0.0, 1.0, ("tensor", "")), g, TF).check_rows(sipx.TDOperator("TV_xy", g, TF))
    with pytest.raises(sipx.SipxError, match=f"TV_xy range: {R.rows(N3)} entries on this grid, 7 given"):
        P(np.zeros(7, TF))


def test_refusals(sipx):
    TF = np.float32
    g3, g2 = sipx.compgrid(H3, N3), sipx.compgrid((25.0, 6.0), (16, 12))

    def setup(st, op, mx, mode, g, **kw):
        return sipx.setup_constraints([sipx.set_definitions(st, op, 0.0, mx, mode)], g, TF, **kw)
    # a 2-D grid: TV is in-plane already
    for f in (lambda: sipx.TDOperator("TV_xy", g2, TF), lambda: sipx.get_TD_operator(g2, "TV_xy", TF),
              lambda: setup("l1", "TV_xy", 1.0, ("matrix", ""), g2), lambda: setup("l21", "TV_xy", 1.0, ("matrix", ""), g2),
              lambda: sipx.l21_norm(np.zeros(16 * 12, TF), g2, "TV_xy"),
              lambda: sipx.TDOperator("TV_xy", sipx.compgrid(H3, (16, 12, 1)), TF)):
        with pytest.raises(sipx.SipxError, match=UNKNOWN):
            f()
    # frames run along z
    for mode in (("slice", "x"), ("slice", "y"), ("fiber", "x"), ("fiber", "y"), ("fiber", "z")):
        with pytest.raises(sipx.SipxError, match="frames run along z"):
            setup("l21", "TV_xy", 1.0, mode, g3)
        with pytest.raises(sipx.SipxError, match="frames run along z"):
            sipx.l21_norm(np.zeros(int(np.prod(N3)), TF), g3, "TV_xy", mode)
    # radii
    for mx in (0.0, -1.0, float("nan"), np.array([1.0] * 7 + [0.0]), np.array([1.0, -2.0] * 4), np.array([np.nan] * 8)):
        for mode in (("slice", "z"),) + ((("tensor", ""),) if np.ndim(mx) == 0 else ()):
            with pytest.raises(sipx.SipxError, match="Radius of L1 ball is negative"):
                setup("l21", "TV_xy", mx, mode, g3)
    with pytest.raises(sipx.SipxError, match="takes one radius"):
        setup("l21", "TV_xy", np.ones(8), ("tensor", ""), g3)
    # every existing refusal keeps its text
    for mode in (("fiber", "x"), ("slice", "z")):
        with pytest.raises(sipx.SipxError, match="the l2,1 ball applies to the whole array"):
            setup("l21", "TV", 1.0, mode, g3)
        with pytest.raises(sipx.SipxError, match="the l2,1 ball applies to the whole array"):
            sipx.l21_norm(np.zeros(int(np.prod(N3)), TF), g3, "TV", mode)
    for op in ("identity", "D_x", "D_z", "DFT", "wavelet"):
        with pytest.raises(sipx.SipxError, match="the l2,1 ball acts on the range of the TV operator: TD_OP must be TV"):
            setup("l21", op, 1.0, ("slice", "z"), g3)
    import scipy.sparse as sp
    with pytest.raises(sipx.SipxError, match="TD_OP must be TV"):
        sipx.setup_constraints([sipx.set_definitions("l21", "TV_xy", 0.0, 1.0, ("tensor", ""), (sp.identity(int(np.prod(N3)), format="csc"), False))], g3, TF)
    for st in ("l1", "l2", "annulus"):
        with pytest.raises(sipx.SipxError, match="fiber / slice modes need an operator with one block"):
            sipx.setup_constraints([sipx.set_definitions(st, "TV_xy", 0.5, 1.0, ("slice", "z"))], g3, TF, segment_norms=True)
        with pytest.raises(sipx.SipxError, match="fiber / slice modes need an operator with one block"):
            sipx.setup_constraints([sipx.set_definitions(st, "TV", 0.5, 1.0, ("slice", "z"))], g3, TF, segment_norms=True)


def test_multilevel_and_minkowski_refusals(sipx):
    TF = np.float32
    g = sipx.compgrid((1.0, 1.0, 1.0), (32, 24, 16))
    m = np.zeros(32 * 24 * 16, TF)
    opt = sipx.PARSDMM_options(FL=TF)
    for c in ([sipx.set_definitions("l21", "TV_xy", 0.0, 2.0, ("slice", "z"))], [sipx.set_definitions("l1", "TV_xy", 0.0, 2.0, ("tensor", ""))]):
        with pytest.raises(sipx.SipxError, match="TV_xy operator is not built for PARSDMM_multi_level"):
            sipx.setup_multi_level_PARSDMM(m, 2, 2, g, c, opt)
        P, A, prop = sipx.setup_constraints(c, g, TF)
        A, AtA, l, y = sipx.PARSDMM_precompute_distribute(A, prop, g, opt)
        with pytest.raises(sipx.SipxError, match="TV_xy operator is not built for PARSDMM_multi_level"):
            sipx.PARSDMM_multi_level(m, [A, A], [AtA, AtA], [P, P], [prop, prop], [g, g], opt)
    c1 = [sipx.set_definitions("bounds", "identity", 0.0, 1.0, ("tensor", ""))]
    c2 = [sipx.set_definitions("l1", "TV_xy", 0.0, 2.0, ("tensor", ""))]
    P1, A1, p1 = sipx.setup_constraints(c1, g, TF)
    P2, A2, p2 = sipx.setup_constraints(c2, g, TF)
    for args in ((A1, A2, A1, p1, p2, p1), (A2, A1, A1, p2, p1, p1), (A1, A1, A2, p1, p1, p2)):
        with pytest.raises(sipx.SipxError, match="the TV_xy operator takes no Minkowski component"):
            sipx.PARSDMM_precompute_distribute_Minkowski(*args, g, opt)
    with pytest.raises(sipx.SipxError, match="the TV_xy operator takes no Minkowski component"):
        sipx.TDOperator("TV_xy", g, TF, component=1)
