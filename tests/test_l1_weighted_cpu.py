"""The weighted l1 ball without a GPU: the numpy reference (tests/l1_weighted_ref.py) against the properties of a projection and the plain
l1 ball's exact threshold, csrc/l1_weighted.h on the CPU (tests/l1_weighted/rule_driver.cpp, compiled by hipcc; the program makes no HIP
call) against the Python emulation of the contract bit for bit and against the exact threshold, the host descriptors and refusals, and
the multilevel refusal."""
import copy
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import l1_exact
from tests import l1_weighted_ref as R
from tests.test_l21_weighted_cpu import FAMILIES, _heavy, _search_cases, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "setintersectionprojection.jl_amd", "csrc")
TIE_ABS = (5, 7, 7, 5, 7, 7, 0, 5)
TIE_SIGN = (1, -1, 1, -1, -1, 1, -1, 1)
TIE_W = (2, 2, 1, 2, 2, 1, 1, 2)


def tie(TF):
    """The tie of the issue on the identity at n = (4, 2): theta = 2.5 exactly for tau = 17."""
    v = (np.array(TIE_ABS, TF) * np.array(TIE_SIGN, TF)).astype(TF)      # (the 0 entry: -0.0)
    return v, np.array(TIE_W, TF), TF(17)


# ---- the layout ---------------------------------------------------------------------------------------------------------------------------
def test_rows_and_members():
    assert [R.rows((7, 5), op) for op in ("identity", "D_x", "D_z", "TV")] == [35, 30, 28, 58]
    assert [R.rows((6, 4, 3), op) for op in R.OPS] == [72, 60, 54, 48, 162, 114]
    for n, op in (((7, 5), "TV"), ((6, 4, 3), "TV"), ((6, 4, 3), "TV_xy"), ((5, 4, 3), "D_x"), ((5, 4, 3), "D_y"), ((4, 3), "identity")):
        mem = R.members(n, op)
        nblk = max(len(R.block_dirs(n, op)), 1)
        assert mem.shape == (R.rows(n, op),) and len(np.unique(mem)) == len(mem) and mem.max() < nblk * int(np.prod(n))
    # D_x on (5, 4, 3): the pad is the last entry of every grid line
    assert np.array_equal(np.setdiff1d(np.arange(60), R.members((5, 4, 3), "D_x")), np.arange(4, 60, 5))
    # TV on (4, 3): block 0 = D_z (the last grid line is pad), block 1 = D_x
    assert np.array_equal(R.members((4, 3), "TV"), np.concatenate([np.arange(8), 12 + np.setdiff1d(np.arange(12), [3, 7, 11])]))


# ---- the reference is a projection -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,op", [((7, 5), "identity"), ((6, 4, 3), "D_x"), ((7, 5), "TV"), ((6, 4, 3), "TV"), ((6, 4, 3), "TV_xy")])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("frac", [0.9, 0.5, 0.05])
def test_reference_is_the_projection(n, op, family, frac):
    TF = np.float64
    eps = float(np.finfo(TF).eps)
    rng = np.random.default_rng(37 + sum(n) + len(family) + len(op))
    M = R.rows(n, op)
    v = _heavy(rng, M).astype(TF)
    w = weights(family, rng, M, TF)
    b = TF(frac * R.norm(v, w))
    y = R.project(v, w, b)
    assert y is not v
    y = y.astype(np.float64)
    # the boundary is attained
    assert abs(R.norm(y, w) - float(b)) <= 8 * eps * float(b)
    # <v - y, z - y> <= 0 for every z of the ball, up to the rounding of y (tests/test_l21_weighted_cpu.py)
    for k in range(100):
        z = _heavy(rng, M)
        if k % 4 == 0:
            z[rng.random(M) < 0.7] = 0.0
        nz = R.norm(z, w)
        if nz > 0:
            z *= (1.0 if k % 5 == 0 else rng.random()) * float(b) * (1 - 8 * eps) / nz
        vi = float(np.dot(v - y, z - y))
        assert vi <= 64 * eps * np.linalg.norm(v - y) * np.linalg.norm(z - y), (k, vi)
    # rows of weight 0 are not touched
    assert np.array_equal(y[w == 0], v[w == 0])
    if family == "masked":
        assert np.any(w == 0)


def test_reference_returns_a_feasible_input_itself():
    v = _heavy(np.random.default_rng(5), 58).astype(np.float32)
    w = weights("edge", np.random.default_rng(6), 58, np.float32)
    assert R.project(v, w, np.float32(2 * R.norm(v, w))) is v
    assert R.project(v, np.zeros(58, np.float32), np.float32(1e-3)) is v, "all weights zero: every v is inside"


@pytest.mark.parametrize("TF", [np.float32, np.float64])
def test_all_ones_is_the_plain_l1_ball(TF):
    rng = np.random.default_rng(11)
    for M, frac in ((58, 0.5), (162, 0.05), (1000, 0.9)):
        v = _heavy(rng, M).astype(TF)
        b = TF(frac * np.abs(v.astype(np.float64)).sum())
        th, C, S_act = l1_exact.exact_theta(np.abs(v), b)
        assert 0 < C < M - 1, "the cap of the reference's scan is not in play"
        ts = float(R.theta_star(np.abs(v), np.ones(M, TF), b))
        # l1_exact's own error: its running sum in extended precision (M 2^-64 S_act, and S_act - b cancels), one rounding to float64
        assert abs(ts - th) <= 2.0 ** -52 * th + M * 2.0 ** -63 * (S_act + float(b)) / C, (ts, th)
        y = R.project(v, np.ones(M, TF), b).astype(np.float64)
        plain = np.sign(v) * np.maximum(np.abs(v.astype(np.float64)) - th, 0.0)
        assert np.all(np.abs(y - plain) <= 4 * 2.0 ** -52 * np.abs(v.astype(np.float64)))


def test_theta_star_equals_the_extended_precision_threshold_on_small_inputs():
    rng = np.random.default_rng(13)
    for TF in (np.float32, np.float64):
        for family in FAMILIES:
            a = np.abs(_heavy(rng, 300)).astype(TF)
            w = weights(family, rng, 300, TF)
            tau = TF(0.3 * R.norm(a, w))
            th = R.exact_theta(a, w, tau)
            ts, S, C = R.theta_star_parts(a, w, tau)
            # (exact_theta's own error: running sums in extended precision, 300 2^-64 of S and of C, and S - tau cancels)
            assert abs(float(ts) - th) <= 2.0 ** -52 * th + 300 * 2.0 ** -63 * float((S + S) / C), (float(ts), th)
    assert R.theta_star(np.ones(4, np.float32), np.ones(4, np.float32), np.float32(5)) == 0
    v, w, tau = tie(np.float64)
    assert R.theta_star(np.abs(v), w, tau) == 2.5


# ---- csrc/l1_weighted.h on the CPU -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    hipcc = shutil.which("hipcc") or shutil.which("hipcc", path=os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin"))
    assert hipcc, "hipcc not found"
    exe = str(tmp_path_factory.mktemp("l1_weighted") / "rule_driver")
    r = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                        "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "l1_weighted", "rule_driver.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _txt(x):
    x = float(x)
    return x.hex() if np.isfinite(x) else str(x)


def _cases(TF):
    """(v, w, tau): the searches of tests/test_l21_weighted_cpu.py (several lengths, the four families, three fractions, an input inside,
    all-zero weights, -1 / NaN / inf weights, the tie on magnitudes) with signs on v; then the tie of the issue with its signs."""
    rng = np.random.default_rng(47)
    out = []
    for g, w, tau in _search_cases(TF):
        s = np.where(rng.random(len(g)) < 0.5, TF(-1), TF(1))
        out.append(((g * s).astype(TF), w, tau))          # (a zero magnitude under a negative sign: -0.0)
    out.append(tie(TF))
    return out


def _run(driver, TF, cases):
    tag = "f" if TF == np.float32 else "d"
    lines = [f"p {tag} {_txt(tau)} {len(v)} " + " ".join(f"{_txt(a)} {_txt(b)}" for a, b in zip(v, w)) for v, w, tau in cases]
    r = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True)
    out = r.stdout.splitlines()
    assert r.returncode == 0 and out and out[-1] == "ok", r.stdout[-2000:] + r.stderr
    got = [k.split()[1:] for k in out if k.startswith("p ")]
    assert len(got) == len(cases)
    return [(int(k[0]), TF(float.fromhex(k[1])), TF(float.fromhex(k[2])), int(k[3]), np.array([float.fromhex(x) for x in k[4:]]).astype(TF))
            for k in got]


@pytest.mark.parametrize("TF", [np.float32, np.float64])
def test_header_equals_the_emulation_bit_for_bit(driver, TF):
    cases = _cases(TF)
    got = _run(driver, TF, cases)
    most = 0
    for (v, w, tau), (need, theta, asum, passes, y) in zip(cases, got):
        e_need, e_theta, e_asum, e_passes, e_y = R.emulate_project(v, w, tau)
        assert (need, passes) == (e_need, e_passes), (len(v), need, passes, e_need, e_passes)
        assert l1_exact.same_bits(np.array([theta, asum]), np.array([e_theta, e_asum])), (len(v), theta, e_theta, asum, e_asum)
        assert l1_exact.same_bits(y, e_y), len(v)
        if not need:
            assert l1_exact.same_bits(y, v), "an input inside the ball was written"
        most = max(most, passes)
    assert 2 <= most <= 14, most
    # inside; all weights zero; -1 / NaN / inf weights; the tie on magnitudes; the tie of the issue
    assert [k[0] for k in got[-5:]] == [0, 0, 1, 1, 1] and got[-4][1] == 0 and got[-4][3] == 1
    v, bad, tau = cases[-3]
    again = _run(driver, TF, [(v, R.clean(bad), tau)])[0]
    assert got[-3][:4] == again[:4] and l1_exact.same_bits(got[-3][4], again[4]), "bad weights count as 0"
    assert l1_exact.same_bits(got[-3][4][[3, 7, 11]], v[[3, 7, 11]])
    # the tie: theta = 2.5; (5, 2) -> +-0, (7, 2) -> +-2, (7, 1) -> +-4.5, the 0 entry keeps its bits
    v, w, tau = cases[-1]
    assert float(got[-1][1]) == 2.5
    want = (np.array([0, 2, 4.5, 0, 2, 4.5, 0, 0], TF) * np.array(TIE_SIGN, TF)).astype(TF)
    assert l1_exact.same_bits(got[-1][4], want) and np.signbit(got[-1][4][6]) and np.array_equal(np.signbit(got[-1][4]), np.signbit(v))


@pytest.mark.parametrize("TF", [np.float32, np.float64])
def test_non_finite_entries_of_weight_zero_reach_nothing(driver, TF):
    """inf and NaN in v where the weight is 0 (what a pad may hold): theta, asum, the decision and every other entry are exactly those
    of the same input with finite values there; the entries themselves are not written."""
    rng = np.random.default_rng(53)
    L = 200
    v = _heavy(rng, L).astype(TF)
    w = weights("lognormal", rng, L, TF)
    at = np.array([0, 17, 18, 99, 199])
    w[at] = 0
    w[150] = np.nan                                   # (a bad weight is a zero weight)
    tau = TF(0.2 * R.norm(v, R.clean(w)))
    vb = v.copy()
    vb[at] = [np.inf, np.nan, -np.inf, np.nan, np.inf]
    vb[150] = np.nan
    clean_run, bad_run = _run(driver, TF, [(v, w, tau), (vb, w, tau)])
    assert clean_run[0] == bad_run[0] == 1
    assert l1_exact.same_bits(np.array(clean_run[1:3]), np.array(bad_run[1:3])), "theta or asum moved"
    rest = np.setdiff1d(np.arange(L), np.append(at, 150))
    assert l1_exact.same_bits(clean_run[4][rest], bad_run[4][rest])
    assert np.array_equal(np.isnan(bad_run[4]), np.isnan(vb)) and np.array_equal(bad_run[4][[0, 18, 199]], vb[[0, 18, 199]])
    e = R.emulate_project(v, w, tau)
    assert l1_exact.same_bits(np.array(clean_run[1:3]), np.array(e[1:3])) and l1_exact.same_bits(clean_run[4], e[4])


@pytest.mark.parametrize("TF", [np.float32, np.float64])
def test_michelot_reaches_the_exact_threshold(driver, TF):
    """theta of the header against theta*.  Float64: the sums are exact to twice the working precision, S - tau, the quotient and its
    one correction round to within 2^-52 theta* (which adds n 2^-64 for the running sums of its reference); Float32: half
    an ulp of the one rounding to T on top."""
    cases = [c for c in _cases(TF)[:-5] if len(c[0]) > 40 or len(c[0]) == 12]
    got = _run(driver, TF, cases)
    worst = 0.0
    for (v, w, tau), (need, theta, _, _, _) in zip(cases, got):
        th = float(R.theta_star(np.abs(v), w, tau))
        assert need == 1 and th > 0
        tol = (2.0 ** -52 + len(v) * 2.0 ** -64) * th + (0.5 * l1_exact.ulp(th, TF) if TF == np.float32 else 0.0)
        worst = max(worst, abs(float(theta) - th) / tol)
        assert abs(float(theta) - th) <= tol, (len(v), float(theta), th)
    print(f"worst |theta - theta*| / tol = {worst:.3f}")


@pytest.mark.parametrize("TF", [np.float32, np.float64])
def test_header_shrink_equals_the_emulation_bit_for_bit(driver, TF):
    rng = np.random.default_rng(43)
    K = 2000
    v = _heavy(rng, K).astype(TF)
    w = weights("lognormal", rng, K, TF)
    w[:300] = weights("masked", rng, 300, TF)
    theta = (np.abs(rng.standard_normal(K)) * 0.7).astype(TF)
    v[320:340] = -0.0
    v[340:360] = 0.0
    v[400:406], w[400:406], theta[400:406] = [5, -5, 7, -7, 7, -7], [2, 2, 2, 2, 1, 1], 2.5
    tag = "f" if TF == np.float32 else "d"
    lines = [f"a {tag} {_txt(x)} {_txt(b)} {_txt(t)}" for x, b, t in zip(v, w, theta)]
    r = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True)
    out = r.stdout.splitlines()
    assert r.returncode == 0 and out[-1] == "ok", r.stdout[-2000:] + r.stderr
    got = np.array([float.fromhex(k.split()[1]) for k in out if k.startswith("a ")]).astype(TF)
    want = np.concatenate([R.emulate_apply(v[k:k + 1], w[k:k + 1], theta[k]) for k in range(K)])
    assert l1_exact.same_bits(got, want)
    assert l1_exact.same_bits(got[400:406], np.array([0.0, -0.0, 2, -2, 4.5, -4.5], TF))
    assert l1_exact.same_bits(got[:300][w[:300] == 0], v[:300][w[:300] == 0]), "weight 0: not touched"
    assert np.array_equal(np.signbit(got), np.signbit(v))


# ---- host side ---------------------------------------------------------------------------------------------------------------------------
def test_setup_constraints_carries_the_weights(sipx):
    g3 = sipx.compgrid((25.0, 25.0, 25.0), (16, 12, 8))
    g2 = sipx.compgrid((25.0, 6.0), (16, 12))
    assert sipx.host.PROJ["l1_weighted"] == 18
    for TF in (np.float32, np.float64):
        for op, g, mode, n in (("TV", g3, ("tensor", ""), (16, 12, 8)), ("TV", g2, ("matrix", ""), (16, 12)), ("D2D", g2, ("matrix", ""), (16, 12)),
                               ("TV_xy", g3, ("tensor", ""), (16, 12, 8)), ("identity", g2, ("matrix", ""), (16, 12)),
                               ("D_x", g3, ("tensor", ""), (16, 12, 8)), ("D_y", g3, ("tensor", ""), (16, 12, 8)), ("D_z", g2, ("matrix", ""), (16, 12))):
            rows = R.rows(n, op)
            w = np.linspace(0.0, 2.0, rows)                       # float64: setup_constraints takes it to the working precision
            c = [sipx.set_definitions("bounds", "identity", 1.0, 2.0, mode), sipx.set_definitions("l1_weighted", op, 0.0, 3.5, mode, weights=w)]
            P, A, prop = sipx.setup_constraints(copy.deepcopy(c), g, TF)
            assert A[1].shape[0] == rows
            assert P[1].weighted and P[1].lb.dtype == TF and P[1].ub is None and np.array_equal(P[1].lb, w.astype(TF))
            assert P[1].data_len(A[1]) == rows and P[0].data_len(A[0]) is None
            assert prop.tag[1] == ("l1_weighted", op, mode[0], "") and prop.ncvx[1] is False
            d = P[1].desc(A[1].kind, prop.ncvx[1])
            assert (d.proj, d.mode, d.pmax, d.reserved, d.transform) == (18, 0, 3.5, rows, 0) and d.lb is not None and d.ub is None
            # the automatic context caches refuse lists with array arguments
            opt = sipx.PARSDMM_options()
            opt.FL = TF
            assert sipx.host._context_key(np.zeros(1, TF), None, A, prop, P, g, opt, None) is None


def test_host_refusals(sipx):
    TF = np.float32
    n = (16, 12, 8)
    g3 = sipx.compgrid((25.0, 25.0, 25.0), n)
    g2 = sipx.compgrid((25.0, 6.0), (16, 12))
    M = R.rows(n, "TV")
    w = np.ones(M, TF)

    def P(op, mode, weights, g=g3, mx=1.0, st="l1_weighted", cust=((), False)):
        return sipx.Projector(sipx.set_definitions(st, op, 0.0, mx, mode, cust, weights), g, TF)
    # the plain set still takes no weights, in the words it always had
    with pytest.raises(sipx.SipxError, match="set type 'l1' takes no weights: weights belong to the l2,1 sets"):
        P("TV", ("tensor", ""), w, st="l1")
    with pytest.raises(sipx.SipxError, match=r"needs weights, one per row of the operator: without weights the set is the plain \(\"l1\", op\)"):
        P("TV", ("tensor", ""), None)
    for mode in (("fiber", "x"), ("slice", "z")):
        for op in ("TV", "D_x", "identity"):
            with pytest.raises(sipx.SipxError, match=r"applies to the whole array \(matrix / tensor mode\): per fiber or slice use "
                                                     r"\(\"l1\", op, mode\) with segment_norms=True"):
                P(op, mode, w)
    for op in ("DFT", "DCT", "wavelet"):
        with pytest.raises(sipx.SipxError, match=r"takes no transform \(DFT, DCT, wavelet\).*use the plain \(\"l1\", transform\)"):
            P(op, ("tensor", ""), w)
    import scipy.sparse as sp
    with pytest.raises(sipx.SipxError, match=r"takes no custom operator.*use the plain \(\"l1\", op\)"):
        P("identity", ("tensor", ""), w, cust=(sp.identity(1536, format="csc"), False))
    with pytest.raises(sipx.SipxError, match="takes no custom operator"):
        P("D_xz", ("matrix", ""), w, g=g2)
    with pytest.raises(sipx.SipxError, match="unknown transform domain operator"):
        P("D_q", ("tensor", ""), w)
    with pytest.raises(sipx.SipxError, match="TV_xy is the in-plane gradient of a 3-D grid"):
        P("TV_xy", ("matrix", ""), w, g=g2)
    with pytest.raises(sipx.SipxError, match="unknown transform domain operator"):
        P("D_y", ("matrix", ""), w, g=g2)
    with pytest.raises(sipx.SipxError, match=rf"l1_weighted weights have shape \({M - 1},\): \({M},\) is needed -- one per row of TV, in the order of A @ x"):
        P("TV", ("tensor", ""), w[:-1])
    with pytest.raises(sipx.SipxError, match=rf"l1_weighted weights have shape \({M},\): \(1536,\) is needed -- one per row of identity"):
        P("identity", ("tensor", ""), w)
    with pytest.raises(sipx.SipxError, match="l1_weighted weights have dtype float64: not the working precision"):
        P("TV", ("tensor", ""), w.astype(np.float64))
    with pytest.raises(sipx.SipxError, match="l1_weighted weights must be a numpy array, not list"):
        P("TV", ("tensor", ""), list(w))
    for bad, at in ((-1.0, 5), (np.nan, 0), (np.inf, 77), (-np.inf, 1400)):
        wb = w.copy()
        wb[at] = wb[4000] = bad             # the message names the first offender
        with pytest.raises(sipx.SipxError, match=rf"the weighted l1 ball \(l1_weighted\): weight {at} is negative, NaN or infinite"):
            P("TV", ("tensor", ""), wb)
    assert P("TV", ("tensor", ""), np.zeros(M, TF)).weighted, "all weights zero is a set"
    for mx in (0.0, -1.0, float("nan")):
        with pytest.raises(sipx.SipxError, match="Radius of L1 ball is negative"):
            P("TV", ("tensor", ""), w, mx=mx)
    with pytest.raises(sipx.SipxError, match="takes one radius"):
        P("TV", ("tensor", ""), w, mx=np.ones(3))
    # the operator a list pairs the set with
    Pw = P("TV", ("tensor", ""), w)
    with pytest.raises(sipx.SipxError, match="one weight per row of TV, the operator is D_z"):
        Pw.check_rows(sipx.TDOperator("D_z", g3, TF))
    with pytest.raises(sipx.SipxError, match="takes no Minkowski component"):
        Pw.check_rows(sipx.TDOperator("TV", g3, TF, component=1))
    Pw.check_rows(sipx.TDOperator("D3D", g3, TF))
    with pytest.raises(sipx.SipxError, match=f"projects a vector of the TV range: {M} entries on this grid, 7 given"):
        Pw(np.zeros(7, TF))
    # the observer
    x = np.zeros(1536, TF)
    with pytest.raises(sipx.SipxError, match=f"weights has {M - 1} entries, {M} are needed"):
        sipx.l1_weighted_norm(x, g3, "TV", w[:-1])
    wb = w.copy()
    wb[9] = -0.5
    with pytest.raises(sipx.SipxError, match=r"the weighted l1 ball \(l1_weighted\): weight 9 is negative, NaN or infinite"):
        sipx.l1_weighted_norm(x, g3, "TV", wb)
    with pytest.raises(sipx.SipxError, match="takes no transform"):
        sipx.l1_weighted_norm(x, g3, "DCT", w)
    with pytest.raises(sipx.SipxError, match="needs weights"):
        sipx.l1_weighted_norm(x, g3, "TV", None)
    with pytest.raises(sipx.SipxError, match="x must be a Float32 or Float64"):
        sipx.l1_weighted_norm(list(x), g3, "TV", w)
    for s in ("sipx_l1_weighted_norm", "sipx_l1_weighted_norm_dev"):
        assert s in sipx.EXPORTED_SYMBOLS


def test_the_constant_is_declared_everywhere():
    head = open(os.path.join(ROOT, "include", "sipx.h")).read()
    assert "SIPX_PROJ_L1_WEIGHTED = 18" in head
    assert "EXT_L1_WEIGHTED = 19" in open(os.path.join(CSRC, "ext_proj.h")).read()
    assert "SIPX_PROJ_L1_WEIGHTED = 18" in open(os.path.join(ROOT, "julia", "SipxPARSDMM.jl")).read()
    # the refusals are worded beside the rule, none as a literal of set_config.h
    assert 'runtime_error("the weighted l1' not in open(os.path.join(CSRC, "set_config.h")).read()
    assert 'L1W_NO_MODE = "the weighted l1 ball' in open(os.path.join(CSRC, "l1_weighted.h")).read()


def test_constraint2coarse_refuses_the_set(sipx):
    g = sipx.compgrid((1.0, 1.0), (64, 48))
    plain = [sipx.set_definitions("l1", "TV", 0.0, 12.0, ("matrix", ""))]
    assert sipx.constraint2coarse(copy.deepcopy(plain), g, 2)[0].max == 3.0
    c = [sipx.set_definitions("l1_weighted", "TV", 0.0, 12.0, ("matrix", ""), weights=np.ones(R.rows((64, 48), "TV"), np.float32))]
    with pytest.raises(sipx.SipxError, match="multilevel: the weighted l1 ball .l1_weighted. has no rule that takes its weights to a coarser grid"):
        sipx.constraint2coarse(c, g, 2)
