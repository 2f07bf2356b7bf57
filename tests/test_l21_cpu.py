"""Isotropic total variation without a GPU: the numpy reference (tests/l21_ref.py) against the oracle's TV operator and against the
properties of a projection, csrc/l21.h on the CPU (tests/l21/rule_driver.cpp, compiled by hipcc; the program makes no HIP call)
against a numpy emulation of the contract bit for bit, the host descriptors and refusals, and the multilevel scaling."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import parsdmm_oracle as O
from tests import l1_exact, l21_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "setintersectionprojection.jl_amd", "csrc")


# ---- the groups ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,h", [((7, 5), (25.0, 6.0)), ((6, 4, 3), (25.0, 10.0, 6.0))])
def test_groups_agree_with_the_oracle_operator(n, h):
    TF = np.float64
    x = np.random.default_rng(3).standard_normal(n)
    TV = O.get_TD_operator(O.compgrid(h, n), "TV", TF)[0]
    v = np.asarray(TV @ x.reshape(-1, order="F"), TF)
    G = l21_ref.groups(n)
    assert v.shape == (l21_ref.rows(n),) and G.shape == (x.size, len(n))
    used = G[G >= 0]
    assert sorted(used) == list(range(len(v))), "every row of the operator belongs to exactly one group"
    far = np.zeros(x.size, int)
    coords = np.unravel_index(np.arange(x.size), n, order="F")
    for q, d in enumerate(l21_ref.block_dirs(n)):
        diff = (np.diff(x, axis=d) / h[d])                       # forward difference that starts at the point, along d
        pad = [(0, 0)] * len(n)
        pad[d] = (0, 1)
        diff = np.pad(diff, pad, constant_values=np.nan).reshape(-1, order="F")
        has = G[:, q] >= 0
        assert np.array_equal(has, coords[d] < n[d] - 1)
        assert np.allclose(v[G[has, q]], diff[has], rtol=1e-12, atol=1e-12)
        far += ~has
    assert np.array_equal((G >= 0).sum(axis=1), len(n) - far)   # members: ndim minus the coordinates on the far face
    assert (G[-1] < 0).all(), "the last corner has no member"


# ---- the reference is a projection -------------------------------------------------------------------------------------------------------
def _heavy(rng, M):
    return rng.standard_normal(M) * np.exp(rng.standard_normal(M))


@pytest.mark.parametrize("n", [(7, 5), (6, 4, 3), (33, 20)])
@pytest.mark.parametrize("frac", [0.9, 0.5, 0.05])
def test_reference_is_the_projection(n, frac):
    TF = np.float64
    eps = float(np.finfo(TF).eps)
    rng = np.random.default_rng(11 + sum(n))
    M = l21_ref.rows(n)
    v = _heavy(rng, M).astype(TF)
    b = TF(frac * l21_ref.norm21(v, n))
    y = l21_ref.project(v, n, b)
    assert y is not v
    assert l21_ref.norm21(y, n) <= float(b) * (1 + 4 * eps)
    assert l21_ref.norm21(y, n) >= float(b) * (1 - 4 * eps), "an infeasible point projects onto the boundary"
    # <v - y, z - y> <= 0 for every z of the ball.  y carries a relative error of a few eps per entry (theta: l1_exact.theta_tol, the
    # weights: three roundings), so the inner product is off by at most that times sum |v - y| |z - y| <= ||v - y|| ||z - y||
    for k in range(200):
        z = _heavy(rng, M)
        if k % 4 == 0:
            z[rng.random(M) < 0.7] = 0.0
        z *= (1.0 if k % 5 == 0 else rng.random()) * float(b) * (1 - 8 * eps) / l21_ref.norm21(z, n)
        vi = float(np.dot(v - y, z - y))
        assert vi <= 64 * eps * np.linalg.norm(v - y) * np.linalg.norm(z - y), (k, vi)
    # theta against a float64 bisection of sum(max(g - theta, 0)) = b
    g = l21_ref.norms(v, n, TF).astype(np.float64)
    th, C, S = l1_exact.exact_theta(g, b)
    lo, hi = 0.0, float(g.max())
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if np.maximum(g - mid, 0).sum() > float(b) else (lo, mid)
    assert abs(0.5 * (lo + hi) - th) <= l1_exact.theta_tol(C, S, b, th, TF) + (hi - lo) + 4 * eps * g.sum() / C


def test_reference_returns_a_feasible_input_itself():
    n = (6, 4, 3)
    v = _heavy(np.random.default_rng(5), l21_ref.rows(n)).astype(np.float32)
    assert l21_ref.project(v, n, np.float32(2 * l21_ref.norm21(v, n))) is v


# ---- csrc/l21.h on the CPU -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    hipcc = shutil.which("hipcc") or shutil.which("hipcc", path=os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin"))
    assert hipcc, "hipcc not found"
    exe = str(tmp_path_factory.mktemp("l21") / "rule_driver")
    r = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                        "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "l21", "rule_driver.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def emulate(v, mask, theta):
    """The contract of csrc/l21.h in numpy, in v's precision: (g, f, y) of the groups v[k, :] with members mask[k, :]."""
    TF = v.dtype.type
    ss = np.zeros(len(v), np.float64)
    for q in range(3):
        t = v[:, q].astype(np.float64)
        ss = ss + np.where(mask[:, q], t * t, 0.0)
    g = np.sqrt(ss).astype(TF)
    t = (g - theta.astype(TF)).astype(TF)
    t = np.where(t > 0, t, TF(0)).astype(TF)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(g > 0, (t / g).astype(TF), TF(0)).astype(TF)
    y = np.where(mask, (v * f[:, None]).astype(TF), v).astype(TF)
    return g, f, y


def _rule_inputs(TF):
    rng = np.random.default_rng(17)
    K = 3000
    v = (rng.standard_normal((K, 3)) * np.exp(rng.standard_normal((K, 3)))).astype(TF)
    mask = rng.random((K, 3)) < 0.8
    mask[:200] = np.eye(3, dtype=bool)[rng.integers(0, 3, 200)]          # one-member groups
    mask[200:230] = False                                                 # the last corner: no member
    v[300:400][rng.random((100, 3)) < 0.5] = 0.0
    v[400:500][rng.random((100, 3)) < 0.5] = -0.0
    v[500:520] = 0.0
    v[520:540] = -0.0
    theta = (np.abs(rng.standard_normal(K)) * 1.5).astype(TF)
    theta[600:650] = 0.0
    # the tie values of the GPU test: norms 7, 5 and 1 against theta = 5
    ties = np.array([(7, 0, 0), (0, 7, 0), (0, 0, 7), (3, 4, 0), (5, 0, 0), (0, 3, 4), (-3, 0, 4), (0, -5, 0), (1, 0, 0), (0, 0, -1)], TF)
    v[700:700 + len(ties)] = ties
    mask[700:700 + len(ties)] = True
    theta[700:700 + len(ties)] = 5.0
    return v, mask, theta


@pytest.mark.parametrize("TF", [np.float32, np.float64])
def test_header_rule_equals_the_emulation_bit_for_bit(driver, TF):
    v, mask, theta = _rule_inputs(TF)
    tag = "f" if TF == np.float32 else "d"
    lines = [f"{tag} {int(m[0]) + 2 * int(m[1]) + 4 * int(m[2])} " + " ".join(float(x).hex() for x in row) + " " + float(t).hex()
             for row, m, t in zip(v, mask, theta)]
    r = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True)
    out = r.stdout.splitlines()
    assert r.returncode == 0 and out and out[-1] == "ok", "\n".join(k for k in out if k.startswith("FAIL"))[:4000] + r.stderr
    got = np.array([[float.fromhex(w) for w in k.split()[1:]] for k in out if k.startswith("g ")])
    assert got.shape == (len(v), 5)
    g, f, y = emulate(v, mask, theta)
    assert l1_exact.same_bits(got[:, 0].astype(TF), g)
    assert l1_exact.same_bits(got[:, 1].astype(TF), f)
    assert l1_exact.same_bits(np.ascontiguousarray(got[:, 2:]).astype(TF), y)
    # the ties: exact norms, groups on the threshold are zeroed, members keep the sign of zero
    assert list(g[700:710]) == [7, 7, 7, 5, 5, 5, 5, 5, 1, 1]
    assert np.all(f[703:710] == 0) and np.all(f[700:703] == TF(TF(2) / TF(7)))
    assert np.any(np.signbit(y[400:540]) & (y[400:540] == 0)), "-0.0 members stay -0.0"
    assert np.all(g[200:230] == 0) and l1_exact.same_bits(y[200:230], v[200:230]), "a group without members is not written"


def test_float64_threshold_is_correctly_rounded(driver):
    """l21_theta_refined on the active set of a plain float64 evaluation of theta: within 2^-52 theta* of the exact fixed point (the sum
    is exact to twice the precision; one rounding for S - tau, one for the division), where the plain evaluation is ulps of S / C off."""
    rng = np.random.default_rng(23)
    cases = []
    for L, frac in ((60, 0.9), (60, 0.5), (660, 0.9), (660, 0.05), (5000, 0.97), (5000, 0.5), (12, 0.9)):
        g = np.abs(rng.standard_normal(L) * np.exp(rng.standard_normal(L)))
        g[-1] = 0.0                                             # the last corner of a grid
        b = frac * float(g.sum())
        th, C, S = l1_exact.exact_theta(g, b)
        act = g[g > th]
        plain = (float(np.sum(act[::-1])) - b) / len(act)       # what a float64 evaluation may return
        cases.append((g, b, th, plain))
    cases.append((np.array([7.0, 5, 7, 1, 5, 7, 5, 1, 7, 0]), 8.0, 5.0, 5.0))      # the ties of the GPU test
    lines = [f"theta {float(b).hex()} {float(p).hex()} {len(g)} " + " ".join(float(x).hex() for x in g) for g, b, _, p in cases]
    r = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True)
    out = r.stdout.splitlines()
    assert r.returncode == 0 and out[-1] == "ok", r.stdout[-2000:] + r.stderr
    got = [float.fromhex(k.split()[1]) for k in out if k.startswith("theta ")]
    assert len(got) == len(cases)
    worse = 0
    for (g, b, th, plain), t in zip(cases, got):
        assert abs(t - th) <= 2.0 ** -52 * th, (len(g), t, th, plain)
        worse += abs(plain - th) > 2.0 ** -52 * th
    assert got[-1] == 5.0
    assert worse >= 2, "no case in which the plain evaluation is off: the inputs show nothing"


# ---- host side -------------------------------------------------------------------------------------------------------------------------
def test_setup_constraints_takes_the_set(sipx):
    TF = np.float32
    for n, h, op in (((16, 12), (25.0, 6.0), "TV"), ((16, 12, 8), (25.0, 25.0, 25.0), "TV"), ((16, 12), (1.0, 1.0), "D2D"),
                     ((16, 12, 8), (1.0, 1.0, 1.0), "D3D")):
        g = sipx.compgrid(h, n)
        mode = ("matrix", "") if len(n) == 2 else ("tensor", "")
        c = [sipx.set_definitions("bounds", "identity", 1.0, 2.0, mode), sipx.set_definitions("l21", op, 0.0, 3.5, mode)]
        P, A, prop = sipx.setup_constraints(c, g, TF)
        assert prop.tag[1] == ("l21", op, mode[0], "") and prop.ncvx == [False, False]
        ref = sipx.setup_constraints([sipx.set_definitions("l1", op, 0.0, 3.5, mode)], g, TF)
        assert prop.TD_n[1] == ref[2].TD_n[0] and A[1].shape == ref[1][0].shape == (l21_ref.rows(n), int(np.prod(n)))
        assert (P[1].kind, P[1].mode, P[1].pmax, P[1].transform, P[1].seg_radii) == ("l21", 0, 3.5, 0, False)
        d = P[1].desc(A[1].kind, prop.ncvx[1])
        assert (d.op, d.proj, d.pmin, d.pmax, d.mode, d.transform, d.ncvx) == (4, 14, 0.0, 3.5, 0, 0, 0)
        assert d.lb is None and d.ub is None
        P[1].check_rows(A[1])
        assert P[1].data_len(A[1]) is None
    assert sipx.host.PROJ["l21"] == 14 and "sipx_l21_norm" in sipx.EXPORTED_SYMBOLS and "sipx_l21_norm_dev" in sipx.EXPORTED_SYMBOLS
    assert callable(sipx.l21_norm)


def test_host_refusals(sipx):
    TF = np.float32
    g3 = sipx.compgrid((25.0, 25.0, 25.0), (16, 12, 8))
    g2 = sipx.compgrid((25.0, 6.0), (16, 12))

    def setup(op, mx, mode, g, custom=((), False)):
        return sipx.setup_constraints([sipx.set_definitions("l21", op, 0.0, mx, mode, custom)], g, TF)
    for op in ("identity", "D_x", "D_z", "DFT", "DCT", "wavelet", "curvelet"):
        with pytest.raises(sipx.SipxError, match="the l2,1 ball acts on the range of the TV operator: TD_OP must be TV"):
            setup(op, 1.0, ("tensor", ""), g3)
    for mode in (("fiber", "x"), ("slice", "z")):
        with pytest.raises(sipx.SipxError, match="the l2,1 ball applies to the whole array"):
            setup("TV", 1.0, mode, g3)
    with pytest.raises(sipx.SipxError, match="the l2,1 ball applies to the whole array"):
        setup("TV", 1.0, ("fiber", "z"), g2)
    for mx in (0.0, -1.0, float("nan")):
        with pytest.raises(sipx.SipxError, match="Radius of L1 ball is negative"):
            setup("TV", mx, ("matrix", ""), g2)
    import scipy.sparse as sp
    with pytest.raises(sipx.SipxError, match="TD_OP must be TV"):
        setup("TV", 1.0, ("matrix", ""), g2, (sp.identity(16 * 12, format="csc"), False))
    # a descriptor never reaches an operator it was not made for
    P = sipx.Projector(sipx.set_definitions("l21", "TV", 0.0, 1.0, ("matrix", "")), g2, TF)
    for kind in ("identity", "D_x"):
        with pytest.raises(sipx.SipxError, match="TD_OP must be TV"):
            P.check_rows(sipx.TDOperator(kind, g2, TF))
    with pytest.raises(sipx.SipxError, match="TD_OP must be TV"):
        sipx.l21_norm(np.zeros(16 * 12, TF), g2, "D_x")
    with pytest.raises(sipx.SipxError, match="TV range: 356 entries on this grid, 192 given"):
        P(np.zeros(16 * 12, TF))


def test_constraint2coarse_scales_like_l1(sipx):
    for n, div in (((64, 48), 4.0), ((64, 48, 1), 4.0), ((32, 24, 16), 8.0)):
        g = sipx.compgrid(tuple(1.0 for _ in n), n)
        c = [sipx.set_definitions("l21", "TV", 0.0, 12.0, ("matrix", "")), sipx.set_definitions("l1", "TV", 0.0, 12.0, ("matrix", ""))]
        out = sipx.constraint2coarse(c, g, 2)
        assert out[0].max == out[1].max == 12.0 / div
