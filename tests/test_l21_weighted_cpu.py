"""The weighted l2,1 ball without a GPU: the numpy reference (tests/l21_weighted_ref.py) against the properties of a projection,
csrc/l21_weighted.h on the CPU (tests/l21_weighted/rule_driver.cpp, compiled by hipcc; the program makes no HIP call) against a Python
emulation of the contract bit for bit and against the exact threshold, the host descriptors and refusals, and the multilevel refusal."""
import copy
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import l1_exact, l21_ref
from tests import l21_weighted_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "setintersectionprojection.jl_amd", "csrc")
FAMILIES = ("ones", "edge", "masked", "lognormal")


def _heavy(rng, M):
    return rng.standard_normal(M) * np.exp(rng.standard_normal(M))


def weights(family, rng, n, TF):
    """The four families of the issue: flat, 1 / (1 + |heavy-tailed|), 30 % zeros with the rest in [0.5, 2], exp(3 randn)."""
    if family == "ones":
        return np.ones(n, TF)
    if family == "edge":
        return (1.0 / (1.0 + np.abs(_heavy(rng, n)))).astype(TF)
    if family == "masked":
        w = rng.uniform(0.5, 2.0, n)
        w[rng.random(n) < 0.3] = 0.0
        return w.astype(TF)
    return np.exp(3.0 * rng.standard_normal(n)).astype(TF)


# ---- the reference is a projection -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,kind", [((7, 5), "TV"), ((6, 4, 3), "TV"), ((6, 4, 3), "TV_xy"), ((6, 5, 4), "joint")])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("frac", [0.9, 0.5, 0.05])
def test_reference_is_the_projection(n, kind, family, frac):
    TF = np.float64
    eps = float(np.finfo(TF).eps)
    rng = np.random.default_rng(31 + sum(n) + len(family))
    M = R.rows(n, kind)
    v = _heavy(rng, M).astype(TF)
    w = weights(family, rng, R.ngroups(n, kind), TF)
    b = TF(frac * R.norm(v, n, kind, w))
    y = R.project(v, n, kind, w, b)
    assert y is not v
    # the boundary is attained: a few eps per group norm, weighted
    assert abs(R.norm(y, n, kind, w) - float(b)) <= 8 * eps * float(b)
    # <v - y, z - y> <= 0 for every z of the ball, up to the rounding of y (tests/test_l21_cpu.py)
    for k in range(100):
        z = _heavy(rng, M)
        if k % 4 == 0:
            z[rng.random(M) < 0.7] = 0.0
        nz = R.norm(z, n, kind, w)
        if nz > 0:
            z *= (1.0 if k % 5 == 0 else rng.random()) * float(b) * (1 - 8 * eps) / nz
        vi = float(np.dot(v - y, z - y))
        assert vi <= 64 * eps * np.linalg.norm(v - y) * np.linalg.norm(z - y), (k, vi)
    # groups of weight 0 are not touched
    G = R.members(n, kind)
    idx = G[np.asarray(w) == 0]
    idx = idx[idx >= 0]
    assert np.array_equal(y[idx], v[idx])


def test_reference_all_ones_is_the_unweighted_reference():
    n = (7, 5)
    v = _heavy(np.random.default_rng(2), l21_ref.rows(n)).astype(np.float64)
    b = np.float64(0.4 * l21_ref.norm21(v, n))
    assert np.allclose(R.project(v, n, "TV", np.ones(35), b), l21_ref.project(v, n, b), rtol=1e-13, atol=0)


def test_reference_returns_a_feasible_input_itself():
    n = (6, 4, 3)
    v = _heavy(np.random.default_rng(5), R.rows(n, "TV")).astype(np.float32)
    w = weights("edge", np.random.default_rng(6), 72, np.float32)
    assert R.project(v, n, "TV", w, np.float32(2 * R.norm(v, n, "TV", w))) is v
    assert R.project(v, n, "TV", np.zeros(72, np.float32), np.float32(1e-3)) is v, "all weights zero: every v is inside"


# ---- csrc/l21_weighted.h on the CPU ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    hipcc = shutil.which("hipcc") or shutil.which("hipcc", path=os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin"))
    assert hipcc, "hipcc not found"
    exe = str(tmp_path_factory.mktemp("l21_weighted") / "rule_driver")
    r = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                        "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "l21_weighted", "rule_driver.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _hex(x):
    return float(x).hex()


def _search_cases(TF):
    rng = np.random.default_rng(41)
    out = []
    for L in (12, 60, 660, 2500):
        for family in FAMILIES:
            for frac in (0.9, 0.5, 0.05):
                g = np.abs(_heavy(rng, L)).astype(TF)
                g[-1] = 0.0                                         # the last corner of a grid
                w = weights(family, rng, L, TF)
                tau = TF(frac * float(np.sum(w.astype(np.float64) * g.astype(np.float64))))
                out.append((g, w, tau))
    g = np.abs(_heavy(rng, 40)).astype(TF)
    out.append((g, np.ones(40, TF), TF(2 * g.sum())))               # inside
    out.append((g, np.zeros(40, TF), TF(1e-3)))                      # all weights zero
    bad = np.ones(40, TF)
    bad[[3, 7, 11]] = [-1.0, np.nan, np.inf]                         # what only device memory can bring: counted as 0
    out.append((g, bad, TF(0.3 * g.sum())))
    # the ties of the GPU test: theta = 2.5 exactly
    gt = np.array([5, 7, 7, 5, 7, 7, 0, 5], TF)
    wt = np.array([2, 2, 1, 2, 2, 1, 1, 2], TF)
    out.append((gt, wt, TF(17)))        # active: the four groups of norm 7, S = 42, C = 10, tau = S - 2.5 C
    return out


def _run_search(driver, TF, cases):
    tag = "f" if TF == np.float32 else "d"
    lines = [f"s {tag} {_hex(tau)} {len(g)} " + " ".join(f"{_hex(a)} {_hex(b)}" if np.isfinite(b) else f"{_hex(a)} {str(float(b))}"
                                                         for a, b in zip(g, w)) for g, w, tau in cases]
    r = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True)
    out = r.stdout.splitlines()
    assert r.returncode == 0 and out and out[-1] == "ok", r.stdout[-2000:] + r.stderr
    got = [k.split()[1:] for k in out if k.startswith("s ")]
    assert len(got) == len(cases)
    return [(int(a), TF(float.fromhex(b)), TF(float.fromhex(c)), int(d)) for a, b, c, d in got]


@pytest.mark.parametrize("TF", [np.float32, np.float64])
def test_header_search_equals_the_emulation_bit_for_bit(driver, TF):
    cases = _search_cases(TF)
    got = _run_search(driver, TF, cases)
    most = 0
    for (g, w, tau), (need, theta, asum, passes) in zip(cases, got):
        e_need, e_theta, e_asum, e_passes = R.emulate_search(g, w, tau)
        assert (need, passes) == (e_need, e_passes), (len(g), need, passes, e_need, e_passes)
        assert l1_exact.same_bits(np.array([theta, asum]), np.array([e_theta, e_asum])), (len(g), theta, e_theta, asum, e_asum)
        most = max(most, passes)
    assert 2 <= most <= 14, most
    assert [k[0] for k in got[-4:]] == [0, 0, 1, 1] and got[-3][1] == 0 and got[-3][3] == 1
    assert float(got[-1][1]) == 2.5, "the ties: theta is 2.5 exactly"
    # bad weights count as 0: the same search as with zeros in their place
    g, bad, tau = cases[-2]
    assert got[-2] == _run_search(driver, TF, [(g, R.clean(bad), tau)])[0]


@pytest.mark.parametrize("TF", [np.float32, np.float64])
def test_michelot_reaches_the_exact_threshold(driver, TF):
    """theta of the header against the sort-based threshold in extended precision.  Float64: the sums are exact to twice the working
    precision, S - tau, the quotient and its one correction round to within 2^-52 theta*; the reference's own cumulative sums add up
    to n 2^-64 relative.  Float32: half an ulp of the one rounding to T on top."""
    cases = [c for c in _search_cases(TF) if len(c[0]) > 40 or len(c[0]) == 12]
    got = _run_search(driver, TF, cases)
    worst = 0.0
    for (g, w, tau), (need, theta, _, _) in zip(cases, got):
        th = R.exact_theta(g, w, tau)
        assert need == 1 and th > 0
        tol = (2.0 ** -52 + len(g) * 2.0 ** -64) * th + (0.5 * l1_exact.ulp(th, TF) if TF == np.float32 else 0.0)
        worst = max(worst, abs(float(theta) - th) / tol)
        assert abs(float(theta) - th) <= tol, (len(g), float(theta), th)
    print(f"worst |theta - theta*| / tol = {worst:.3f}")


@pytest.mark.parametrize("TF", [np.float32, np.float64])
def test_header_factor_equals_the_emulation_bit_for_bit(driver, TF):
    rng = np.random.default_rng(43)
    K = 2000
    g = np.abs(_heavy(rng, K)).astype(TF)
    w = weights("lognormal", rng, K, TF)
    w[:300] = weights("masked", rng, 300, TF)
    theta = (np.abs(rng.standard_normal(K)) * 0.7).astype(TF)
    v = _heavy(rng, K).astype(TF)
    g[300:320] = 0.0
    v[320:340] = -0.0
    # the ties of the GPU test against theta = 2.5: (5, 2) is zeroed, (7, 2) scaled by 2 / 7, (7, 1) by 4.5 / 7
    g[400:403], w[400:403], theta[400:403], v[400:403] = [5, 7, 7], [2, 2, 1], 2.5, [3, -7, 7]
    tag = "f" if TF == np.float32 else "d"
    lines = [f"a {tag} {_hex(a)} {_hex(b)} {_hex(t)} {_hex(x)}" for a, b, t, x in zip(g, w, theta, v)]
    r = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True)
    out = r.stdout.splitlines()
    assert r.returncode == 0 and out[-1] == "ok", r.stdout[-2000:] + r.stderr
    got = np.array([[float.fromhex(x) for x in k.split()[1:]] for k in out if k.startswith("a ")])
    y = np.empty(K, TF)
    f = np.empty(K, TF)
    for k in range(K):                  # (theta differs from group to group here)
        yk, fk = R.emulate_apply(v[k:k + 1, None], g[k:k + 1], w[k:k + 1], theta[k])
        y[k], f[k] = yk[0, 0], fk[0]
    assert l1_exact.same_bits(got[:, 0].astype(TF), f) and l1_exact.same_bits(got[:, 1].astype(TF), y)
    assert list(f[400:403]) == [0, TF(TF(2) / TF(7)), TF(TF(4.5) / TF(7))]
    assert np.all(f[:300][w[:300] == 0][g[:300][w[:300] == 0] > 0] == 1), "weight 0: the factor is 1 exactly"
    assert l1_exact.same_bits(y[:300][w[:300] == 0], v[:300][w[:300] == 0])


# ---- host side ---------------------------------------------------------------------------------------------------------------------------
def test_set_definitions_without_weights_builds_the_same_descriptor(sipx):
    TF = np.float32
    g3 = sipx.compgrid((25.0, 25.0, 25.0), (16, 12, 8))
    for st, op in (("l21", "TV"), ("l21", "TV_xy"), ("l21_joint", "TV_xy"), ("l1", "TV")):
        a = sipx.set_definitions(st, op, 0.0, 3.5, ("tensor", ""))
        b = sipx.set_definitions(st, op, 0.0, 3.5, ("tensor", ""), ((), False), None)
        assert a == b and a.weights is None
        P, A, prop = sipx.setup_constraints([a], g3, TF)
        d = P[0].desc(A[0].kind, prop.ncvx[0])
        assert d.lb is None and d.ub is None and d.reserved == 0 and not P[0].weighted
        assert P[0].data_len(A[0]) is None


def test_setup_constraints_carries_the_weights(sipx):
    g3 = sipx.compgrid((25.0, 25.0, 25.0), (16, 12, 8))
    g2 = sipx.compgrid((25.0, 6.0), (16, 12))
    for TF in (np.float32, np.float64):
        for st, op, g, mode, ng, proj in (("l21", "TV", g3, ("tensor", ""), 1536, 14), ("l21", "TV", g2, ("matrix", ""), 192, 14),
                                          ("l21", "TV_xy", g3, ("tensor", ""), 1536, 14), ("l21_joint", "TV_xy", g3, ("tensor", ""), 192, 15)):
            w = np.linspace(0.0, 2.0, ng)                         # float64: setup_constraints takes it to the working precision
            c = [sipx.set_definitions("bounds", "identity", 1.0, 2.0, mode), sipx.set_definitions(st, op, 0.0, 3.5, mode, weights=w)]
            P, A, prop = sipx.setup_constraints(copy.deepcopy(c), g, TF)
            assert P[1].weighted and P[1].lb.dtype == TF and P[1].ub is None and np.array_equal(P[1].lb, w.astype(TF))
            assert P[1].data_len(A[1]) == ng and P[0].data_len(A[0]) is None
            d = P[1].desc(A[1].kind, prop.ncvx[1])
            assert (d.proj, d.mode, d.pmax, d.reserved) == (proj, 0, 3.5, ng) and d.lb is not None and d.ub is None
            # the automatic context caches refuse lists with array arguments
            opt = sipx.PARSDMM_options()
            opt.FL = TF
            assert sipx.host._context_key(np.zeros(1, TF), None, A, prop, P, g, opt, None) is None


def test_host_refusals(sipx):
    TF = np.float32
    g3 = sipx.compgrid((25.0, 25.0, 25.0), (16, 12, 8))
    w = np.ones(1536, TF)

    def P(st, op, mode, weights, g=g3, mx=1.0):
        return sipx.Projector(sipx.set_definitions(st, op, 0.0, mx, mode, weights=weights), g, TF)
    with pytest.raises(sipx.SipxError, match="per frame takes no weights.*tensor mode"):
        P("l21", "TV_xy", ("slice", "z"), w)
    for st, op in (("l1", "TV"), ("l2", "identity"), ("bounds", "identity"), ("cardinality", "D_z")):
        with pytest.raises(sipx.SipxError, match=f"set type '{st}' takes no weights: weights belong to the l2,1 sets"):
            P(st, op, ("tensor", ""), w)
    with pytest.raises(sipx.SipxError, match=r"l21 weights have shape \(1535,\): \(1536,\) is needed -- one per grid point"):
        P("l21", "TV", ("tensor", ""), w[:-1])
    with pytest.raises(sipx.SipxError, match=r"l21_joint weights have shape \(1536,\): \(192,\) is needed -- one per pixel"):
        P("l21_joint", "TV_xy", ("tensor", ""), w)
    with pytest.raises(sipx.SipxError, match=r"shape \(16, 12, 8\)"):
        P("l21", "TV", ("tensor", ""), w.reshape(16, 12, 8))
    with pytest.raises(sipx.SipxError, match="l21 weights have dtype float64: not the working precision"):
        P("l21", "TV", ("tensor", ""), w.astype(np.float64))
    with pytest.raises(sipx.SipxError, match="l21 weights must be a numpy array, not list"):
        P("l21", "TV", ("tensor", ""), list(w))
    for bad, at in ((-1.0, 5), (np.nan, 0), (np.inf, 77), (-np.inf, 1400)):
        wb = w.copy()
        wb[at] = wb[1500] = bad             # the message names the first offender
        with pytest.raises(sipx.SipxError, match=rf"the weighted l2,1 ball \(l21\): weight {at} is negative, NaN or infinite"):
            P("l21", "TV", ("tensor", ""), wb)
    assert P("l21", "TV", ("tensor", ""), np.zeros(1536, TF)).weighted, "all weights zero is a set"
    with pytest.raises(sipx.SipxError, match="Radius of L1 ball is negative"):
        P("l21", "TV", ("tensor", ""), w, mx=0.0)
    # the observers
    x = np.zeros(1536, TF)
    with pytest.raises(sipx.SipxError, match="per frame takes no weights"):
        sipx.l21_norm(x, g3, "TV_xy", ("slice", "z"), weights=w)
    with pytest.raises(sipx.SipxError, match="weights has 1535 entries, 1536 are needed"):
        sipx.l21_norm(x, g3, "TV", weights=w[:-1])
    with pytest.raises(sipx.SipxError, match="weights has 1536 entries, 192 are needed"):
        sipx.l21_joint_norm(x, g3, weights=w)
    wb = w.copy()
    wb[9] = -0.5
    with pytest.raises(sipx.SipxError, match="weight 9 is negative, NaN or infinite"):
        sipx.l21_norm(x, g3, "TV", weights=wb)
    for s in ("sipx_l21_weighted_norm", "sipx_l21_weighted_norm_dev"):
        assert s in sipx.EXPORTED_SYMBOLS


def test_constraint2coarse_refuses_weights(sipx):
    g = sipx.compgrid((1.0, 1.0), (64, 48))
    plain = [sipx.set_definitions("l21", "TV", 0.0, 12.0, ("matrix", ""))]
    assert sipx.constraint2coarse(copy.deepcopy(plain), g, 2)[0].max == 3.0
    c = [sipx.set_definitions("l21", "TV", 0.0, 12.0, ("matrix", ""), weights=np.ones(64 * 48, np.float32))]
    with pytest.raises(sipx.SipxError, match="multilevel: a weighted l2,1 set has no rule that takes its weights to a coarser grid"):
        sipx.constraint2coarse(c, g, 2)
