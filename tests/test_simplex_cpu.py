"""Simplex sets without a GPU: the exact reference (tests/simplex_ref.py) against the properties of a projection, csrc/seg_simplex.h on the
CPU (tests/simplex/rule_driver.cpp, compiled by hipcc; the program makes no HIP call) against the Python emulation of the rule bit for
bit and against the exact threshold, its termination on NaN and infinities, the lane route's buckets, the host refusals and the
constants."""
import copy
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import simplex_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "setintersectionprojection.jl_amd", "csrc")
BOUNDS = [(1.0, 1.0), (0.5, 2.0), (0.0, 1.0)]
FAMILIES = ("mixed", "above", "below", "negative", "quarters", "zero")


def segment(family, rng, L, TF, b=1.0):
    """One segment of each input family of the GPU tests."""
    if family == "mixed":
        v = rng.standard_normal(L) * 10.0 ** rng.uniform(-2, 2)
    elif family in ("above", "below"):
        p = rng.random(L) + 0.05
        v = p / p.sum() * b * (1.0 + (1 if family == "above" else -1) * 10.0 ** rng.uniform(-3, -1))
    elif family == "negative":
        v = -50.0 - 100.0 * rng.random(L)
    elif family == "quarters":
        v = rng.integers(-8, 13, L) / 4.0
    else:
        v = np.zeros(L)
        v[::2] = -0.0
    return v.astype(TF)


# ---- the reference ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("smin,smax", BOUNDS)
@pytest.mark.parametrize("family", FAMILIES)
def test_reference_is_the_projection(family, smin, smax):
    """Feasible exactly, and <v - x, z - x> <= 0 for feasible z up to the one rounding of x: the variational inequality."""
    rng = np.random.default_rng(11 + len(family))
    eps = float(np.finfo(np.float64).eps)
    for L in (1, 2, 3, 8, 33):
        v = segment(family, rng, L, np.float64, smax)
        x, th, case = R.exact_segment(v, smin, smax)
        assert np.all(x >= 0)
        s = sum(Fraction(a) for a in x)
        scale = max(float(np.abs(v).max()), smax, abs(float(th)))
        assert Fraction(smin) - L * eps * scale <= s <= Fraction(smax) + L * eps * scale, (family, L, float(s))
        if case == R.KEEP:
            assert np.array_equal(x, v)
        for _ in range(20):
            # feasible exactly: multiples of 1 / 1024 whose sum is a multiple of 1 / 1024 in [smin, smax]
            total = int(rng.integers(int(smin * 1024), int(smax * 1024) + 1))
            z = rng.multinomial(total, rng.dirichlet(np.ones(L))) / 1024.0
            assert R.is_feasible(z, smin, smax)
            vi = float(np.dot(v - x, z - x))
            assert vi <= 64 * L * eps * scale * max(scale, 1.0), (family, L, vi)


def test_reference_cases():
    x, th, case = R.exact_segment(np.array([0.25, 0.5, 0.25]), 1.0, 1.0)
    assert case == R.KEEP and th == 0 and np.array_equal(x, [0.25, 0.5, 0.25])
    x, th, case = R.exact_segment(np.array([0.25, -3.0, 0.5]), 0.5, 2.0)
    assert case == R.CLIP and np.array_equal(x, [0.25, 0.0, 0.5])
    x, th, case = R.exact_segment(np.array([2.0, 1.0, -1.0]), 1.0, 1.0)          # theta = 1: the entry on the threshold comes back 0
    assert case == R.SHIFT and th == 1 and np.array_equal(x, [1.0, 0.0, 0.0])
    x, th, case = R.exact_segment(np.array([-2.0, -4.0]), 1.0, 1.0)              # the lower side: theta < 0
    assert case == R.SHIFT and th == -3 and np.array_equal(x, [1.0, 0.0])
    x, th, case = R.exact_segment(np.zeros(4), 0.5, 2.0)                          # the constant fill smin / L
    assert th == Fraction(-1, 8) and np.array_equal(x, np.full(4, 0.125))
    x, th, case = R.exact_segment(np.array([-7.0]), 1.0, 3.0)
    assert th == -8 and np.array_equal(x, [1.0])
    x, th, case = R.exact_segment(np.array([7.0]), 1.0, 3.0)
    assert th == 4 and np.array_equal(x, [3.0])
    n = (4, 3, 2)
    assert R.rows(n, "D_z") == 12 and len(R.segments(n, "D_x", ("fiber", "z"))) == 9 and len(R.segments(n, "identity", ("slice", "y"))) == 3


# ---- the header -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    hipcc = shutil.which("hipcc") or shutil.which("hipcc", path=os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin"))
    assert hipcc, "hipcc not found"
    exe = str(tmp_path_factory.mktemp("simplex") / "rule_driver")
    r = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                        "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "simplex", "rule_driver.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _hex(a):
    a = float(a)
    return "nan" if a != a else ("inf" if a == np.inf else ("-inf" if a == -np.inf else a.hex()))


def _run(driver, TF, cases, stride=1, pad=None):
    """cases: (v, smin, smax) -> (case, theta, spos, steps, buffer) of each, the buffer of (L - 1) stride + 1 entries."""
    tf = "f" if TF == np.float32 else "d"
    lines = []
    for v, smin, smax in cases:
        buf = np.full((len(v) - 1) * stride + 1, np.nan if pad is None else pad, TF)
        buf[::stride] = v
        lines.append(f"p {tf} {_hex(TF(smin))} {_hex(TF(smax))} {len(v)} {stride} " + " ".join(_hex(a) for a in buf))
    r = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    out = r.stdout.splitlines()
    assert r.returncode == 0 and out and out[-1] == "ok", r.stdout[-2000:] + r.stderr
    got = [k.split()[1:] for k in out if k.startswith("p ")]
    assert len(got) == len(cases)
    return [(int(g[0]), TF(float.fromhex(g[1])), TF(float.fromhex(g[2])), int(g[3]), np.array([float.fromhex(a) for a in g[4:]]).astype(TF))
            for g in got]


def _nearest(TF, q):
    """The Fraction q rounded once to TF (ties away from the float64 detour are not met: the candidates are compared exactly)."""
    c = TF(float(q))
    cands = [c, np.nextafter(c, TF(np.inf)), np.nextafter(c, TF(-np.inf))]
    return min(cands, key=lambda a: abs(Fraction(float(a)) - q))


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _cases(TF, count=40):
    rng = np.random.default_rng(29)
    cases = []
    for family in FAMILIES:
        for smin, smax in BOUNDS:
            for L in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 70):
                for _ in range(max(1, count // 12)):
                    cases.append((segment(family, rng, L, TF, smax), smin, smax))
    return cases


@pytest.mark.parametrize("TF", [np.float32, np.float64])
def test_header_equals_the_emulation_bit_for_bit(driver, TF):
    cases = _cases(TF)
    got = _run(driver, TF, cases)
    seen = set()
    for (v, smin, smax), (case, theta, spos, steps, y) in zip(cases, got):
        want = R.emulate(v, smin, smax)
        assert case == want[0] and steps == want[3], (v, smin, smax)
        assert _same_bits(np.array([theta, spos]), np.array([want[1], want[2]], TF)), (v, smin, smax, theta, want[1])
        assert _same_bits(y, want[4]), (v, smin, smax)
        if case == R.KEEP:
            assert _same_bits(y, v), "a segment inside its set was written"
        if case == R.CLIP:
            assert _same_bits(y[v >= 0], v[v >= 0]) and not np.any(np.signbit(y[v < 0])) and np.all(y[v < 0] == 0)
        seen.add(case)
    assert seen == {R.KEEP, R.CLIP, R.SHIFT}


@pytest.mark.parametrize("TF", [np.float32, np.float64])
def test_michelot_reaches_the_exact_threshold(driver, TF):
    """theta of the header is theta* rounded to T, on the upper and on the lower side; the families hold all-negative input on the lower
    side, a zero segment with smin > 0 (the constant fill smin / L) and L = 1."""
    cases = [c for c in _cases(TF, 120)]
    got = _run(driver, TF, cases)
    eps = float(np.finfo(TF).eps)
    sides, worst = set(), 0.0
    for (v, smin, smax), (case, theta, spos, steps, y) in zip(cases, got):
        x, th, want_case = R.exact_segment(v, TF(smin), TF(smax))
        assert case == want_case, (v, smin, smax)
        if case != R.SHIFT:
            continue
        assert theta == _nearest(TF, th), (v, smin, smax, float(theta), float(th))
        assert steps <= len(v) + 1
        sides.add(theta > 0)
        scale = np.maximum(np.abs(v.astype(np.float64)), abs(float(th)))
        worst = max(worst, float(np.max(np.abs(y.astype(np.float64) - x) / (eps * scale))))
    assert sides == {True, False}
    print(f"simplex serial rule {np.dtype(TF).name}: worst error {worst:.3f} eps max(|v|, |theta*|)")
    assert worst <= 2.0
    zero = _run(driver, TF, [(np.zeros(5, TF), 0.5, 2.0), (np.array([-3.0], TF), 1.0, 1.0), (np.array([5.0], TF), 0.5, 2.0)])
    assert _same_bits(zero[0][4], np.full(5, TF(TF(0.5) / 5), TF)) and zero[0][1] == -TF(TF(0.5) / 5)
    assert _same_bits(zero[1][4], np.array([1.0], TF)) and _same_bits(zero[2][4], np.array([2.0], TF))


@pytest.mark.parametrize("TF", [np.float32, np.float64])
def test_the_loop_ends_on_nan_and_infinities(driver, TF):
    """The driver returns (the subprocess has a time limit), within L + 1 steps; a segment without such an entry beside them is untouched by
    them: each line is a call of its own."""
    rng = np.random.default_rng(31)
    cases = []
    for bad in (np.nan, np.inf, -np.inf):
        for L in (1, 4, 33):
            for where in (0, L - 1):
                v = segment("mixed", rng, L, TF)
                v[where] = bad
                cases.append((v, 1.0, 1.0))
    cases.append((np.array([np.inf, -np.inf, np.nan, 1.0], TF), 0.0, 1.0))
    cases.append((np.full(7, np.finfo(TF).max, TF), 0.5, 2.0))
    for (v, _, _), (case, theta, spos, steps, y) in zip(cases, _run(driver, TF, cases)):
        assert steps <= len(v) + 2 and len(y) == len(v)
        if np.isnan(v).any() or (np.isinf(v).any() and (v == np.inf).any()):
            assert case == R.SHIFT and not np.isnan(y).any()


@pytest.mark.parametrize("TF", [np.float32, np.float64])
def test_entries_between_the_segments_elements_are_not_touched(driver, TF):
    """A strided segment (a fiber across the array): what lies between its elements -- other segments, a pad row or plane -- is neither
    read nor written, NaN included."""
    rng = np.random.default_rng(37)
    cases = [(segment(f, rng, L, TF), 1.0, 1.0) for f in FAMILIES for L in (2, 5, 9)]
    plain = _run(driver, TF, cases)
    for stride in (3, 8):
        got = _run(driver, TF, cases, stride=stride)
        for a, b in zip(plain, got):
            assert a[0] == b[0] and a[3] == b[3] and _same_bits(np.array(a[1:3]), np.array(b[1:3]))
            assert _same_bits(b[4][::stride], a[4])
            rest = np.delete(b[4], np.arange(0, len(b[4]), stride))
            assert np.isnan(rest).all()


def test_lane_buckets(driver):
    """simplex_lane_bucket: the lane route where neighbouring segments are contiguous (sSa == 1), the segments are fibers (LB == 1) and
    L <= SIMPLEX_REG_MAX = 16; buckets 4, 8, 16."""
    head = open(os.path.join(CSRC, "seg_simplex.h")).read()
    assert "constexpr int SIMPLEX_REG_MAX = 16;" in head
    asks = [(L, 1, 1) for L in (1, 2, 4, 5, 8, 9, 16, 17, 32, 33, 300)] + [(8, 1, 33), (8, 4, 1)]
    r = subprocess.run([driver], input="".join(f"k {L} {LB} {s}\n" for L, LB, s in asks), capture_output=True, text=True, timeout=60)
    got = [int(k.split()[1]) for k in r.stdout.splitlines() if k.startswith("k ")]
    assert got == [4, 4, 4, 8, 8, 16, 16, 0, 0, 0, 0, 0, 0]


# ---- host side ----------------------------------------------------------------------------------------------------------------------------
def test_setup_constraints_takes_the_set(sipx):
    g3 = sipx.compgrid((25.0, 25.0, 25.0), (16, 12, 8))
    g2 = sipx.compgrid((25.0, 6.0), (16, 12))
    assert sipx.host.PROJ["simplex"] == 19
    for TF in (np.float32, np.float64):
        for op, g, mode, rows in (("identity", g3, ("fiber", "z"), 1536), ("D_z", g3, ("fiber", "z"), 16 * 12 * 7), ("D_x", g3, ("slice", "y"), 15 * 12 * 8),
                                  ("identity", g2, ("fiber", "x"), 192), ("D_z", g2, ("fiber", "z"), 16 * 11)):
            c = [sipx.set_definitions("bounds", "identity", 0.0, 1.0, ("tensor", "")), sipx.set_definitions("simplex", op, 0.5, 2.0, mode)]
            P, A, prop = sipx.setup_constraints(copy.deepcopy(c), g, TF)
            assert A[1].shape[0] == rows and P[1].kind == "simplex" and not P[1].weighted and not P[1].seg_radii
            assert P[1].data_len(A[1]) is None and P[1].lb is None and P[1].ub is None
            assert prop.tag[1] == ("simplex", op, mode[0], mode[1]) and prop.ncvx[1] is False
            d = P[1].desc(A[1].kind, prop.ncvx[1])
            assert (d.proj, d.mode, d.pmin, d.pmax, d.reserved, d.transform) == (19, P[1].mode, 0.5, 2.0, 0, 0) and d.lb is None and d.ub is None


def test_host_refusals(sipx):
    TF = np.float32
    H = sipx.host
    g3 = sipx.compgrid((25.0, 25.0, 25.0), (16, 12, 8))
    g2 = sipx.compgrid((25.0, 6.0), (16, 12))

    def P(op, mode, lo=1.0, hi=1.0, g=g3, cust=((), False), weights=None):
        return sipx.Projector(sipx.set_definitions("simplex", op, lo, hi, mode, cust, weights), g, TF)

    def refused(text, *a, **k):
        with pytest.raises(sipx.SipxError) as e:
            P(*a, **k)
        assert str(e.value).startswith(text), str(e.value)
    for mode in (("tensor", ""), ("matrix", "")):
        refused(H.SIMPLEX_NEEDS_MODE, "identity", mode)
    assert "not built yet" in H.SIMPLEX_NEEDS_MODE and '("bounds") together with ("l1")' in H.SIMPLEX_NEEDS_MODE
    refused(H.SIMPLEX_2D_SLICE, "identity", ("slice", "x"), g=g2)
    for op in ("TV", "D3D", "TV_xy", "D_xz"):
        refused(H.SIMPLEX_ONE_BLOCK, op, ("fiber", "z"))
    import scipy.sparse as sp
    refused(H.SIMPLEX_ONE_BLOCK, "identity", ("fiber", "z"), cust=(sp.identity(1536, format="csc"), False))
    for op in ("DFT", "DCT", "wavelet"):
        refused(H.SIMPLEX_NO_TRANSFORM, op, ("fiber", "z"))
    refused("provided an unknown transform domain operator", "D_y", ("fiber", "x"), g=g2)
    refused(H.SIMPLEX_NO_VECTORS, "identity", ("fiber", "z"), hi=np.ones(192, TF))
    refused(H.SIMPLEX_NO_VECTORS, "identity", ("fiber", "z"), lo=np.zeros(192, TF), hi=np.ones(192, TF))
    assert "one pair of scalars" in H.SIMPLEX_NO_VECTORS
    refused(H.SIMPLEX_NO_WEIGHTS, "identity", ("fiber", "z"), weights=np.ones(192, TF))
    for lo, hi in ((-0.5, 1.0), (2.0, 1.0), (0.0, 0.0), (0.0, np.inf), (np.nan, 1.0), (0.0, np.nan), (0.0, -1.0)):
        refused(H.SIMPLEX_BAD_BOUNDS, "identity", ("fiber", "z"), lo=lo, hi=hi)
    ok = P("D_z", ("fiber", "z"), 0.0, 1.0)
    assert (ok.kind, ok.pmin, ok.pmax, ok.op) == ("simplex", 0.0, 1.0, "D_z")
    with pytest.raises(sipx.SipxError, match="this set was built for D_z, the operator is D_x"):
        ok.check_rows(sipx.TDOperator("D_x", g3, TF))
    with pytest.raises(sipx.SipxError, match="takes no Minkowski component"):
        ok.check_rows(sipx.TDOperator("D_z", g3, TF, component=1))
    with pytest.raises(sipx.SipxError, match=f"the simplex set projects a vector of the D_z range: {16 * 12 * 7} entries on this grid, 7 given"):
        ok(np.zeros(7, TF))
    # the observer
    x = np.zeros(1536, TF)
    for op, mode, text in (("TV", ("fiber", "z"), H.SIMPLEX_ONE_BLOCK), ("DCT", ("fiber", "z"), H.SIMPLEX_NO_TRANSFORM),
                           ("identity", ("tensor", ""), H.SIMPLEX_NEEDS_MODE)):
        with pytest.raises(sipx.SipxError) as e:
            sipx.segment_sums(x, g3, op, mode)
        assert str(e.value) == text
    with pytest.raises(sipx.SipxError, match="x must be a Float32 or Float64"):
        sipx.segment_sums(list(x), g3, "identity", ("fiber", "z"))
    for s in ("sipx_segment_sums", "sipx_segment_sums_dev"):
        assert s in sipx.EXPORTED_SYMBOLS
    # multilevel
    c = [sipx.set_definitions("simplex", "identity", 1.0, 1.0, ("fiber", "z"))]
    with pytest.raises(sipx.SipxError, match="multilevel: the simplex set .simplex. has no rule"):
        sipx.constraint2coarse(c, g3, 2)


def test_the_constant_and_the_texts_are_declared_everywhere(sipx):
    head = open(os.path.join(ROOT, "include", "sipx.h")).read()
    assert "SIPX_PROJ_SIMPLEX = 19" in head and "int sipx_segment_sums(" in head and "int sipx_segment_sums_dev(" in head
    assert "EXT_SIMPLEX_SEG = 20" in open(os.path.join(CSRC, "ext_proj.h")).read()
    assert "SIPX_PROJ_SIMPLEX = 19" in open(os.path.join(ROOT, "julia", "SipxPARSDMM.jl")).read()
    rule = open(os.path.join(CSRC, "seg_simplex.h")).read()
    assert 'runtime_error("the simplex' not in open(os.path.join(CSRC, "set_config.h")).read()
    for name in ("SIMPLEX_NEEDS_MODE", "SIMPLEX_2D_SLICE", "SIMPLEX_ONE_BLOCK", "SIMPLEX_NO_TRANSFORM", "SIMPLEX_NO_MINKOWSKI", "SIMPLEX_NO_VECTORS",
                 "SIMPLEX_BAD_BOUNDS"):
        # the engine's words and the front end's are the same
        i = rule.index(f"constexpr const char* {name} = ")
        lit = rule[i:rule.index(";", i)].split("=", 1)[1]
        text = "".join(eval(part) for part in __import__("re").findall(r'"(?:[^"\\]|\\.)*"', lit))
        assert text == getattr(sipx.host, name), name
