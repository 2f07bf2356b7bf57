"""Group cardinality without a GPU: the numpy reference (tests/card_groups_ref.py) against the selection contract of tests/card_exact.py,
csrc/card_groups.h on the CPU (tests/card_groups/rule_driver.cpp, a stand-alone program built by the host compiler, with
-fsanitize=address,undefined where the compiler has the runtimes) -- the serial rule and the rank-by-counting rule of the small route
held to the same contract --, the plans of the norms launch for the cases of tests/test_gpu_card_groups.py (csrc/l21_groups.h through
tests/l21_groups/rule_driver.cpp), the host descriptors and the refusals, word for word against the header."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import card_exact
from tests import card_groups_cases as CS
from tests import card_groups_ref as R
from tests import seg_norms_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "setintersectionprojection.jl_amd", "csrc")
PRECISIONS = [np.float32, np.float64]


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------
def test_reference_example():
    """(2, 3) fiber x: norms (3, 5, 4); k = 2 keeps fibers 1 and 2, k = 1 fiber 1, k = 3 and the all-zero input give v itself."""
    v = np.array([3.0, 0.0, 0.0, -5.0, 4.0, -0.0])
    n, mode = (2, 3), ("fiber", "x")
    assert np.array_equal(R.norms(v, n, "identity", mode, np.float64), [3.0, 5.0, 4.0])
    assert np.array_equal(R.project(v, n, "identity", mode, 2), [0.0, 0.0, 0.0, -5.0, 4.0, -0.0])
    assert np.array_equal(R.project(v, n, "identity", mode, 1), [0.0, 0.0, 0.0, -5.0, 0.0, 0.0])
    assert R.project(v, n, "identity", mode, 3) is v and R.project(v, n, "identity", mode, 7) is v
    z = np.zeros(6)
    assert R.project(z, n, "identity", mode, 1) is z
    y = R.project(v, n, "identity", mode, 2)
    assert R.project(y, n, "identity", mode, 2) is y, "the projection of a projection drops something"
    assert R.gap([3.0, 5.0, 4.0], 2) == 0.25 and R.gap([3.0, 5.0, 4.0], 3) == float("inf")


@pytest.mark.parametrize("TF", PRECISIONS)
def test_reference_selection_is_the_contract_on_the_key(TF):
    for op, n, mode in [c for c in CS.CASES if int(np.prod(c[1])) < 5000]:
        ns = R.nseg(n, op, mode)
        for k in CS.ks(ns):
            v = CS.mixed_input(op, n, mode, TF, zeros=k != ns - 1)
            g = R.norms(v, n, op, mode, TF)
            keep = R.kept(g, k)
            card_exact.check_card_output(g, np.where(keep, g, TF(0)).astype(TF), k)
            y = R.project(v, n, op, mode, k)
            for s, idx in enumerate(CS.segs(op, n, mode)):
                assert np.array_equal(y[idx], v[idx]) if keep[s] else not y[idx].any()


def test_exact_norms_agree_with_the_rational_sum():
    rng = np.random.default_rng(3)
    for TF in PRECISIONS:
        v = (rng.standard_normal(60) * np.exp(3 * rng.standard_normal(60))).astype(TF)
        g = R.norms(v, (5, 4, 3), "identity", ("slice", "z"), TF)
        assert R.norm_error_units(g, v, (5, 4, 3), "identity", ("slice", "z")) <= 0.52       # (half a unit, and the bisection's 1/64)
        bad = g.copy()
        bad[1] = np.nextafter(np.nextafter(bad[1], TF(np.inf)), TF(np.inf))
        assert R.norm_error_units(bad, v, (5, 4, 3), "identity", ("slice", "z")) > 0.98


# ---- csrc/card_groups.h on the CPU -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    exe = str(tmp_path_factory.mktemp("card_groups") / "rule_driver")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "card_groups", "rule_driver.cpp"),
            "-o", exe]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if r.returncode != 0:          # a compiler without the sanitizer runtimes: the plain program
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _run(driver, lines):
    r = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True)
    out = r.stdout.splitlines()
    assert r.returncode == 0 and out and out[-1] == "ok", "\n".join(k for k in out if k.startswith("FAIL"))[:4000] + r.stderr[:4000]
    return out[:-1]


def _hex(x):
    return float(x).hex()


def _rule_cases(TF):
    """[(g, k)]: random keys with zeros, tie groups straddling the k-th place, k = 1, k = nseg - 1, k >= nseg, all-zero g, one segment."""
    rng = np.random.default_rng(11)
    out = []
    for ns in (2, 3, 7, 64, 65, 300, 1025):
        g = np.abs(card_exact.heavy(rng, ns, TF))
        g[g == 0] = TF(1)
        if ns > 3:
            g[1::7] = 0
        for k in sorted({1, 2, ns // 3, int((g > 0).sum()) - 1, int((g > 0).sum()), ns - 1, ns, ns + 5}):
            if k >= 1:
                out.append((g.copy(), k))
    tie = np.array([5, 1, 1, 9, 1, 1, 0, 1, 1, 7, 1], TF)                        # three above, a group of seven, a zero
    out += [(tie, k) for k in (3, 4, 5, 9, 10, 11)]
    out += [(np.full(50, 2.5, TF), k) for k in (1, 17, 49, 50)]                   # one tie group: the lowest k indices
    sub = np.nextafter(TF(0), TF(1))
    out += [(np.array([sub, 2 * sub, sub, 0, 2 * sub, sub], TF), k) for k in (1, 2, 3, 4)]      # the smallest subnormals
    out += [(np.array([np.finfo(TF).max, 1, np.finfo(TF).max], TF), 1)]
    out += [(np.zeros(9, TF), 1), (np.zeros(9, TF), 9), (np.array([3.0], TF), 1), (np.array([0.0], TF), 1), (np.array([3.0], TF), 4)]
    return out


@pytest.mark.parametrize("TF", PRECISIONS)
def test_both_rules_are_the_stable_selection(driver, TF):
    cases = _rule_cases(TF)
    p = "f" if TF == np.float32 else "d"
    out = _run(driver, [f"s {p} {k} {len(g)} " + " ".join(_hex(x) for x in g) for g, k in cases])
    assert len(out) == len(cases)
    straddled = 0
    for (g, k), row in zip(cases, out):
        f = row.split()
        need, tau, cut, need2, tau2, cut2, word = int(f[1]), TF(float.fromhex(f[2])), int(f[3]), int(f[4]), TF(float.fromhex(f[5])), int(f[6]), f[7]
        assert (need, tau, cut) == (need2, tau2, cut2), "the serial rule and the rank rule differ"
        keep = np.array([c == "1" for c in word])
        card_exact.check_card_output(g, np.where(keep, g, TF(0)).astype(TF), k)
        assert np.array_equal(keep, R.kept(g, k)), (g, k)
        nnz = int((g > 0).sum())
        assert need == (1 if nnz > k and k < len(g) else 0)
        if need:
            assert tau > 0 and tau == np.sort(g)[::-1][k - 1] and g[cut] == tau and int(keep.sum()) == k
            straddled += card_exact.straddles(g, k)[0]
        else:
            assert tau == 0 and cut == 2 ** 63 - 1 and keep.all()
    assert straddled >= 8, "no tie group straddles the k-th place"


def _constants():
    """name -> text of every `constexpr const char* CARDG_...` of the header (adjacent literals joined)."""
    src = open(os.path.join(CSRC, "card_groups.h"), encoding="utf-8").read()
    out = {}
    for m in re.finditer(r"constexpr const char\* (CARDG_[A-Z0-9_]+) = ((?:\s*\"(?:[^\"\\]|\\.)*\")+);", src):
        out[m.group(1)] = "".join(re.findall(r"\"((?:[^\"\\]|\\.)*)\"", m.group(2))).replace('\\"', '"')
    return out


def test_refusals_are_worded_once(sipx):
    c = _constants()
    assert set(c) == {"CARDG_NEEDS_MODE", "CARDG_2D_SLICE", "CARDG_ONE_BLOCK", "CARDG_NO_TRANSFORM", "CARDG_NO_MINKOWSKI", "CARDG_NO_VECTORS",
                      "CARDG_NO_SET_DATA", "CARDG_SHARDED", "CARDG_BAD_K", "CARDG_K_INEXACT", "CARDG_TOO_LARGE"}
    for name, text in c.items():
        assert getattr(sipx.host, name) == text, name
    # every text names a way out
    for name, way in [("CARDG_NEEDS_MODE", "drop the set"), ("CARDG_2D_SLICE", "(fiber,x) or (fiber,z)"), ("CARDG_ONE_BLOCK", "use the cardinality set"),
                      ("CARDG_NO_TRANSFORM", "use the cardinality set behind the transform"), ("CARDG_NO_MINKOWSKI", "the sum of the components"),
                      ("CARDG_NO_VECTORS", "use the l21_groups set"), ("CARDG_NO_SET_DATA", "build a new context"), ("CARDG_SHARDED", "use a single process"),
                      ("CARDG_BAD_K", "use bounds"), ("CARDG_K_INEXACT", "use Float64"), ("CARDG_TOO_LARGE", "split the array")]:
        assert way in c[name], name
    assert "another number of segments" in sipx.host.CARDG_NO_COARSE and "one level" in sipx.host.CARDG_NO_COARSE


def test_k_is_checked_alike_in_the_header_and_on_the_host(driver, sipx):
    H = sipx.host
    g = sipx.compgrid((1.0, 1.0, 1.0), (300, 300, 200))          # fiber z: 90000 segments; slice z: 200
    asks = [("f", 1.0, 7, "ok"), ("f", 0.0, 7, H.CARDG_BAD_K), ("f", -2.0, 7, H.CARDG_BAD_K), ("f", 2.5, 7, H.CARDG_BAD_K),
            ("f", float("nan"), 7, H.CARDG_BAD_K), ("d", float("inf"), 7, H.CARDG_BAD_K),
            ("f", 2.0 ** 24 + 1, 2 ** 25, H.CARDG_K_INEXACT), ("f", 2.0 ** 24, 2 ** 25, "ok"), ("d", 2.0 ** 24 + 1, 2 ** 25, "ok"),
            ("f", 2.0 ** 24 + 1, 1000, "ok")]                      # (k >= nseg: every segment stays, k is not read)
    out = _run(driver, [f"k {p} {_hex(k) if np.isfinite(k) else k} {ns}" for p, k, ns, _ in asks])
    for (p, k, ns, want), row in zip(asks, out):
        assert row == "k " + want, (p, k, ns, row)
    for k, text in [(0, H.CARDG_BAD_K), (-1, H.CARDG_BAD_K), (1.5, H.CARDG_BAD_K), (float("nan"), H.CARDG_BAD_K), (float("inf"), H.CARDG_BAD_K),
                    (True, H.CARDG_BAD_K)]:
        with pytest.raises(sipx.SipxError) as e:
            sipx.Projector(sipx.set_definitions("card_groups", "identity", 0.0, k, ("fiber", "z")), g, np.float32)
        assert str(e.value) == text, k
    big = sipx.compgrid((1.0, 1.0, 1.0), (8192, 4096, 2))        # fiber z: 2^25 segments
    with pytest.raises(sipx.SipxError) as e:
        sipx.Projector(sipx.set_definitions("card_groups", "identity", 0.0, 2 ** 24 + 1, ("fiber", "z")), big, np.float32)
    assert str(e.value) == H.CARDG_K_INEXACT
    assert sipx.Projector(sipx.set_definitions("card_groups", "identity", 0.0, 2 ** 24 + 1, ("fiber", "z")), big, np.float64).pmax == 2.0 ** 24 + 1
    assert sipx.Projector(sipx.set_definitions("card_groups", "identity", 0.0, 2 ** 24 + 1, ("slice", "z")), big, np.float32).pmax == 2.0 ** 24 + 1
    # through setup_constraints, which rounds the scalars of other sets to TF when min is a float: k must reach the check unrounded
    for lo in (0, 0.0, np.float32(0)):
        with pytest.raises(sipx.SipxError) as e:
            sipx.setup_constraints([sipx.set_definitions("card_groups", "identity", lo, 2 ** 24 + 1, ("fiber", "z"))], big, np.float32)
        assert str(e.value) == H.CARDG_K_INEXACT, lo
    small = sipx.compgrid((1.0, 1.0, 1.0), (6, 5, 4))
    P, _, _ = sipx.setup_constraints([sipx.set_definitions("card_groups", "identity", 0.0, 2 ** 24 + 1, ("fiber", "z"))], small, np.float32)
    assert P[0].pmax == 2.0 ** 24 + 1, "k >= nseg keeps its value"
    assert int(_run(driver, ["c"])[0].split()[1]) == CS.SMALL_MAX


# ---- the host: descriptor, ncvx, refusals ------------------------------------------------------------------------------------------------------
def _def(sipx, op="D_z", k=3, mode=("fiber", "z"), **kw):
    return sipx.set_definitions("card_groups", op, 0.0, k, mode, **kw)


def test_descriptor_and_ncvx(sipx):
    g = sipx.compgrid((1.0, 1.0, 1.0), (16, 12, 8))
    for TF in PRECISIONS:
        P, A, prop = sipx.setup_constraints([sipx.set_definitions("bounds", "identity", 0.0, 1.0, ("tensor", "")), _def(sipx, "D_z", 5),
                                             _def(sipx, "identity", 2, ("slice", "z"))], g, TF)
        assert prop.ncvx == [False, True, True]
        assert prop.tag[1] == ("card_groups", "D_z", "fiber", "z")
        d = P[1].desc("D_z", True)
        assert (d.proj, d.pmin, d.pmax, d.mode, d.dir, d.reserved, d.ncvx, d.transform) == (20, 0.0, 5.0, 1, 2, 0, 1, 0) and not d.lb and not d.ub
        assert P[1].nseg(A[1]) == 16 * 12 and P[2].nseg(A[2]) == 8 and P[1].data_len(A[1]) is None
    assert sipx.host.PROJ["card_groups"] == 20
    assert {"sipx_group_norms", "sipx_group_norms_dev", "sipx_card_groups_route"} <= set(sipx.EXPORTED_SYMBOLS)
    assert "count_nonzero(group_norms)" in sipx.group_norms.__doc__


def test_host_refusals(sipx):
    H = sipx.host
    g3, g2 = sipx.compgrid((1.0, 1.0, 1.0), (16, 12, 8)), sipx.compgrid((1.0, 1.0), (16, 12))
    TF = np.float32

    def refused(c, g, text):
        for build in (lambda: sipx.Projector(c, g, TF), lambda: sipx.setup_constraints([c], g, TF)):
            with pytest.raises(sipx.SipxError) as e:
                build()
            assert str(e.value) == text, (str(e.value), text)
    refused(_def(sipx, mode=("tensor", "")), g3, H.CARDG_NEEDS_MODE)
    refused(_def(sipx, "identity", mode=("matrix", "")), g2, H.CARDG_NEEDS_MODE)
    refused(_def(sipx, "identity", mode=("slice", "x")), g2, H.CARDG_2D_SLICE)
    for op in ("TV", "TV_xy", "D2D"):
        refused(_def(sipx, op), g3, H.CARDG_ONE_BLOCK)
    for op in ("DFT", "DCT", "wavelet"):
        refused(_def(sipx, op), g3, H.CARDG_NO_TRANSFORM)
    import scipy.sparse as sp
    refused(_def(sipx, "identity", custom_TD_OP=(sp.identity(16 * 12 * 8, format="csc", dtype=TF), False)), g3, H.CARDG_ONE_BLOCK)
    refused(_def(sipx, weights=np.ones(16 * 12, TF)), g3, H.CARDG_NO_VECTORS)
    refused(_def(sipx, k=np.full(16 * 12, 3.0, TF)), g3, H.CARDG_NO_VECTORS)
    refused(_def(sipx, "identity"), sipx.compgrid((1.0, 1.0, 1.0), (2048, 1024, 1024)), H.CARDG_TOO_LARGE)
    # multilevel: no rule takes k to another grid
    with pytest.raises(sipx.SipxError) as e:
        sipx.constraint2coarse([_def(sipx)], g3, (2, 2, 2))
    assert str(e.value) == H.CARDG_NO_COARSE
    # the observer refuses what the set refuses, before a context exists
    x = np.zeros(16 * 12 * 8, TF)
    for op, mode, text in [("TV", ("fiber", "z"), H.CARDG_ONE_BLOCK), ("DFT", ("fiber", "z"), H.CARDG_NO_TRANSFORM),
                           ("D_z", ("tensor", ""), H.CARDG_NEEDS_MODE)]:
        with pytest.raises(sipx.SipxError) as e:
            sipx.group_norms(x, g3, op, mode)
        assert str(e.value) == text
    with pytest.raises(sipx.SipxError) as e:
        sipx.group_norms(np.zeros(16 * 12, TF), g2, "identity", ("slice", "z"))
    assert str(e.value) == H.CARDG_2D_SLICE


# ---- the plans of the GPU cases (csrc/l21_groups.h, csrc/seg_norm.h through the l21_groups driver) ------------------------------------------------
@pytest.fixture(scope="module")
def plan_driver(tmp_path_factory):
    hipcc = shutil.which("hipcc") or shutil.which("hipcc", path=os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin"))
    assert hipcc, "hipcc not found"
    exe = str(tmp_path_factory.mktemp("card_groups_plan") / "plan_driver")
    r = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                        "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "l21_groups", "rule_driver.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _plan_line(op, n, mode):
    n3 = tuple(n) + (1,) * (3 - len(n))
    opdir = -1 if op == "identity" else {"D_x": 0, "D_y": 1, "D_z": len(n) - 1}[op]
    return f"plan {len(n)} {n3[0]} {n3[1]} {n3[2]} {opdir} {1 if mode[0] == 'fiber' else 2} {seg_norms_ref.axis_of(n, mode)}"


def test_the_gpu_cases_reach_what_they_claim(plan_driver):
    cases = CS.CASES + [CS.BIG_TIE]
    rows = [k.split() for k in _run(plan_driver, [_plan_line(*c) for c in cases]) if k.startswith("plan ")]
    assert len(rows) == 2 * len(cases)
    plans = {}
    for i, c in enumerate(cases):
        for j, eb in enumerate((4, 8)):
            row = rows[2 * i + j]
            plans[(c, eb)] = {row[q]: int(row[q + 1]) for q in range(1, len(row), 2)}
            assert plans[(c, eb)]["bytes"] == eb
    for eb in (4, 8):
        fib = [plans[(c, eb)] for c in CS.CASES if c[2][0] == "fiber"]
        assert all(p["slices"] == 0 for p in fib)
        assert {p["path"] for p in fib} == {0, 1, 2, 3}, "the fiber cases miss a path of seg_norm_plan"
        rest = {plans[(c, eb)]["path"] for c in CS.CASES if c[2][0] == "fiber" and c[1] != (8200, 3)}
        assert rest != {0, 1, 2, 3}, "(8200,3) is listed for a path no other fiber case reaches"
        ragged = [c for c in CS.CASES if c[2][0] == "slice" and plans[(c, eb)]["nchunk"] >= 2 and plans[(c, eb)]["last"] < plans[(c, eb)]["chunk"]]
        assert {c[2][1] for c in ragged} == {"x", "y", "z"} and len(ragged) >= 3, "three slice cases with two or more ragged chunks"
        for c in cases:
            assert plans[(c, eb)]["nseg"] == R.nseg(c[1], c[0], c[2])
    # the selection routes and the stores of the apply kernel
    ns = {c: R.nseg(c[1], c[0], c[2]) for c in cases}
    above = [c for c in CS.CASES if ns[c] > CS.SMALL_MAX]
    assert [ns[c] for c in above] == [CS.SMALL_MAX + 1], "one listed case, the first size above the cap, takes the search route by default"
    assert CS.SMALL_MAX in [ns[c] for c in CS.CASES], "no case has exactly the cap's number of segments"
    assert ns[CS.BIG_TIE] == 9216 > CS.CARD_CAP > CS.SMALL_MAX, "the big tie group must exceed CARD_CAP and go through the search"
    assert sorted(ns[c] for c in CS.CASES if c[2][0] == "slice") == [8, 8, 9, 10, 10, 10] and max(ns.values()) == 9216
    wide = [c for c in CS.CASES if c[1][0] % 4 == 0]
    assert ("identity", (32, 12, 8), ("fiber", "z")) in wide and ("identity", (30, 12, 8), ("fiber", "z")) not in wide
    assert any(c[0] == "D_x" and c[1][0] % 4 == 0 for c in CS.CASES), "no case mixes 16-byte stores with the pad column of D_x"
    assert ("D_z", (4, 5, 2), ("fiber", "z")) in CS.CASES and plans[(("D_z", (4, 5, 2), ("fiber", "z")), 4)]["L"] == 1


def test_the_julia_binding_maps_the_tag(sipx):
    src = open(os.path.join(ROOT, "julia", "SipxPARSDMM.jl"), encoding="utf-8").read()
    assert "const SIPX_PROJ_CARD_GROUPS = 20" in src and 'st == "card_groups"' in src
    assert "return (SIPX_PROJ_CARD_GROUPS, 0.0, Float64(c.max), nothing_[3:5]...)" in src
    for text in (sipx.host.CARDG_ONE_BLOCK, sipx.host.CARDG_NEEDS_MODE, sipx.host.CARDG_BAD_K):
        assert 'error("' + text + '")' in src, text
