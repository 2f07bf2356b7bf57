"""The l2,0 sets on TV / TV_xy without a GPU: the numpy reference (tests/l20_ref.py) against brute force on tiny grids and against the
selection contract of tests/card_exact.py; csrc/l20.h on the CPU (tests/l20/rule_driver.cpp, a stand-alone program built by the host
compiler, with -fsanitize=address,undefined where the compiler has the runtimes) -- the serial selection and the per-frame radix select
held to an argsort, the keep rule to card_exact.check_card_output with tie groups across the k-th place --; the plans of the cases of
tests/test_gpu_l20.py; the host descriptors and the refusals, word for word against the header."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import card_exact, l21_joint_ref
from tests import l20_cases as CS
from tests import l20_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "setintersectionprojection.jl_amd", "csrc")
PRECISIONS = [np.float32, np.float64]


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------
def test_reference_example():
    """(2, 2) grid, TV: rows [D_z: (0,0)->(0,1), (1,0)->(1,1); D_x: (0,0)->(1,0), (0,1)->(1,1)].  Groups: p0 = {v0, v2}, p1 = {v1},
    p2 = {v3}, p3 = {}."""
    n, v = (2, 2), np.array([3.0, -5.0, 4.0, -0.0])
    assert R.rows(n, "TV") == 4 and np.array_equal(R.members(n, "TV"), [[0, 2], [1, -1], [-1, 3], [-1, -1]])
    g = R.norms(v, n, "TV", "whole", np.float64)
    assert np.array_equal(g, [5.0, 5.0, 0.0, 0.0])
    assert np.array_equal(R.project(v, n, "TV", "whole", 1), [3.0, 0.0, 4.0, 0.0]), "the tie goes to the lower point index"
    assert R.project(v, n, "TV", "whole", 2) is v and R.project(v, n, "TV", "whole", 9) is v
    y = R.project(v, n, "TV", "whole", 1)
    assert not np.signbit(y[3]), "the zero group is dropped and written +0 once anything is dropped"
    assert R.project(y, n, "TV", "whole", 1) is y, "the projection of a projection drops something"


@pytest.mark.parametrize("TF", PRECISIONS)
def test_reference_against_brute_force_on_tiny_grids(TF):
    rng = np.random.default_rng(5)
    for op, n, form in [("TV", (3, 4), "whole"), ("TV", (3, 2, 3), "whole"), ("TV_xy", (3, 2, 3), "whole"), ("TV_xy", (3, 3, 2), "frames"),
                        ("TV_xy", (3, 2, 3), "joint")]:
        ng = R.ngroups(n, op, form)
        for trial in range(3):
            v = rng.integers(-3, 4, R.rows(n, op)).astype(TF)            # small integers: many ties, many zero groups
            budgets = [1, 2, ng // 2, ng - 1, ng]
            if form == "frames":
                budgets.append(rng.integers(1, ng + 1, n[2]))
            for k in budgets:
                assert np.array_equal(R.project(v, n, op, form, k), R.brute_force(v, n, op, form, k)), (op, n, form, k, trial)


@pytest.mark.parametrize("TF", PRECISIONS)
def test_reference_selection_is_the_contract_on_the_key(TF):
    for op, n, form in [c for c in CS.CASES if int(np.prod(c[1])) < 3000]:
        v = CS.mixed_input(op, n, form, TF)
        g = R.norms(v, n, op, form, TF)
        ng = R.ngroups(n, op, form)
        for k in CS.ks(ng):
            keep = R.kept_points(g, n, op, form, k)
            y = R.project(v, n, op, form, k)
            G = R.members(n, op)
            for p in range(G.shape[0]):
                idx = G[p][G[p] >= 0]
                assert np.array_equal(y[idx], v[idx]) if keep[p] else not y[idx].any()
            pools = [g] if form != "frames" else [g[f * ng:(f + 1) * ng] for f in range(n[2])]
            kp = keep if form != "joint" else keep[:ng]
            for f, pool in enumerate(pools):
                kf = kp[f * ng:(f + 1) * ng] if form == "frames" else kp
                card_exact.check_card_output(pool, np.where(kf, pool, TF(0)).astype(TF), k)


# ---- csrc/l20.h on the CPU ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    exe = str(tmp_path_factory.mktemp("l20") / "rule_driver")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "l20", "rule_driver.cpp"), "-o", exe]
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
    """[(g, k)]: random keys with zeros, tie groups straddling the k-th place, k = 1, k = n - 1, k >= n, all-zero g, one group."""
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
    five = np.array([np.hypot(3, 4), 5, 2, np.sqrt(TF(25)), 1, 5, 0, 5], TF)     # (3,4), (5,0), (0,5): different members, equal norm bits
    out += [(five, k) for k in (1, 2, 3, 4, 5)]
    out += [(np.full(50, 2.5, TF), k) for k in (1, 17, 49, 50)]                   # one tie group: the lowest k indices
    sub = np.nextafter(TF(0), TF(1))
    out += [(np.array([sub, 2 * sub, sub, 0, 2 * sub, sub], TF), k) for k in (1, 2, 3, 4)]      # the smallest subnormals
    out += [(np.array([np.finfo(TF).max, 1, np.finfo(TF).max], TF), 1)]
    near = np.array([1.0, np.nextafter(TF(1), TF(2)), np.nextafter(TF(1), TF(0)), 1.0, 256.0, np.nextafter(TF(256), TF(0))], TF)
    out += [(near, k) for k in (1, 2, 3, 4, 5)]                                   # neighbours in the last radix byte and across a byte
    out += [(np.zeros(9, TF), 1), (np.zeros(9, TF), 9), (np.array([3.0], TF), 1), (np.array([0.0], TF), 1), (np.array([3.0], TF), 4)]
    return out


@pytest.mark.parametrize("what", ["s", "r"])
@pytest.mark.parametrize("TF", PRECISIONS)
def test_serial_and_radix_selection_are_the_stable_argsort(driver, TF, what):
    """`s`: l20_select_serial (whole array, joint); `r`: l20_frame_select, the radix select of k_l20_frames."""
    cases = _rule_cases(TF)
    p = "f" if TF == np.float32 else "d"
    out = _run(driver, [f"{what} {p} {k} {len(g)} " + " ".join(_hex(x) for x in g) for g, k in cases])
    assert len(out) == len(cases)
    straddled = 0
    for (g, k), row in zip(cases, out):
        f = row.split()
        assert f[0] == what
        need, tau, cut, word = int(f[1]), TF(float.fromhex(f[2])), int(f[3]), f[4]
        keep = np.array([c == "1" for c in word])
        card_exact.check_card_output(g, np.where(keep, g, TF(0)).astype(TF), k)
        order = np.argsort(-g.astype(np.float64), kind="stable")
        nnz = int((g > 0).sum())
        assert need == (1 if nnz > k and k < len(g) else 0)
        if need:
            want = np.zeros(len(g), bool)
            want[order[:k]] = True
            assert np.array_equal(keep, want), (g, k)
            assert tau > 0 and tau == g[order[k - 1]] and cut == order[k - 1] and int(keep.sum()) == k
            straddled += card_exact.straddles(g, k)[0]
        else:
            assert tau == 0 and cut == 2 ** 63 - 1 and keep.all()
        assert np.array_equal(keep, R.kept(g, k))
    assert straddled >= 8, "no tie group straddles the k-th place"


def test_key_and_membership(driver):
    asks = ["m 0 5", "m 3 5", "m 4 5", "m 0 1", "g f 2 1 0x1.8p+1 1 0x1p+2", "g f 2 1 0x1.8p+1 0 0x1p+2", "g d 3 1 0x1p+0 1 0x1p+1 1 0x1p+1",
            "g d 3 0 0x1p+0 0 0x1p+1 0 0x1p+1", "g f 2 1 0x1p-80 1 0x1p-80"]
    out = _run(driver, asks)
    assert out[:4] == ["m 1", "m 1", "m 0", "m 0"]
    vals = [float.fromhex(r.split()[1]) for r in out[4:]]
    assert vals[:4] == [5.0, 3.0, 3.0, 0.0]
    assert vals[4] == float(np.float32(np.sqrt(2.0 ** -159))), "the squares are taken in float64: no underflow in Float32"


def _constants():
    """name -> text of every `constexpr const char* L20_...` of the header (adjacent literals joined)."""
    src = open(os.path.join(CSRC, "l20.h"), encoding="utf-8").read()
    out = {}
    for m in re.finditer(r"constexpr const char\* (L20_[A-Z0-9_]+) = ((?:\s*\"(?:[^\"\\]|\\.)*\")+);", src):
        out[m.group(1)] = "".join(re.findall(r"\"((?:[^\"\\]|\\.)*)\"", m.group(2))).replace('\\"', '"')
    return out


def test_refusals_are_worded_once(sipx):
    c = _constants()
    assert set(c) == {"L20_NEEDS_TV", "L20_JOINT_ROUTE", "L20_MODES", "L20_NO_TRANSFORM", "L20_NO_MINKOWSKI", "L20_NO_WEIGHTS", "L20_K_VECTOR",
                      "L20_NO_SET_DATA", "L20_SET_DATA_UB", "L20_SHARDED", "L20_NO_COARSE", "L20_BAD_K", "L20_K_INEXACT", "L20_TOO_LARGE"}
    for name, text in c.items():
        assert getattr(sipx.host, name) == text, name
    # every text names a way out
    for name, way in [("L20_NEEDS_TV", "use the cardinality set"), ("L20_JOINT_ROUTE", "(\"l20\", \"TV_xy\")"), ("L20_MODES", "use card_groups"),
                      ("L20_NO_TRANSFORM", "use the cardinality set behind the transform"), ("L20_NO_MINKOWSKI", "the sum of the components"),
                      ("L20_NO_WEIGHTS", "use the l21 set with weights"), ("L20_K_VECTOR", "pass a scalar"),
                      ("L20_NO_SET_DATA", "a vector of n3 budgets"), ("L20_SET_DATA_UB", "its ub"), ("L20_SHARDED", "use a single process"),
                      ("L20_NO_COARSE", "one level"), ("L20_BAD_K", "use bounds"), ("L20_K_INEXACT", "use Float64"),
                      ("L20_TOO_LARGE", "split the array")]:
        assert way in c[name], name


def test_k_is_checked_alike_in_the_header_and_on_the_host(driver, sipx):
    H = sipx.host
    asks = [("f", 1.0, 7, "ok"), ("f", 0.0, 7, H.L20_BAD_K), ("f", -2.0, 7, H.L20_BAD_K), ("f", 2.5, 7, H.L20_BAD_K),
            ("f", float("nan"), 7, H.L20_BAD_K), ("d", float("inf"), 7, H.L20_BAD_K),
            ("f", 2.0 ** 24 + 1, 2 ** 25, H.L20_K_INEXACT), ("f", 2.0 ** 24, 2 ** 25, "ok"), ("d", 2.0 ** 24 + 1, 2 ** 25, "ok"),
            ("f", 2.0 ** 24 + 1, 1000, "ok")]                      # (k >= the number of groups: every group stays, k is not read)
    out = _run(driver, [f"k {p} {_hex(k) if np.isfinite(k) else k} {ns}" for p, k, ns, _ in asks])
    for (p, k, ns, want), row in zip(asks, out):
        assert row == "k " + want, (p, k, ns, row)
    g = sipx.compgrid((1.0, 1.0, 1.0), (16, 12, 8))
    for k, text in [(0, H.L20_BAD_K), (-1, H.L20_BAD_K), (1.5, H.L20_BAD_K), (float("nan"), H.L20_BAD_K), (float("inf"), H.L20_BAD_K),
                    (True, H.L20_BAD_K)]:
        for st, op, mode in [("l20", "TV", ("tensor", "")), ("l20", "TV_xy", ("slice", "z")), ("l20_joint", "TV_xy", ("tensor", ""))]:
            with pytest.raises(sipx.SipxError) as e:
                sipx.Projector(sipx.set_definitions(st, op, 0.0, k, mode), g, np.float32)
            assert str(e.value) == text, (k, st)
    with pytest.raises(sipx.SipxError) as e:
        sipx.Projector(sipx.set_definitions("l20", "TV_xy", 0.0, [3, 0.5, 2, 2, 2, 2, 2, 2], ("slice", "z")), g, np.float32)
    assert str(e.value) == H.L20_BAD_K
    big = sipx.compgrid((1.0, 1.0, 1.0), (8192, 4096, 2))        # 2^26 points, 2^25 pixels
    for st, op, mode in [("l20", "TV", ("tensor", "")), ("l20", "TV_xy", ("slice", "z")), ("l20_joint", "TV_xy", ("tensor", ""))]:
        with pytest.raises(sipx.SipxError) as e:
            sipx.Projector(sipx.set_definitions(st, op, 0.0, 2 ** 24 + 1, mode), big, np.float32)
        assert str(e.value) == H.L20_K_INEXACT
        assert sipx.Projector(sipx.set_definitions(st, op, 0.0, 2 ** 24 + 1, mode), big, np.float64).pmax == 2.0 ** 24 + 1
    # through setup_constraints, which rounds the scalars of other sets to TF when min is a float: k must reach the check unrounded
    for lo in (0, 0.0, np.float32(0)):
        with pytest.raises(sipx.SipxError) as e:
            sipx.setup_constraints([sipx.set_definitions("l20", "TV", lo, 2 ** 24 + 1, ("tensor", ""))], big, np.float32)
        assert str(e.value) == H.L20_K_INEXACT, lo
    P, _, _ = sipx.setup_constraints([sipx.set_definitions("l20", "TV", 0.0, 2 ** 24 + 1, ("tensor", ""))], g, np.float32)
    assert P[0].pmax == 2.0 ** 24 + 1, "k >= the number of groups keeps its value"


# ---- the host: descriptor, ncvx, refusals ------------------------------------------------------------------------------------------------------
def test_descriptor_and_ncvx(sipx):
    g = sipx.compgrid((1.0, 1.0, 1.0), (16, 12, 8))
    for TF in PRECISIONS:
        c = [sipx.set_definitions("bounds", "identity", 0.0, 1.0, ("tensor", "")), sipx.set_definitions("l20", "TV", 0, 50, ("tensor", "")),
             sipx.set_definitions("l20", "TV_xy", 0, 9, ("tensor", "")), sipx.set_definitions("l20", "TV_xy", 0, 7, ("slice", "z")),
             sipx.set_definitions("l20", "TV_xy", 0, np.arange(1, 9), ("slice", "z")), sipx.set_definitions("l20_joint", "TV_xy", 0, 11, ("tensor", ""))]
        P, A, prop = sipx.setup_constraints(c, g, TF)
        assert prop.ncvx == [False, True, True, True, True, True]
        assert prop.tag[1] == ("l20", "TV", "tensor", "") and prop.tag[3] == ("l20", "TV_xy", "slice", "z")
        d = P[1].desc("TV", True)
        assert (d.proj, d.pmin, d.pmax, d.mode, d.reserved, d.ncvx, d.transform) == (21, 0.0, 50.0, 0, 0, 1, 0) and not d.lb and not d.ub
        d = P[3].desc("TV_xy", True)
        assert (d.proj, d.pmax, d.mode, d.dir) == (21, 7.0, 2, 2) and not d.ub and P[3].data_len(A[3]) is None
        d = P[4].desc("TV_xy", True)
        assert (d.proj, d.mode, d.dir) == (21, 2, 2) and d.ub and not d.lb and P[4].data_len(A[4]) == 8
        assert P[4].ub.dtype == TF and np.array_equal(P[4].ub, np.arange(1, 9))
        d = P[5].desc("TV_xy", True)
        assert (d.proj, d.pmax, d.mode) == (22, 11.0, 0)
        assert P[1].data_len(A[1]) is None and P[5].data_len(A[5]) is None
    assert sipx.host.PROJ["l20"] == 21 and sipx.host.PROJ["l20_joint"] == 22
    assert {"sipx_tv_group_norms", "sipx_tv_group_norms_dev"} <= set(sipx.EXPORTED_SYMBOLS)
    assert "count_nonzero(g)" in sipx.tv_group_norms.__doc__


def test_host_refusals(sipx):
    H = sipx.host
    g3, g2 = sipx.compgrid((1.0, 1.0, 1.0), (16, 12, 8)), sipx.compgrid((1.0, 1.0), (16, 12))
    TF = np.float32

    def D(st="l20", op="TV", k=3, mode=("tensor", ""), **kw):
        return sipx.set_definitions(st, op, 0.0, k, mode, **kw)

    def refused(c, g, text):
        for build in (lambda: sipx.Projector(c, g, TF), lambda: sipx.setup_constraints([c], g, TF)):
            with pytest.raises(sipx.SipxError) as e:
                build()
            assert str(e.value) == text, (str(e.value), text)
    for op in ("identity", "D_x", "D_z", "D_xz"):
        refused(D(op=op), g2 if op == "D_xz" else g3, H.L20_NEEDS_TV)
    for op in ("TV", "D3D", "identity"):
        refused(D("l20_joint", op), g3, H.L20_JOINT_ROUTE)
    refused(D("l20_joint", "TV_xy", mode=("slice", "z")), g3, H.L20_JOINT_ROUTE)
    for op in ("DFT", "DCT", "wavelet"):
        refused(D(op=op), g3, H.L20_NO_TRANSFORM)
        refused(D("l20_joint", op), g3, H.L20_NO_TRANSFORM)
    import scipy.sparse as sp
    refused(D(custom_TD_OP=(sp.identity(16 * 12 * 8, format="csc", dtype=TF), False)), g3, H.L20_NEEDS_TV)
    for mode in (("fiber", "z"), ("fiber", "x"), ("slice", "x"), ("slice", "y")):
        refused(D(op="TV_xy", mode=mode), g3, H.L20_MODES)
    refused(D(op="TV", mode=("slice", "z")), g3, H.L20_MODES)
    refused(D(op="TV", mode=("fiber", "x")), g2, H.L20_MODES)
    refused(D(op="TV_xy"), g2, H.TV_XY_NEEDS_3D)
    refused(D(weights=np.ones(16 * 12 * 8, TF)), g3, H.L20_NO_WEIGHTS)
    refused(D("l20_joint", "TV_xy", weights=np.ones(16 * 12, TF)), g3, H.L20_NO_WEIGHTS)
    refused(D(k=np.full(8, 3.0)), g3, H.L20_K_VECTOR)
    refused(D(op="TV_xy", k=np.full(8, 3.0)), g3, H.L20_K_VECTOR)
    refused(D("l20_joint", "TV_xy", k=np.full(8, 3.0)), g3, H.L20_K_VECTOR)
    refused(D(op="TV_xy", k=np.full((8, 1), 3.0), mode=("slice", "z")), g3, H.L20_K_VECTOR)
    refused(D(), sipx.compgrid((1.0, 1.0, 1.0), (2048, 1024, 1024)), H.L20_TOO_LARGE)
    with pytest.raises(sipx.SipxError, match="l20 budgets per frame: max has 5 entries, n3 = 8"):
        P, A, _ = sipx.setup_constraints([D(op="TV_xy", k=np.full(5, 3.0), mode=("slice", "z"))], g3, TF)
        P[0].check_rows(A[0])
    # multilevel: no rule takes k to another grid
    for c in (D(), D("l20_joint", "TV_xy")):
        with pytest.raises(sipx.SipxError) as e:
            sipx.constraint2coarse([c], g3, (2, 2, 2))
        assert str(e.value) == H.L20_NO_COARSE
    # the observer refuses what the set refuses, before a context exists
    x = np.zeros(16 * 12 * 8, TF)
    for op, joint, text in [("D_z", False, H.L20_NEEDS_TV), ("DFT", False, H.L20_NO_TRANSFORM), ("TV", True, H.L20_JOINT_ROUTE)]:
        with pytest.raises(sipx.SipxError) as e:
            sipx.tv_group_norms(x, g3, op, joint)
        assert str(e.value) == text
    with pytest.raises(sipx.SipxError) as e:
        sipx.tv_group_norms(np.zeros(16 * 12, TF), g2, "TV_xy")
    assert str(e.value) == H.TV_XY_NEEDS_3D


# ---- the plans of the GPU cases ------------------------------------------------------------------------------------------------------------------
def _header_int(name, header):
    src = open(os.path.join(CSRC, header), encoding="utf-8").read()
    m = re.search(r"constexpr (?:int|long long) " + name + r" = ([^;]+);", src)
    assert m, name
    return int(eval(m.group(1).replace("ll", ""), {}))


def test_the_gpu_cases_reach_what_they_claim():
    assert _header_int("CARDG_SMALL_MAX", "card_groups.h") == CS.SMALL_MAX and _header_int("SEGN_LDS_BYTES", "seg_norm.h") == CS.LDS_BYTES
    assert card_exact.CAP == CS.CARD_CAP
    ng = {c: R.ngroups(c[1], c[0], c[2]) for c in CS.CASES + [CS.BIG_TIE]}
    # both widths of the apply kernel (16-byte stores need n1 % 4 == 0), in 2-D, 3-D, joint and per frame
    for sel in (lambda c: len(c[1]) == 2, lambda c: len(c[1]) == 3 and c[2] == "whole", lambda c: c[2] == "joint", lambda c: c[2] == "frames"):
        widths = {c[1][0] % 4 == 0 for c in CS.CASES if sel(c)}
        assert widths == {True, False}, "a form misses a store width"
    assert ("TV", (8, 6), "whole") in CS.CASES, "wide stores with the far face along x inside a vector"
    # both selection routes: the cap itself and the first size above it, and a 3-D case above it
    whole = sorted(ng[c] for c in CS.WHOLE)
    assert CS.SMALL_MAX in whole and CS.SMALL_MAX + 1 in whole and whole[-1] == 2880
    assert ng[CS.BIG_TIE] == 9216 > CS.CARD_CAP
    assert {ng[c] > CS.SMALL_MAX for c in CS.JOINT} == {False}, "the joint cases take the small route: the search route is forced for them"
    # both paths of the frame plan in each precision: L * bytes against the LDS budget
    for eb in (4, 8):
        paths = {c[1]: ng[c] * eb <= CS.LDS_BYTES for c in CS.FRAMES}
        assert set(paths.values()) == {True, False}
        assert paths[(64, 64, 3)] and not paths[(96, 96, 3)] and paths[(72, 64, 3)] == (eb == 4)
    assert 64 * 64 * 8 == CS.LDS_BYTES, "(64, 64, 3) fits exactly in Float64"
    # a joint chunk plan with two or more ragged chunks
    for eb in (4, 8):
        nchunk, zc = l21_joint_ref.plan(8 * 4, 67, eb)
        assert nchunk >= 2 and 67 - (nchunk - 1) * zc < zc, "(8, 4, 67): the last chunk is not ragged"
        assert l21_joint_ref.plan(4 * 3, 16, eb)[0] == 2 and l21_joint_ref.plan(33 * 20, 3, eb)[0] == 1


def test_the_julia_binding_maps_the_tags(sipx):
    src = open(os.path.join(ROOT, "julia", "SipxPARSDMM.jl"), encoding="utf-8").read()
    assert "const SIPX_PROJ_L20 = 21" in src and "const SIPX_PROJ_L20_JOINT = 22" in src and 'st == "l20"' in src and 'st == "l20_joint"' in src
    for text in (sipx.host.L20_NEEDS_TV, sipx.host.L20_JOINT_ROUTE, sipx.host.L20_MODES, sipx.host.L20_BAD_K):
        assert 'error("' + text.replace('"', '\\"') + '")' in src, text
