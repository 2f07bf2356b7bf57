"""The l2,1 ball over fibers or slices without a GPU: the numpy reference (tests/l21_groups_ref.py) against the properties of a
projection, csrc/l21_groups.h on the CPU (tests/l21_groups/rule_driver.cpp, compiled by hipcc; the program makes no HIP call) -- the plan
of the norms launch for the cases of tests/test_gpu_l21_groups.py, the serial rule against the Python emulation bit for bit -- the host
descriptors and refusals, and the refusals that must not move."""
import copy
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import l1_exact, seg_norms_ref
from tests import l21_groups_ref as G
from tests import l21_weighted_ref as R
from tests.test_gpu_l21_groups import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "setintersectionprojection.jl_amd", "csrc")
COMPUTE_UNITS = 256


def _heavy(rng, M):
    return rng.standard_normal(M) * np.exp(rng.standard_normal(M))


# ---- the reference is a projection -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op,n,mode", [("identity", (7, 5), ("fiber", "x")), ("D_z", (6, 4, 5), ("fiber", "z")),
                                       ("D_x", (6, 4, 3), ("slice", "z")), ("identity", (5, 4, 6), ("slice", "x"))])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("frac", [0.9, 0.5, 0.05])
def test_reference_is_the_projection(op, n, mode, weighted, frac):
    TF = np.float64
    eps = float(np.finfo(TF).eps)
    rng = np.random.default_rng(31 + sum(n) + len(op))
    M = G.rows(n, op)
    v = _heavy(rng, M).astype(TF)
    ns = G.nseg(n, op, mode)
    w = rng.uniform(0.5, 2.0, ns) if weighted else np.ones(ns)
    if weighted:
        w[1] = 0.0
    b = TF(frac * G.norm(v, n, op, mode, w))
    y = G.project(v, n, op, mode, w if weighted else None, b)
    assert y is not v
    assert abs(G.norm(y, n, op, mode, w) - float(b)) <= 8 * eps * float(b)
    for k in range(60):                 # <v - y, z - y> <= 0 for every z of the ball, up to the rounding of y
        z = _heavy(rng, M)
        nz = G.norm(z, n, op, mode, w)
        z *= (1.0 if k % 5 == 0 else rng.random()) * float(b) * (1 - 8 * eps) / nz
        vi = float(np.dot(v - y, z - y))
        assert vi <= 64 * eps * np.linalg.norm(v - y) * np.linalg.norm(z - y), (k, vi)
    if weighted:
        idx = G.segments(n, op, mode)[1]
        assert np.array_equal(y[idx], v[idx])
    assert G.project(v, n, op, mode, w, TF(2 * G.norm(v, n, op, mode, w))) is v


def test_reference_example_of_the_rule():
    """g = (3, 4, 5), tau = 6: the projection is (1, 2, 3) with theta = 2; the capped l1 rule would give theta = 1.5 and a sum of 7.5."""
    g = np.array([3.0, 4.0, 5.0])
    assert R.exact_theta(g, np.ones(3), 6.0) == 2.0
    v = np.array([3.0, 0.0, 0.0, 4.0, 5.0, 0.0])            # (2, 3): the fibers along x have norms 3, 4, 5
    y = G.project(v, (2, 3), "identity", ("fiber", "x"), None, 6.0)
    assert np.allclose(y, [1.0, 0.0, 0.0, 2.0, 3.0, 0.0], rtol=1e-15, atol=0)


# ---- csrc/l21_groups.h on the CPU --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    hipcc = shutil.which("hipcc") or shutil.which("hipcc", path=os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin"))
    assert hipcc, "hipcc not found"
    exe = str(tmp_path_factory.mktemp("l21_groups") / "rule_driver")
    r = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                        "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "l21_groups", "rule_driver.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _run(driver, lines):
    r = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True)
    out = r.stdout.splitlines()
    assert r.returncode == 0 and out and out[-1] == "ok", "\n".join(k for k in out if k.startswith("FAIL"))[:4000] + r.stderr
    return out


def _plan_line(op, n, mode):
    n3 = tuple(n) + (1,) * (3 - len(n))
    opdir = -1 if op == "identity" else {"D_x": 0, "D_y": 1, "D_z": len(n) - 1}[op]
    return f"plan {len(n)} {n3[0]} {n3[1]} {n3[2]} {opdir} {1 if mode[0] == 'fiber' else 2} {seg_norms_ref.axis_of(n, mode)}"


def _plans(driver, cases):
    rows = [k.split() for k in _run(driver, [_plan_line(*c) for c in cases]) if k.startswith("plan ")]
    assert len(rows) == 2 * len(cases)
    out = {}
    for i, c in enumerate(cases):
        for j, eb in enumerate((4, 8)):
            row = rows[2 * i + j]
            p = {row[q]: int(row[q + 1]) for q in range(1, len(row), 2)}
            assert p["bytes"] == eb
            out[(c, eb)] = p
    return out


def test_plan_of_the_gpu_cases(driver):
    plans = _plans(driver, CASES)
    for eb in (4, 8):
        fib = [plans[(c, eb)] for c in CASES if c[2][0] == "fiber"]
        assert all(p["slices"] == 0 for p in fib)
        assert {p["path"] for p in fib} == {0, 1, 2, 3}, "the fiber cases miss a path of seg_norm_plan"
        assert any(p["F"] > 1 and p["tiles_ragged"] for p in fib), "no fiber case has a ragged last tile"
        assert all(p["nseg"] == G.nseg(c[1], c[0], c[2]) and p["L"] == len(G.segments(c[1], c[0], c[2])[0])
                   for c in CASES for p in [plans[(c, eb)]])
        for d in "xyz":
            sl = [plans[(c, eb)] for c in CASES if c[2] == ("slice", d)]
            assert sl and all(p["slices"] == 1 for p in sl)
            assert any(p["nchunk"] >= 2 and p["last"] < p["chunk"] for p in sl), f"slice {d}: no case with a ragged last chunk"
        one = plans[(("identity", (32, 12, 8), ("slice", "z")), eb)]
        assert one["nchunk"] == 1 and one["L"] == 384 and one["vw"] == 16 // eb
        sx = plans[(("identity", (10, 96, 96), ("slice", "x")), eb)]
        assert sx["F"] == 16 and sx["vw"] == 1 and sx["tiles_ragged"] == 1, "slice x: tiles of neighbouring slices"
        # every workgroup of a slice plan owns one (tile, chunk): the grid is never bounded by the number of slices alone
        for c in CASES:
            p = plans[(c, eb)]
            if p["slices"]:
                assert p["grid"] == -(-p["nseg"] // p["F"]) * p["nchunk"] and p["nchunk"] == -(-p["L"] // p["chunk"])


def test_plan_fills_the_device_where_seg_norm_gives_a_slice_to_one_workgroup(driver):
    big = ("identity", (1024, 1024, 8), ("slice", "z"))
    p = _plans(driver, [big])[(big, 4)]
    assert p["nseg"] == 8 and p["grid"] >= 8 + COMPUTE_UNITS, p
    assert p["grid"] == 8 * p["nchunk"] and p["chunk"] * 4 == 20 * 1024


def _hex(x):
    return float(x).hex()


def _rule_cases(TF):
    rng = np.random.default_rng(47)
    out = []
    for L in (1, 3, 10, 35, 210, 1200):
        for weighted in (False, True):
            for frac in (0.9, 0.5, 0.05):
                g = np.abs(_heavy(rng, L)).astype(TF)
                w = (1.0 / (1.0 + np.abs(_heavy(rng, L)))).astype(TF)
                if L > 3:
                    w[rng.random(L) < 0.1] = 0.0
                    g[2] = 0.0
                ww = w if weighted else np.ones(L, TF)
                tau = TF(frac * float(np.sum(ww.astype(np.float64) * g.astype(np.float64))))
                if tau > 0:
                    out.append((g, w if weighted else None, tau))
    # adversarial: all groups equal and active, nearly equal, inside, all weights zero, the ties of the GPU test
    out.append((np.full(64, 2.0, TF), None, TF(64.0)))
    out.append(((1.0 + 0.2 * rng.random(500)).astype(TF), None, TF(250.0)))
    out.append((np.abs(_heavy(rng, 40)).astype(TF), None, TF(1e6)))
    out.append((np.abs(_heavy(rng, 40)).astype(TF), np.zeros(40, TF), TF(1e-3)))
    gt = np.array([5, 7, 1, 2, 0.5] * 7, TF)
    wt = np.array([2, 1, 1, 2, 1] * 7, TF)
    out.append((gt, wt, TF(84)))
    out.append((np.array([3, 4, 5], TF), None, TF(6)))
    return out


def _run_rule(driver, TF, cases):
    tag = "f" if TF == np.float32 else "d"
    lines = []
    for g, w, tau in cases:
        ww = np.ones(len(g), TF) if w is None else w
        lines.append(f"r {tag} {_hex(tau)} {len(g)} {0 if w is None else 1} " + " ".join(f"{_hex(a)} {_hex(b)}" for a, b in zip(g, ww)))
    got = [k.split()[1:] for k in _run(driver, lines) if k.startswith("r ")]
    assert len(got) == len(cases)
    return [(int(r[0]), TF(float.fromhex(r[1])), TF(float.fromhex(r[2])), int(r[3]), np.array([float.fromhex(x) for x in r[4:]]).astype(TF))
            for r in got]


@pytest.mark.parametrize("TF", [np.float32, np.float64])
def test_header_rule_equals_the_emulation_bit_for_bit(driver, TF):
    cases = _rule_cases(TF)
    got = _run_rule(driver, TF, cases)
    for (g, w, tau), (need, theta, asum, passes, f) in zip(cases, got):
        ww = np.ones(len(g), TF) if w is None else w
        e_need, e_theta, e_asum, e_passes = R.emulate_search(g, ww, tau)
        assert (need, passes) == (e_need, e_passes), (len(g), need, passes, e_need, e_passes)
        assert l1_exact.same_bits(np.array([theta, asum]), np.array([e_theta, e_asum])), (len(g), theta, e_theta)
        if need:
            _, ef = R.emulate_apply(np.ones((len(g), 1), TF), g, ww, theta)
            ef = np.where(R.clean(ww) > 0, ef, TF(1)).astype(TF)
        else:
            ef = np.ones(len(g), TF)
        assert l1_exact.same_bits(f, ef), len(g)
        if need:                        # the header's theta against the exact threshold (tests/test_l21_weighted_cpu.py's tolerance)
            th = R.exact_theta(g, ww, tau)
            tol = (2.0 ** -52 + len(g) * 2.0 ** -64) * th + (0.5 * l1_exact.ulp(th, TF) if TF == np.float32 else 0.0)
            assert abs(float(theta) - th) <= tol, (len(g), float(theta), th)
    # g = (3, 4, 5), tau = 6: theta = 2 exactly, not the capped rule's 1.5; the factors give (1, 2, 3)
    need, theta, _, _, f = got[-1]
    assert need == 1 and float(theta) == 2.0
    assert l1_exact.same_bits(f, np.array([TF(1) / TF(3), TF(2) / TF(4), TF(3) / TF(5)], TF))
    # the ties: theta = 1 exactly, groups on it are zeroed
    need, theta, _, _, f = got[-2]
    assert need == 1 and float(theta) == 1.0 and np.all(f.reshape(7, 5)[:, 2:] == 0) and np.all(f.reshape(7, 5)[:, :2] > 0)
    # all equal: every group active, theta = (S - tau) / n
    assert float(got[-6][1]) == 1.0 and np.all(got[-6][4] == 0.5)


@pytest.mark.parametrize("TF", [np.float32, np.float64])
def test_no_weights_give_the_bits_of_ones(driver, TF):
    cases = [c for c in _rule_cases(TF) if c[1] is None]
    a = _run_rule(driver, TF, cases)
    b = _run_rule(driver, TF, [(g, np.ones(len(g), TF), tau) for g, _, tau in cases])
    for x, y in zip(a, b):
        assert x[0] == y[0] and x[3] == y[3] and l1_exact.same_bits(np.array([x[1], x[2]]), np.array([y[1], y[2]]))
        assert l1_exact.same_bits(x[4], y[4])


# ---- host side ---------------------------------------------------------------------------------------------------------------------------
def test_descriptor_and_data_len(sipx):
    g3 = sipx.compgrid((25.0, 25.0, 25.0), (16, 12, 8))
    g2 = sipx.compgrid((25.0, 6.0), (16, 12))
    assert sipx.host.PROJ["l21_groups"] == 16
    for TF in (np.float32, np.float64):
        for op, g, mode, md, ns in (("D_z", g3, ("fiber", "z"), (1, 2), 192), ("D_z", g3, ("slice", "z"), (2, 2), 7),
                                    ("identity", g3, ("slice", "x"), (2, 0), 16), ("D_x", g3, ("fiber", "y"), (1, 1), 15 * 8),
                                    ("identity", g2, ("fiber", "x"), (1, 0), 12), ("D_z", g2, ("fiber", "z"), (1, 1), 16)):
            w = np.linspace(0.0, 2.0, ns)                         # float64: setup_constraints takes it to the working precision
            whole = ("tensor", "") if len(g.n) == 3 else ("matrix", "")
            c = [sipx.set_definitions("bounds", "identity", 1.0, 2.0, whole), sipx.set_definitions("l21_groups", op, 0.0, 3.5, mode, weights=w),
                 sipx.set_definitions("l21_groups", op, 0.0, 3.5, mode)]
            P, A, prop = sipx.setup_constraints(copy.deepcopy(c), g, TF)
            assert prop.tag[1] == ("l21_groups", op, mode[0], mode[1]) and prop.ncvx == [False] * 3
            assert P[1].weighted and P[1].lb.dtype == TF and P[1].ub is None and np.array_equal(P[1].lb, w.astype(TF))
            assert P[1].data_len(A[1]) == ns and P[1].nseg(A[1]) == ns and P[2].data_len(A[2]) is None and not P[2].weighted
            d = P[1].desc(A[1].kind, prop.ncvx[1])
            assert (d.proj, d.mode, d.dir, d.pmax, d.reserved) == (16, md[0], md[1], 3.5, ns) and d.lb is not None and d.ub is None
            d = P[2].desc(A[2].kind, prop.ncvx[2])
            assert (d.proj, d.mode, d.dir, d.pmax, d.reserved) == (16, md[0], md[1], 3.5, 0) and d.lb is None and d.ub is None
            # the automatic context cache refuses lists that carry weights, and takes the set without them
            opt = sipx.PARSDMM_options()
            opt.FL = TF
            assert sipx.host._context_key(np.zeros(1, TF), None, A, prop, P, g, opt, None) is None
            assert sipx.host._context_key(np.zeros(1, TF), None, [A[0], A[2]], prop, [P[0], P[2]], g, opt, None) is not None
    for s in ("sipx_l21_groups_norm", "sipx_l21_groups_norm_dev"):
        assert s in sipx.EXPORTED_SYMBOLS
    assert callable(sipx.l21_groups_norm)


def test_host_refusals(sipx):
    TF = np.float32
    g3 = sipx.compgrid((25.0, 25.0, 25.0), (16, 12, 8))
    g2 = sipx.compgrid((25.0, 6.0), (16, 12))

    def P(op, mode, weights=None, g=g3, mx=1.0, custom=((), False)):
        return sipx.Projector(sipx.set_definitions("l21_groups", op, 0.0, mx, mode, custom, weights), g, TF)
    with pytest.raises(sipx.SipxError, match=r"needs a fiber or slice mode.*use the l2 set"):
        P("D_z", ("tensor", ""))
    with pytest.raises(sipx.SipxError, match=r"needs a fiber or slice mode.*use the l2 set"):
        P("identity", ("matrix", ""), g=g2)
    for op in ("TV", "D3D", "TV_xy", "D_xz"):
        with pytest.raises(sipx.SipxError, match="groups the range of a one-block operator: TD_OP must be the identity, D_x, D_y or D_z"):
            P(op, ("fiber", "z"))
    for op in ("DFT", "DCT", "wavelet", "curvelet"):
        with pytest.raises(sipx.SipxError, match=r"\(l21_groups\) takes no transform"):
            P(op, ("fiber", "z"))
    import scipy.sparse as sp
    with pytest.raises(sipx.SipxError, match=r"\(l21_groups\) takes no custom operator"):
        P("identity", ("fiber", "z"), custom=(sp.identity(16 * 12 * 8, format="csc", dtype=TF), False))
    with pytest.raises(sipx.SipxError, match=r"for 2D models, the mode of application for l21_groups sets needs to be \(fiber,x\) or \(fiber,z\)"):
        P("identity", ("slice", "x"), g=g2)
    with pytest.raises(sipx.SipxError, match="direction must be one of"):
        P("identity", ("fiber", "y"), g=g2)
    for mx in (0.0, -1.0, float("nan")):
        with pytest.raises(sipx.SipxError, match="Radius of L1 ball is negative"):
            P("D_z", ("fiber", "z"), mx=mx)
    with pytest.raises(sipx.SipxError, match="takes one radius"):
        P("D_z", ("fiber", "z"), mx=np.ones(192, TF))
    # the weights: checked like those of the l2,1 sets on TV, naming both lengths and what a segment is
    w = np.ones(192, TF)
    with pytest.raises(sipx.SipxError, match=r"l21_groups weights have shape \(191,\): \(192,\) is needed -- one per segment, a segment being a "
                                             r"fiber along dimension 3 of the array of shape \(16, 12, 7\)"):
        P("D_z", ("fiber", "z"), w[:-1])
    with pytest.raises(sipx.SipxError, match=r"shape \(192,\): \(7,\) is needed -- one per segment, a segment being a slice orthogonal to dimension 3"):
        P("D_z", ("slice", "z"), w)
    with pytest.raises(sipx.SipxError, match="l21_groups weights have dtype float64: not the working precision"):
        P("D_z", ("fiber", "z"), w.astype(np.float64))
    with pytest.raises(sipx.SipxError, match="l21_groups weights must be a numpy array, not list"):
        P("D_z", ("fiber", "z"), list(w))
    for bad, at in ((-1.0, 5), (np.nan, 0), (np.inf, 77)):
        wb = w.copy()
        wb[at] = wb[150] = bad
        with pytest.raises(sipx.SipxError, match=rf"the weighted l2,1 ball \(l21_groups\): weight {at} is negative, NaN or infinite"):
            P("D_z", ("fiber", "z"), wb)
    assert P("D_z", ("fiber", "z"), np.zeros(192, TF)).weighted, "all weights zero is a set"
    # a Minkowski component, an operator the set was not built for
    pr = P("D_z", ("fiber", "z"))
    with pytest.raises(sipx.SipxError, match=r"\(l21_groups\) takes no Minkowski component"):
        pr.check_rows(sipx.TDOperator("D_z", g3, TF, component=1))
    with pytest.raises(sipx.SipxError, match="one-block operator"):
        pr.check_rows(sipx.TDOperator("TV", g3, TF))
    # the stand-alone projector acts on the M-vector of the operator's range
    with pytest.raises(sipx.SipxError, match=r"projects a vector of the D_z range: 1344 entries on this grid, 1536 given"):
        pr(np.zeros(1536, TF))
    # the observer
    x = np.zeros(1536, TF)
    with pytest.raises(sipx.SipxError, match="one-block operator"):
        sipx.l21_groups_norm(x, g3, "TV", ("fiber", "z"))
    with pytest.raises(sipx.SipxError, match="needs a fiber or slice mode"):
        sipx.l21_groups_norm(x, g3, "D_z", ("tensor", ""))
    with pytest.raises(sipx.SipxError, match="weights has 191 entries, 192 are needed"):
        sipx.l21_groups_norm(x, g3, "D_z", ("fiber", "z"), weights=w[:-1])
    wb = w.copy()
    wb[9] = -0.5
    with pytest.raises(sipx.SipxError, match="weight 9 is negative, NaN or infinite"):
        sipx.l21_groups_norm(x, g3, "D_z", ("fiber", "z"), weights=wb)
    with pytest.raises(sipx.SipxError, match="x must be a Float32 or Float64"):
        sipx.l21_groups_norm(x.astype(np.int32), g3, "D_z", ("fiber", "z"))


def test_constraint2coarse_refuses_the_set(sipx):
    g = sipx.compgrid((1.0, 1.0), (64, 48))
    c = [sipx.set_definitions("l21_groups", "D_z", 0.0, 12.0, ("fiber", "z"))]
    with pytest.raises(sipx.SipxError, match=r"multilevel: the l2,1 ball over fibers or slices \(l21_groups\) has no rule that takes its radius"):
        sipx.constraint2coarse(c, g, 2)


def test_existing_refusals_have_not_moved(sipx):
    TF = np.float32
    g3 = sipx.compgrid((25.0, 25.0, 25.0), (16, 12, 8))
    w = np.ones(1536, TF)

    def P(st, op, mode, weights=None):
        return sipx.Projector(sipx.set_definitions(st, op, 0.0, 1.0, mode, weights=weights), g3, TF)
    for op in ("identity", "D_x", "D_y", "D_z"):
        with pytest.raises(sipx.SipxError) as e:
            P("l21", op, ("tensor", ""))
        assert str(e.value) == "the l2,1 ball acts on the range of the TV operator: TD_OP must be TV (D2D, D3D)" == sipx.host.L21_NEEDS_TV
        with pytest.raises(sipx.SipxError) as e:
            P("l21", op, ("fiber", "z"))
        assert str(e.value) == sipx.host.L21_NEEDS_TV
    with pytest.raises(sipx.SipxError) as e:
        P("l21", "TV", ("fiber", "z"))
    assert str(e.value) == "the l2,1 ball applies to the whole array (mode matrix/tensor)" == sipx.host.L21_WHOLE_ONLY
    for st, op in (("l1", "TV"), ("l2", "identity"), ("bounds", "identity"), ("cardinality", "D_z")):
        with pytest.raises(sipx.SipxError) as e:
            P(st, op, ("tensor", ""), w)
        assert str(e.value) == f"set type '{st}' takes no weights: " + sipx.host.L21_WEIGHTS_WHERE
        assert str(e.value).startswith(f"set type '{st}' takes no weights: weights belong to the l2,1 sets on the whole array -- ")
    with pytest.raises(sipx.SipxError, match="per frame takes no weights"):
        P("l21", "TV_xy", ("slice", "z"), w)
    with pytest.raises(KeyError):
        sipx.host.PROJ["l21_fibers"]
    assert sipx.host.PROJ["l21"] == 14 and sipx.host.PROJ["l21_joint"] == 15
    with pytest.raises(sipx.SipxError, match="set type 'l21_fibers' is not part of this engine"):
        P("l21_fibers", "D_z", ("fiber", "z"))
