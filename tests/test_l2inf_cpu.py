"""The l2,inf ball -- every group norm at most c_p (csrc/l2inf.h) -- without a GPU: the numpy reference (tests/l2inf_ref.py) held to the
properties of a projection in its three layouts, the rule functions of the header (tests/l2inf/rule_driver.cpp, compiled by hipcc; the
program makes no HIP call) against a numpy emulation bit for bit, the descriptor rules of csrc/set_config.h through
tests/l2inf/config_driver.cpp, and the refusals of the front end and of the multilevel helpers."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from tests import l1_exact, l21_frames_ref, l21_ref
from tests import l2inf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "setintersectionprojection.jl_amd", "csrc")
BLOCKS = [1, 2, 3, 6, 8]


def _heavy(rng, M):
    return rng.standard_normal(M) * np.exp(rng.standard_normal(M))


def _layouts():
    """(name, idx, M, joint grid or None) of one small case per layout."""
    out = [("TV (7, 5)", R.layout_tv((7, 5)), l21_ref.rows((7, 5)), None),
           ("TV (5, 4, 3)", R.layout_tv((5, 4, 3)), l21_ref.rows((5, 4, 3)), None),
           ("TV_xy (5, 4, 3)", R.layout_tv_xy((5, 4, 3)), l21_frames_ref.rows((5, 4, 3)), None),
           ("joint (5, 4, 3)", R.layout_joint((5, 4, 3)), l21_frames_ref.rows((5, 4, 3)), (5, 4, 3))]
    for B in BLOCKS:
        out.append((f"stacked B {B}", R.layout_stacked(B * 17, B), B * 17, None))
    return out


# ---- the reference is the projection ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("TF", [np.float32, np.float64])
@pytest.mark.parametrize("form", ["scalar", "vector"])
def test_reference_is_the_projection(TF, form):
    """Feasible output, idempotent to the header's bound, and <v - P v, z - P v> <= rounding for feasible z."""
    u = float(np.finfo(TF).eps) / 2
    for case, (name, idx, M, jn) in enumerate(_layouts()):
        rng = np.random.default_rng(411 + case)
        v = _heavy(rng, M).astype(TF)
        groups, m = idx.shape
        g = R.norms(v, idx, TF, jn).astype(np.float64)
        if form == "scalar":
            c = TF(0.5 * g.max())
        else:
            c = (rng.choice([0.0, 0.5, 1.0, 2.0, np.inf], groups) * g).astype(TF)
            c[np.isnan(c)] = TF(0)      # (0 * inf where g = 0 meets inf)
        cv = R.bounds(c, groups, TF).astype(np.float64)
        y = R.project(v, idx, c, jn)
        assert y is not v, name
        # feasible: the exact norms of the float64 output, up to the rounding kg u of the TF norm the decision is taken on (csrc/l2inf.h)
        gy = np.sqrt(R.sumsq(y, idx))
        kg = (R.excess_units(TF, m) - 2.01) / 2
        assert np.all(gy <= cv * (1 + kg * u + 8 * np.finfo(np.float64).eps * m)), name
        # unclipped groups keep their values
        keep = ~(g > cv)
        for q in range(m):
            has = (idx[:, q] >= 0) & keep
            assert np.array_equal(y[idx[has, q]], v[idx[has, q]].astype(np.float64)), name
        # idempotent to the header's bound: the output rounded to TF is, observed in TF, within excess_units u c of c
        yt = y.astype(TF)
        gt = R.norms(yt, idx, TF, jn).astype(np.float64)
        assert np.all(gt <= cv * (1 + (R.excess_units(TF, m) + 1) * u)), name      # (+ 1: the rounding of y to TF here)
        # the variational inequality against feasible points z: scaled copies of v and of random vectors
        for trial in range(4):
            z = _heavy(rng, M) if trial % 2 else v.astype(np.float64) * rng.random(M)
            gz = np.sqrt(R.sumsq(z, idx))
            with np.errstate(divide="ignore", invalid="ignore"):
                s = np.where(gz > cv, cv / gz, 1.0)
            s[~np.isfinite(s)] = 0.0
            for q in range(m):
                has = idx[:, q] >= 0
                z[idx[has, q]] = z[idx[has, q]] * s[has] * (1 - 1e-12)
            lhs = float(np.dot(v.astype(np.float64) - y, z - y))
            scale = float(np.linalg.norm(v.astype(np.float64) - y) * (np.linalg.norm(z) + np.linalg.norm(y)))
            assert lhs <= 1e-12 * scale, (name, trial, lhs, scale)


def test_reference_returns_a_feasible_input_itself():
    for name, idx, M, jn in _layouts():
        v = _heavy(np.random.default_rng(5), M).astype(np.float32)
        c = R.max_norm(v, idx, np.float32, jn)
        assert R.project(v, idx, c, jn) is v, name
        assert R.project(v, idx, R.norms(v, idx, np.float32, jn), jn) is v, name


# ---- csrc/l2inf.h on the CPU -----------------------------------------------------------------------------------------------------------------
def _compile(tmp_path_factory, name):
    hipcc = shutil.which("hipcc") or shutil.which("hipcc", path=os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin"))
    assert hipcc, "hipcc not found"
    exe = str(tmp_path_factory.mktemp("l2inf") / name)
    r = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                        "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "l2inf", name + ".cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _compile(tmp_path_factory, "rule_driver")


def emulate(v, member, c):
    """The contract of csrc/l2inf.h for one group in numpy, in v's precision: (g, clipped, y)."""
    TF = v.dtype.type
    ss = 0.0
    for x, m in zip(v, member):
        if m:
            ss = ss + float(x) * float(x)
    g = TF(np.sqrt(np.float64(ss)))
    c = TF(c)
    if not g > c:
        return g, False, v.copy()
    with np.errstate(divide="ignore", invalid="ignore"):
        f = TF(c / g)
        y = np.array([TF(x * f) if m else x for x, m in zip(v, member)], TF)
    return g, True, y


def _hex(x):
    x = float(x)
    return "nan" if np.isnan(x) else ("inf" if x == np.inf else ("-inf" if x == -np.inf else x.hex()))


def _rule_cases(n, nmem, TF, rng):
    """(member, v, c) for a group of n entries of which the first nmem positions chosen are members: heavy-tailed with c below, on, one
    ulp above and one ulp below g, c = 0, c = +inf; an all-zero group; a group of -0.0."""
    member = np.zeros(n, bool)
    member[rng.permutation(n)[:nmem]] = True
    v = _heavy(rng, n).astype(TF)
    g, _, _ = emulate(v, member, np.inf)
    cases = [(member, v, TF(0.37) * g), (member, v, g), (member, v, np.nextafter(g, TF(np.inf))), (member, v, np.nextafter(g, TF(0))),
             (member, v, TF(0)), (member, v, TF(np.inf)), (member, v, TF(3) * g)]
    z = np.zeros(n, TF)
    cases += [(member, z, TF(0)), (member, z, TF(1)), (member, -z, TF(0)), (member, -z, TF(1))]
    w = v.copy()
    w[::2] = -0.0
    cases += [(member, w, TF(0.5) * emulate(w, member, np.inf)[0]), (member, w, TF(np.inf))]
    return cases


@pytest.mark.parametrize("TF", [np.float32, np.float64])
def test_header_rule_equals_the_emulation_bit_for_bit(driver, TF):
    tag = "f" if TF == np.float32 else "d"
    rng = np.random.default_rng(29)
    cases = []
    for n in (1, 2, 3, 6, 8):              # the entries of a group: the blocks of TV (2, 3) and of stacked operators (B)
        for nmem in sorted({0, 1, 2, 3, n} & set(range(n + 1))):
            cases += _rule_cases(n, nmem, TF, rng)
    lines = [f"{tag} {len(v)} {_hex(c)} " + " ".join(str(int(m)) for m in mem) + " " + " ".join(_hex(x) for x in v) for mem, v, c in cases]
    r = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True)
    out = r.stdout.splitlines()
    assert r.returncode == 0 and out and out[-1] == "ok" and len(out) == len(cases) + 1, r.stdout[-2000:] + r.stderr
    seen = {"on": 0, "above": 0, "below": 0, "zero_c": 0, "inf_c": 0, "neg_zero_kept": 0}
    for (mem, v, c), ln in zip(cases, out):
        w = ln.split()
        g_d, clipped_d = TF(float.fromhex(w[1])), int(w[3])
        y_d = np.array([float.fromhex(t) for t in w[5:]]).astype(TF)
        g, clipped, y = emulate(v, mem, c)
        assert l1_exact.same_bits(np.array([g_d]), np.array([g])) and clipped_d == int(clipped) and l1_exact.same_bits(y_d, y), (mem, v, c, ln)
        assert l1_exact.same_bits(y_d[~mem], v[~mem]), "a row the block does not have was written"
        if not clipped:
            assert l1_exact.same_bits(y_d, v), "an unclipped group keeps its bits"
        if g > 0 and c == g:
            seen["on"] += 1
            assert not clipped
        if g > 0 and c == np.nextafter(g, TF(0)):
            seen["above"] += 1
            assert clipped
        if g > 0 and c == np.nextafter(g, TF(np.inf)):
            seen["below"] += 1
            assert not clipped
        if c == 0 and g > 0:
            seen["zero_c"] += 1
            assert clipped and np.all(y_d[mem] == 0)
        if c == np.inf:
            seen["inf_c"] += 1
            assert not clipped
        if np.any(np.signbit(v) & (v == 0)) and not clipped:
            seen["neg_zero_kept"] += 1
            assert np.array_equal(np.signbit(y_d), np.signbit(v))
    assert all(k > 0 for k in seen.values()), seen


def test_header_bound_and_checks(driver):
    lines = ["units f 2", "units d 2", "units d 8", "shape 324 3", "shape 325 3", "shape 324 9", "vector f 4 0 1 0 inf -1 2 0 1 nan",
             "vector f 4 0 1 -1 2 3", "vector d 4 1 1 2 3 nan", "vector d 3 0 0 0 -0.0"]
    out = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True).stdout.splitlines()
    assert float.fromhex(out[0].split()[1]) == R.excess_units(np.float32, 2) and abs(R.excess_units(np.float32, 2) - 4.01) < 1e-6
    assert float.fromhex(out[1].split()[1]) == R.excess_units(np.float64, 2) == 6.01
    assert float.fromhex(out[2].split()[1]) == R.excess_units(np.float64, 8) == 12.01
    assert out[3] == "shape 108"
    assert "M = 325 rows, not a multiple of blocks = 3" in out[4] and "blocks = 9" in out[5]
    assert out[6] == "vector ok", "the entries of the groups without a member (3, 7) are not looked at"
    assert "bound 1 is negative or NaN" in out[7]
    assert "bound 3 is negative or NaN" in out[8], "a stacked operator has no group without a member"
    assert out[9] == "vector ok"


# ---- csrc/set_config.h: the descriptor rules, without a GPU ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = _compile(tmp_path_factory, "config_driver")

    def run(lines):
        lines = list(lines)
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines), out[-3:]
        return [k[len("error "):] if k.startswith("error ") else dict(t.split("=", 1) for t in k.split()[1:]) for k in out]
    return run


G2, G3 = "ndim=2 n=12,9,1", "ndim=3 n=8,6,5"


def test_engine_takes_the_sets(ask):
    for tf in "fd":
        rows = ask([f"set tf={tf} {G2} op=4 proj=24 pmax=2.5",
                    f"set tf={tf} {G3} op=4 proj=24 pmax=2.5",
                    f"set tf={tf} {G3} op=6 proj=24 pmax=2.5",
                    f"set tf={tf} {G3} op=6 proj=25 pmax=2.5",
                    f"set tf={tf} {G2} op=5 proj=26 pmax=2.5 rows=324 blocks=3",
                    f"set tf={tf} {G2} op=5 proj=26 pmax=2.5 rows=324 blocks=3 ata=5",
                    f"set tf={tf} {G2} op=4 proj=24 ub=108 reserved=108 ubat=107:-1",
                    f"set tf={tf} {G3} op=6 proj=24 ub=240 reserved=240 ubat=47:nan",
                    f"set tf={tf} {G3} op=6 proj=25 ub=48 reserved=48 ubat=3:inf",
                    f"set tf={tf} {G3} op=5 proj=26 ub=240 reserved=240 rows=1440 blocks=6 ubat=0:0"])
        for r in rows:
            assert isinstance(r, dict), r
            assert (r["prox"], r["needs_ext"], r["ncvx"], r["two_pass"], r["spec.mode"]) == ("8", "1", "0", "0", "0")
        want = [("26", "108", "2", "108"), ("26", "240", "3", "240"), ("26", "240", "2", "240"), ("27", "48", "2", "240"),
                ("28", "108", "3", "108"), ("28", "108", "3", "108"), ("26", "108", "2", "108"), ("26", "240", "2", "240"),
                ("27", "48", "2", "240"), ("28", "240", "6", "240")]
        for r, (kind, dl, nblk, bstride) in zip(rows, want):
            assert (r["ext_kind"], r["data_len"], r["spec.nblk"], r["spec.bstride"]) == (kind, dl, nblk, bstride), r
        assert rows[4]["mfree"] == "1" and rows[5]["mfree"] == "0" and rows[4]["custom"] == "1" and rows[4]["Mtrue"] == "324"


def test_engine_refusals(sipx, ask):
    H = sipx.host
    tv, jt, st = f"set {G2} op=4 proj=24", f"set {G3} op=6 proj=25", f"set {G2} op=5 proj=26 rows=324 blocks=3"
    cases = [
        (H.L2INF_MIN, tv + " pmax=1 pmin=0.5"), (H.L2INF_MIN, jt + " pmax=1 pmin=-1"), (H.L2INF_MIN, st + " pmax=1 pmin=1"),
        (H.L2INF_BAD_C, tv + " pmax=0"), (H.L2INF_BAD_C, tv + " pmax=-2"), (H.L2INF_BAD_C, jt + " pmax=nan"), (H.L2INF_BAD_C, st + " pmax=0"),
        (H.l2inf_bad_entry(5), tv + " ub=108 reserved=108 ubat=5:-1"), (H.l2inf_bad_entry(7), jt + " ub=48 reserved=48 ubat=7:nan"),
        (H.l2inf_bad_entry(107), st + " ub=108 reserved=108 ubat=107:-0.5"),
        (H.l2inf_bad_length(107, 108), tv + " ub=107 reserved=107"), (H.l2inf_bad_length(240, 48), jt + " ub=240 reserved=240"),
        (H.l2inf_bad_length(324, 108), st + " ub=324 reserved=324"), (H.l2inf_bad_length(0, 108), tv + " ub=108"),
        (H.L2INF_MODES, tv + " pmax=1 mode=1 dir=0"), (H.L2INF_MODES, f"set {G3} op=6 proj=24 pmax=1 mode=2 dir=2"),
        (H.L2INF_MODES, jt + " pmax=1 mode=2 dir=2"), (H.L2INF_MODES, st + " pmax=1 mode=1 dir=0"),
        (H.L2INF_NO_TRANSFORM, tv + " pmax=1 tr=1"), (H.L2INF_NO_TRANSFORM, jt + " pmax=1 tr=2"), (H.L2INF_NO_TRANSFORM, st + " pmax=1 tr=1"),
        (H.L2INF_NO_WEIGHTS, tv + " pmax=1 lb=108 reserved=108"), (H.L2INF_NO_WEIGHTS, jt + " pmax=1 lb=48"),
        (H.L2INF_NO_WEIGHTS, st + " pmax=1 lb=108"),
        (H.L2INF_NO_MINKOWSKI, tv + " pmax=1 comp=1"), (H.L2INF_NO_MINKOWSKI, tv + " pmax=1 comp=3"),
        (H.L2INF_NEEDS_TV, f"set {G2} op=0 proj=24 pmax=1"), (H.L2INF_NEEDS_TV, f"set {G2} op=1 proj=24 pmax=1"),
        (H.L2INF_NEEDS_TV, f"set {G2} op=3 proj=24 pmax=1"), (H.L2INF_NEEDS_TV, f"set {G2} op=5 proj=24 pmax=1 rows=324 blocks=3"),
        (H.L2INF_JOINT_ROUTE, f"set {G3} op=4 proj=25 pmax=1"), (H.L2INF_JOINT_ROUTE, f"set {G3} op=0 proj=25 pmax=1"),
        (H.L2INF_STACKED_NEEDS_CSC, f"set {G2} op=4 proj=26 pmax=1 blocks=2"), (H.L2INF_STACKED_NEEDS_CSC, f"set {G3} op=6 proj=26 pmax=1 blocks=2"),
        (H.L2INF_SHARDED, tv + " pmax=1 single=0"), (H.L2INF_SHARDED, st + " pmax=1 single=0"),
        (H.l2inf_bad_rows(325, 3), f"set {G2} op=5 proj=26 pmax=1 rows=325 blocks=3"),
        (H.l2inf_bad_blocks(0), f"set {G2} op=5 proj=26 pmax=1 rows=324 blocks=0"),
        (H.l2inf_bad_blocks(9), f"set {G2} op=5 proj=26 pmax=1 rows=324 blocks=9"),
    ]
    got = ask(line for _, line in cases)
    for (want, line), g in zip(cases, got):
        assert g == want, (line, g)
    # TV_xy in a sharded context is refused by the operator's own rule before the set's
    r = ask([jt + " pmax=1 single=0"])[0]
    assert isinstance(r, str) and "single-process contexts only" in r
    # every refusal names a way out
    for text in (H.L2INF_MIN, H.L2INF_BAD_C, H.L2INF_MODES, H.L2INF_NO_WEIGHTS, H.L2INF_NEEDS_TV, H.L2INF_JOINT_ROUTE, H.L2INF_STACKED_NEEDS_CSC,
                 H.L2INF_SHARDED, H.L2INF_NO_COARSE, H.L2INF_NO_SET_DATA, H.L2INF_NO_MINKOWSKI, H.L2INF_NO_TRANSFORM):
        assert "l2,inf" in text and len(text) > 60
    assert "np.repeat" in H.L2INF_MODES and "constant within every frame" in H.L2INF_MODES


BS, QT = chr(92), chr(34)
LITERAL = re.compile(QT + "((?:[^" + QT + BS + BS + "]|" + BS + BS + ".)*)" + QT)      # one C string literal, escapes kept


def test_header_and_front_end_word_the_refusals_alike(sipx):
    src = open(os.path.join(CSRC, "l2inf.h")).read()
    H = sipx.host
    for name in ("L2INF_NEEDS_TV", "L2INF_JOINT_ROUTE", "L2INF_STACKED_NEEDS_CSC", "L2INF_MIN", "L2INF_BAD_C", "L2INF_MODES", "L2INF_NO_TRANSFORM",
                 "L2INF_NO_WEIGHTS", "L2INF_NO_MINKOWSKI", "L2INF_SHARDED", "L2INF_NO_COARSE", "L2INF_NO_SET_DATA"):
        start = src.index("constexpr const char* " + name + " =")
        body = src[start:src.index(";", start)]
        text = "".join(t.replace(BS + QT, QT) for t in LITERAL.findall(body))
        assert text == getattr(H, name), name


# ---- the front end ------------------------------------------------------------------------------------------------------------------------------
def test_setup_constraints_takes_the_sets(sipx):
    TF = np.float32
    g2, g3 = sipx.compgrid((1.0, 1.0), (12, 9)), sipx.compgrid((1.0, 1.0, 1.0), (8, 6, 5))
    S = sp.vstack([sp.identity(108, format="csc")] * 2, format="csc")
    c = [sipx.set_definitions("l2inf", "TV", 0, 2.0, ("matrix", "")),
         sipx.set_definitions("l2inf", "TV", 0, np.full(108, 2.0), ("matrix", "")),
         sipx.set_definitions("l2inf", "Hessian", 0, 2.0, ("matrix", "")),
         sipx.set_definitions("l2inf_stacked", "mine", 0, np.full(108, 2.0), ("matrix", ""), custom_TD_OP=(S, False), blocks=2)]
    P, A, prop = sipx.setup_constraints(c, g2, TF)
    assert [p.kind for p in P] == ["l2inf", "l2inf", "l2inf_stacked", "l2inf_stacked"] and prop.ncvx == [False] * 4
    assert [p.seg_radii for p in P] == [False, True, False, True] and [p.blocks for p in P] == [0, 0, 3, 2]
    assert [p.data_len(a) for p, a in zip(P, A)] == [None, 108, None, 108] and A[2].kind == "custom" and A[3].kind == "custom"
    d = P[1].desc("TV", False)
    assert (d.proj, d.reserved, d.pmin) == (24, 108, 0.0) and P[3].desc("custom", False).reserved == 108 and P[3].desc("custom", False).blocks == 2
    c = [sipx.set_definitions("l2inf", "TV_xy", 0, np.full(240, 1.0), ("tensor", "")),
         sipx.set_definitions("l2inf_joint", "TV_xy", 0, 1.0, ("tensor", "")),
         sipx.set_definitions("l2inf_joint", "TV_xy", 0, np.full(48, 1.0), ("tensor", "")),
         sipx.set_definitions("l2inf", "D3D", 0, 1.0, ("tensor", "")),
         sipx.set_definitions("l2inf", "Hessian", 0, np.full(240, 1.0), ("tensor", ""))]
    P, A, prop = sipx.setup_constraints(c, g3, np.float64)
    assert [p.kind for p in P] == ["l2inf", "l2inf_joint", "l2inf_joint", "l2inf", "l2inf_stacked"]
    assert [p.data_len(a) for p, a in zip(P, A)] == [240, None, 48, None, 240] and P[4].blocks == 6 and P[4].rows == 1440
    assert P[0].ub.dtype == np.float64 and [a.kind for a in A[:4]] == ["TV_xy", "TV_xy", "TV_xy", "D3D"]


def test_host_refusals(sipx):
    TF = np.float32
    g = sipx.compgrid((1.0, 1.0), (12, 9))
    g3 = sipx.compgrid((1.0, 1.0, 1.0), (8, 6, 5))
    H = sipx.host
    S = sp.identity(108, format="csc")

    def refused(c, text, grid=g):
        with pytest.raises(sipx.SipxError) as e:
            sipx.setup_constraints([c], grid, TF)
        assert text in str(e.value), str(e.value)

    def sd(st="l2inf", op="TV", mn=0, mx=1.0, mode=("matrix", ""), **kw):
        return sipx.set_definitions(st, op, mn, mx, mode, **kw)
    for st, op, grid in (("l2inf", "TV", g), ("l2inf_joint", "TV_xy", g3), ("l2inf", "Hessian", g)):
        refused(sd(st, op, mn=0.5), H.L2INF_MIN, grid)
        for mx in (0.0, -1.0, float("nan")):
            refused(sd(st, op, mx=mx), H.L2INF_BAD_C, grid)
        refused(sd(st, op, weights=np.ones(108, TF)), H.L2INF_NO_WEIGHTS, grid)
        refused(sd(st, op, mn=np.zeros(108, TF)), H.L2INF_NO_WEIGHTS, grid)
        for mode in (("fiber", "x"), ("slice", "z"), ("fiber", "z")):
            refused(sd(st, op, mode=mode), H.L2INF_MODES, grid)
    refused(sd(mx=np.r_[np.ones(5), -1.0, np.ones(102)]), H.l2inf_bad_entry(5))
    refused(sd(mx=np.r_[np.ones(5), np.nan, np.ones(102)]), H.l2inf_bad_entry(5))
    sipx.setup_constraints([sd(mx=np.r_[np.ones(107), -1.0])], g, TF)      # the last corner has no member: its entry is not looked at
    sipx.setup_constraints([sd(mx=np.r_[np.zeros(50), np.full(58, np.inf)])], g, TF)
    refused(sd(mx=np.ones(107)), H.l2inf_bad_length(107, 108))
    refused(sd(mx=np.ones((12, 9))), H.l2inf_bad_length(108, 108))
    refused(sd("l2inf_joint", "TV_xy", mx=np.ones(240)), H.l2inf_bad_length(240, 48), g3)
    refused(sd("l2inf", "Hessian", mx=np.ones(324)), H.l2inf_bad_length(324, 108))
    refused(sd("l2inf", "Hessian", mx=np.r_[np.ones(107), -1.0]), H.l2inf_bad_entry(107))
    for op in ("DFT", "DCT", "wavelet"):
        refused(sd(op=op), H.L2INF_NO_TRANSFORM)
    for op in ("identity", "D_x", "D_z"):
        refused(sd(op=op), H.L2INF_NEEDS_TV)
    refused(sd(custom_TD_OP=(S, False)), H.L2INF_NEEDS_TV)
    refused(sd("l2inf_joint", "TV"), H.L2INF_JOINT_ROUTE, g3)
    refused(sd("l2inf_joint", "TV_xy"), H.TV_XY_NEEDS_3D)
    refused(sd("l2inf", "TV_xy"), H.TV_XY_NEEDS_3D)
    refused(sd("l2inf", "TV_xy"), H.TV_XY_NEEDS_3D, sipx.compgrid((1.0, 1.0, 1.0), (8, 6, 1)))      # one frame is a 2-D grid: ("l2inf", "TV")
    refused(sd("l2inf_stacked", "TV"), H.L2INF_STACKED_NEEDS_CSC)
    refused(sd("l2inf_stacked", "mine", custom_TD_OP=(S, False)), "needs blocks")
    refused(sd("l2inf_stacked", "mine", custom_TD_OP=(S, False), blocks=5), H.l2inf_bad_rows(108, 5))
    refused(sd("l2inf_stacked", "mine", custom_TD_OP=(S, False), blocks=9), H.l2inf_bad_blocks(9))
    refused(sd("l2inf", "Hessian", blocks=2), "has 3 blocks, blocks = 2 was given")
    refused(sd("l2inf", "Hessian"), "at least 3 grid points", sipx.compgrid((1.0, 1.0), (12, 2)))
    # a descriptor never reaches an operator it was not made for
    P = sipx.Projector(sd(), g, TF)
    with pytest.raises(sipx.SipxError, match="TD_OP must be TV"):
        P.check_rows(sipx.TDOperator("identity", g, TF))
    with pytest.raises(sipx.SipxError, match="the TV range: 195 entries on this grid, 108 given"):
        P(np.zeros(108, TF))

    with pytest.raises(sipx.SipxError, match="takes no Minkowski component"):
        P.check_rows(sipx.TDOperator("TV", g, TF, component=1))
    PH = sipx.Projector(sd("l2inf", "Hessian"), g, TF)
    with pytest.raises(sipx.SipxError, match="the operator must be SIPX_OP_CSC"):
        PH.check_rows(sipx.TDOperator("TV", g, TF))
    with pytest.raises(sipx.SipxError, match="the operator's range: 324 entries, 108 given"):
        PH(np.zeros(108, TF))
    with pytest.raises(sipx.SipxError, match="TD_OP must be TV"):
        sipx.l2inf_norm(np.zeros(108, TF), g, "D_z")
    with pytest.raises(sipx.SipxError, match="TD_OP must be TV_xy"):
        sipx.l2inf_norm(np.zeros(108, TF), g, "TV", joint=True)


def test_multilevel_refuses_the_sets(sipx):
    TF = np.float32
    g = sipx.compgrid((1.0, 1.0), (32, 24))
    m = np.ones(32 * 24, TF)
    opt = sipx.PARSDMM_options(FL=TF)
    S = sp.vstack([sp.identity(768, format="csc")] * 2, format="csc")
    for c in (sipx.set_definitions("l2inf", "TV", 0, 1.0, ("matrix", "")),
              sipx.set_definitions("l2inf", "Hessian", 0, 1.0, ("matrix", "")),
              sipx.set_definitions("l2inf_stacked", "custom", 0, 1.0, ("matrix", ""), custom_TD_OP=(S, False), blocks=2)):
        with pytest.raises(sipx.SipxError) as e:
            sipx.setup_multi_level_PARSDMM(m, 2, 2, g, [c], opt)
        assert str(e.value) == sipx.host.L2INF_NO_COARSE
        with pytest.raises(sipx.SipxError) as e:
            sipx.constraint2coarse([c], g, 2)
        assert str(e.value) == sipx.host.L2INF_NO_COARSE
    P, A, prop = sipx.setup_constraints([sipx.set_definitions("l2inf", "TV", 0, 1.0, ("matrix", ""))], g, TF)
    A, AtA, l, y = sipx.PARSDMM_precompute_distribute(A, prop, g, opt)
    with pytest.raises(sipx.SipxError) as e:
        sipx.PARSDMM_multi_level(m, [A], [AtA], [P], [prop], [g], opt)
    assert str(e.value) == sipx.host.L2INF_NO_COARSE
    g3 = sipx.compgrid((1.0, 1.0, 1.0), (16, 16, 8))
    with pytest.raises(sipx.SipxError):
        sipx.setup_multi_level_PARSDMM(np.ones(2048, TF), 2, 2, g3, [sipx.set_definitions("l2inf_joint", "TV_xy", 0, 1.0, ("tensor", ""))], opt)
