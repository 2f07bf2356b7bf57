"""l1 / l2 / annulus per fiber and per slice without a GPU: the host-side keyword and refusals, and csrc/seg_norm.h on the CPU.

tests/seg_norms/plan_driver.cpp includes seg_norm.h and calls its __host__ __device__ functions: the plan of a launch (mapping, F,
LDS or streaming, grid) for the shapes of tests/test_gpu_seg_norms.py, walking every address the kernel would touch, and the
per-segment threshold update, iterated serially, against tests/l1_exact.py.  hipcc compiles it (the header needs the HIP headers);
the program makes no HIP call."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import l1_exact, seg_norms_ref
from tests.test_gpu_seg_norms import CASES, CLASSES, RADIUS, class_counts, make_input

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "setintersectionprojection.jl_amd", "csrc")


# ---- host side ---------------------------------------------------------------------------------------------------------------------
def test_segment_norms_keyword_accepts_the_sets(sipx):
    TF = np.float32
    g = sipx.compgrid((25.0, 25.0, 25.0), (16, 12, 8))
    c = [sipx.set_definitions("bounds", "identity", 1.0, 2.0, ("tensor", "")),
         sipx.set_definitions("l1", "D_z", 0.0, 3.0, ("fiber", "z")),
         sipx.set_definitions("l1", "D_x", 0.0, 3.0, ("slice", "z")),
         sipx.set_definitions("l2", "identity", 0.0, 3.0, ("fiber", "x")),
         sipx.set_definitions("annulus", "identity", 1.0, 3.0, ("slice", "y"))]
    P, A, prop = sipx.setup_constraints(c, g, TF, segment_norms=True)
    assert prop.tag == [("bounds", "identity", "tensor", ""), ("l1", "D_z", "fiber", "z"), ("l1", "D_x", "slice", "z"),
                        ("l2", "identity", "fiber", "x"), ("annulus", "identity", "slice", "y")]
    assert prop.ncvx == [False] * 5
    assert prop.TD_n == [(16, 12, 8), (16, 12, 7), (15, 12, 8), (16, 12, 8), (16, 12, 8)]
    assert [(p.kind, p.mode, p.dir) for p in P] == [("bounds", 0, 0), ("l1", 1, 2), ("l1", 2, 2), ("l2", 1, 0), ("annulus", 2, 1)]
    d = P[1].desc("D_z", False)
    assert (d.mode, d.dir, d.pmax) == (1, 2, 3.0)
    # a 2-D grid: fiber x and fiber z (its second axis)
    g2 = sipx.compgrid((1.0, 1.0), (40, 28))
    P2, _, prop2 = sipx.setup_constraints([sipx.set_definitions("l1", "identity", 0.0, 3.0, ("fiber", "z")),
                                           sipx.set_definitions("annulus", "D_x", 1.0, 3.0, ("fiber", "x"))], g2, TF, segment_norms=True)
    assert [(p.mode, p.dir) for p in P2] == [(1, 1), (1, 0)] and prop2.ncvx == [False, False]


def test_without_the_keyword_the_reference_error_stays(sipx):
    TF = np.float32
    g = sipx.compgrid((25.0, 25.0, 25.0), (16, 12, 8))
    for st in ("l1", "l2"):
        for mode in (("fiber", "x"), ("slice", "z")):
            with pytest.raises(sipx.SipxError, match="l1 and l2 constraints only available for matrix or tensor mode, currently"):
                sipx.setup_constraints([sipx.set_definitions(st, "identity", 0.0, 1.0, mode)], g, TF)
            with pytest.raises(sipx.SipxError, match="only available for matrix or tensor mode, currently"):
                sipx.setup_constraints([sipx.set_definitions(st, "identity", 0.0, 1.0, mode)], g, TF, segment_norms=False)
    with pytest.raises(sipx.SipxError, match="segment_norms=True"):
        sipx.setup_constraints([sipx.set_definitions("annulus", "identity", 0.5, 1.0, ("fiber", "x"))], g, TF)
    sipx.setup_constraints([sipx.set_definitions("l1", "identity", 0.0, 1.0, ("fiber", "x"))], g, TF, segment_norms=True)


def test_refusals_with_the_keyword(sipx):
    TF = np.float32
    g3 = sipx.compgrid((25.0, 25.0, 25.0), (16, 12, 8))
    g2 = sipx.compgrid((25.0, 6.0), (16, 12))

    def setup(st, op, mode, g):
        return sipx.setup_constraints([sipx.set_definitions(st, op, 0.5, 1.0, mode)], g, TF, segment_norms=True)
    for st in ("l1", "l2", "annulus"):
        with pytest.raises(sipx.SipxError, match="one block"):                 # TV has one block per direction
            setup(st, "TV", ("fiber", "x"), g3)
        with pytest.raises(sipx.SipxError, match="for 2D models"):             # no slices of a 2-D grid
            setup(st, "identity", ("slice", "z"), g2)
        for op in ("DFT", "DCT", "wavelet"):                                   # a mode behind a transform
            with pytest.raises(sipx.SipxError, match="whole array"):
                setup(st, op, ("fiber", "x"), g3)
        with pytest.raises(sipx.SipxError, match="direction"):
            setup(st, "identity", ("fiber", "y"), g2)


# ---- the plan and the threshold update on the CPU --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    hipcc = shutil.which("hipcc") or shutil.which("hipcc", path=os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin"))
    assert hipcc, "hipcc not found"
    exe = str(tmp_path_factory.mktemp("seg_norms") / "plan_driver")
    r = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                        "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "seg_norms", "plan_driver.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _run(driver, lines):
    r = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True)
    out = r.stdout.splitlines()
    assert r.returncode == 0 and out and out[-1] == "ok", "\n".join(k for k in out if k.startswith("FAIL"))[:4000] + r.stderr
    return out


def _plans(driver):
    lines = []
    for n, mode in CASES:
        n3 = tuple(n) + (1,) * (3 - len(n))
        lines.append(f"shape {len(n)} {n3[0]} {n3[1]} {n3[2]} {1 if mode[0] == 'fiber' else 2} {seg_norms_ref.axis_of(n, mode)}")
    rows = [k.split() for k in _run(driver, lines) if k.startswith("plan ")]
    assert len(rows) == 2 * len(CASES)
    plans = {}
    for i, (n, mode) in enumerate(CASES):
        for j, eb in enumerate((4, 8)):
            row = rows[2 * i + j]
            p = {row[q]: int(row[q + 1]) for q in range(1, len(row), 2)}
            assert p["bytes"] == eb
            plans[(n, mode, eb)] = p
    return plans


def test_gpu_shapes_reach_every_path(driver):
    """The driver has walked every address of every plan (identity and difference-operator extents) against seg_addr."""
    plans = _plans(driver)
    BLOCK = 256
    for eb in (4, 8):
        mine = [p for (n, mode, b), p in plans.items() if b == eb]
        assert {p["path"] for p in mine} == {0, 1, 2, 3}, eb            # {segment, tile} x {LDS, streaming}
        for path in (2, 3):                                             # a ragged last tile, resident and streaming
            assert any(p["path"] == path and p["ragged"] != 0 for p in mine), (eb, path)
        assert any(p["path"] == 2 and p["ragged"] == 0 for p in mine)
        assert any(p["F"] == 1 and p["L"] < 64 for p in mine)           # a segment shorter than a wave
        for path in (0, 1):                                             # a segment longer than the workgroup, resident and streaming
            assert any(p["path"] == path and p["L"] > BLOCK for p in mine), (eb, path)
        assert any(p["F"] > 1 and p["L"] < BLOCK // p["F"] for p in mine)   # fewer elements than lanes of a tile's sub-group
        assert any(p["ntiles"] > 1 for p in mine) and all(p["grid"] == p["ntiles"] for p in mine)
    for (n, mode, eb), p in plans.items():
        segs = seg_norms_ref.segment_indices(n, mode)
        assert p["nseg"] == len(segs) and p["L"] == len(segs[0]) and p["nseg"] >= 10, (n, mode)
        assert (p["F"] > 1) == (mode in (("fiber", "y"), ("fiber", "z"), ("slice", "x"))), (n, mode)
        assert p["lds"] == (p["F"] * p["L"] * eb <= 32 * 1024)
    # ... and every input of the GPU test mixes the segment classes, two of each at least
    for TF in (np.float32, np.float64):
        for n, mode in CASES:
            counts = class_counts(n, mode, TF)
            assert set(counts) == set(CLASSES) | {"negzero"} and all(c >= 2 for c in counts.values()), (n, mode, counts)


def _theta_lines(vectors):
    return [f"l1 {'f' if v.dtype == np.float32 else 'd'} {float(b).hex()} {len(v)} " + " ".join(float(x).hex() for x in v) for v, b in vectors]


def test_serial_threshold_update_gives_the_exact_theta(driver):
    vectors = []
    for TF in (np.float32, np.float64):
        rng = np.random.default_rng(7)
        b = TF(RADIUS)
        vectors += [(np.array([9.5], TF), b), (np.array([-0.5], TF), b), (np.array([0.0], TF), b),                # L = 1
                    (np.array([9.0, 1.0], TF), b), (np.array([6.0, -5.0], TF), b), (np.array([3.0, 2.0], TF), b),   # L = 2
                    (np.array([3, 3, 3, 3, -3, 1, 0, 0], TF), TF(5.0)),                                           # heavy ties
                    (np.array([3.0] * 4 + [1.0] * 9 + [0.25] * 7 + [-0.0] * 3, TF), b),                           # ties on the threshold
                    (np.full(37, 1.0, TF), b), (np.zeros(11, TF), b), (np.array([-0.0, 0.0, 20.0, -0.0], TF), b)]
        for L in (2, 3, 7, 33, 300, 2000):
            h = (rng.standard_normal(L) * np.exp(rng.standard_normal(L)))
            vectors.append(((h * 2.5 * RADIUS / np.abs(h).sum()).astype(TF), b))                                  # heavy-tailed
            vectors.append((((RADIUS / L) * (1.5 + 0.1 * rng.random(L))).astype(TF), b))                          # all active: the lv - 1 cap
            h[::3] = 0
            vectors.append(((h * 40 * RADIUS / np.abs(h).sum()).astype(TF), b))                                   # zeros, few survivors
        # segments of the GPU test's own inputs
        for n, mode in (((5, 7, 33), ("fiber", "y")), ((40, 28), ("fiber", "z")), ((4, 5, 2), ("fiber", "z"))):
            v, segs = make_input(n, mode, TF)
            vectors += [(v[ind], b) for ind in segs[:10]]
    rows = [k.split() for k in _run(driver, _theta_lines(vectors)) if k.startswith("theta ")]
    assert len(rows) == len(vectors)
    seen_cap = seen_tie = 0
    for (v, b), row in zip(vectors, rows):
        TF = v.dtype.type
        need, theta, steps = int(row[1]), float.fromhex(row[2]), int(row[3])
        fz = l1_exact.feasibility(v, b)
        assert fz != 0
        assert need == (1 if fz < 0 else 0), (v, b)
        if not need:
            continue
        a = np.abs(v.astype(np.float64))
        th, C, S = l1_exact.exact_theta(a, b)
        tol = l1_exact.theta_tol(C, S, b, th, TF) - 0.5 * l1_exact.ulp(th, TF)      # the float64 theta: before the one rounding to TF
        assert abs(theta - th) <= tol, (len(v), theta, th, tol)
        assert abs(float(TF(theta)) - th) <= l1_exact.theta_tol(C, S, b, th, TF)
        assert 1 <= steps <= len(v) + 2
        l1_exact.check_l1_output(v, l1_exact.soft(v, TF(theta)), b, theta_engine=TF(theta))
        seen_cap += len(v) > 1 and a.min() > (a.sum() - float(b)) / len(v)
        seen_tie += bool(np.any(a == th))
    assert seen_cap >= 8 and seen_tie >= 8
