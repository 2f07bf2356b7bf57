"""The db4 axis passes of csrc/kernels_dwt.hip without a GPU: which launches the edge grids of tests/test_gpu_wavelet.py reach
(plan(), from the constants of the kernel file), and the work items themselves on the CPU.

tests/dwt_passes/passes_driver.cpp includes kernels_dwt.hip and calls the __host__ __device__ item functions
pass_item<T, INV, R> for R = 1, RC and RS over every work item of every level's box of EDGE_SHAPES, against the direct formula
of dwt.h with the coefficients of tests/dwt_ref.py: double to 1e-13, float to 2e-6, inputs NaN and outputs fenced outside the
box.  hipcc compiles it (the file needs the HIP headers); the program makes no HIP call."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import dwt_ref
from tests.test_gpu_learn import WAVELET_GRID
from tests.test_gpu_wavelet import EDGE_SHAPES, KERNELS, kernel_constants, plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.dirname(KERNELS)


def _passes(shapes, ndim):
    """(level, axis, m, h % R) of every axis pass the ndim-dimensional grids of shapes take, and the grids' plans"""
    plans = {n: plan(n) for n in shapes if len(n) == ndim}
    return [(l + 1, a, m, r) for p in plans.values() for l, (kind, axes) in enumerate(p) if kind == "pass"
            for a, (m, r) in enumerate(axes)], plans


def test_kernel_constants_are_read():
    k = kernel_constants()
    assert k["RC"] >= 1 and k["RS"] >= 1 and k["SMALL"] >= 1, k
    # plan() restates first_small / level_box: the levels of the flagship's 256^3, passes down to the first box that fits
    p = plan((256, 256, 256))
    kinds = [kind for kind, _ in p]
    first = kinds.index("small")
    assert len(p) == 8 and kinds == ["pass"] * first + ["small"] * (8 - first)
    assert [m for m, _ in p[first][1]] == [256 >> first] * 3 and (256 >> first) ** 3 <= k["SMALL"] < (512 >> first) ** 3
    assert p[0][1] == ((256, 128 % k["RC"]), (256, 128 % k["RS"]), (256, 128 % k["RS"]))


def test_edge_shapes_are_legal_and_small_enough_for_the_restatement():
    for n in EDGE_SHAPES:
        L = dwt_ref.levels(n)
        assert L >= 1 and all(v % (1 << L) == 0 for v in n), n
        assert max(n) <= 2100, n                    # dwt_ref builds a dense m x m matrix per axis


def test_edge_shapes_reach_the_paths_of_the_pass_kernels():
    p2, plans2 = _passes(EDGE_SHAPES, 2)
    p3, plans3 = _passes(EDGE_SHAPES, 3)
    every = p2 + p3
    assert any(a == 0 and r != 0 for _, a, _, r in every)           # a partial last run along the contiguous axis (RC)
    assert any(a == 1 and r != 0 for _, a, _, r in every)           # ... along each strided axis (RS)
    assert any(a == 2 and r != 0 for _, a, _, r in every)
    for axis in range(3):                                           # an axis shorter than the 8 taps inside a pass
        assert any(a == axis and m < 8 for _, a, m, _ in every), axis
    assert {m for _, _, m, _ in every if m < 8} == {2, 4, 6}
    assert any(l >= 2 for l, _, _, _ in p2) and any(l >= 2 for l, _, _, _ in p3)       # compact boxes, 2-D and 3-D
    assert any(l >= 2 and r != 0 for l, _, _, r in p2) and any(l >= 2 and r != 0 for l, _, _, r in p3)     # ... with ragged runs
    for plans in (plans2, plans3):
        assert any(all(kind == "pass" for kind, _ in p) for p in plans.values())       # no one-workgroup launch at all
        # the one-workgroup kernel after passes, on a grid that is not a power of two
        assert any(p[0][0] == "pass" and p[-1][0] == "small" and any(v & (v - 1) for v in n) for n, p in plans.items())


def test_the_learner_grid_leaves_the_small_box_with_ragged_runs():
    p = plan(WAVELET_GRID)
    assert WAVELET_GRID[0] == WAVELET_GRID[1] and WAVELET_GRID[0] & (WAVELET_GRID[0] - 1)
    assert [kind for kind, _ in p] == ["pass", "pass", "small"]
    assert all(axes[1][1] != 0 for kind, axes in p if kind == "pass")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    hipcc = shutil.which("hipcc") or shutil.which("hipcc", path=os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin"))
    assert hipcc, "hipcc not found"
    exe = str(tmp_path_factory.mktemp("dwt_passes") / "passes_driver")
    r = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                        "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "dwt_passes", "passes_driver.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _boxes():
    out = []
    for n in EDGE_SHAPES:
        n3 = tuple(n) + (1,) * (3 - len(n))
        for l in range(dwt_ref.levels(n)):
            out.append((len(n),) + n3 + tuple(v >> l if a < len(n) else 1 for a, v in enumerate(n3)))
    return out


def test_pass_items_match_the_direct_formula(driver):
    boxes = _boxes()
    assert len(boxes) == sum(len(plan(n)) for n in EDGE_SHAPES)
    text = "\n".join([" ".join(float(v).hex() for v in dwt_ref.LO), " ".join(float(v).hex() for v in dwt_ref.HI)] +
                     [" ".join(str(v) for v in b) for b in boxes]) + "\n"
    r = subprocess.run([driver], input=text, capture_output=True, text=True)
    lines = r.stdout.splitlines()
    print(r.stdout)
    assert r.returncode == 0 and lines[-1] == "ok", "\n".join(k for k in lines if k.startswith("FAIL"))[:4000] + r.stderr
    rows = [k.split() for k in lines if k.startswith("box ")]
    assert len(rows) == len(boxes)
    for b, row in zip(boxes, rows):
        # float and double x two stride layouts x the box's axes x forward and inverse x R in {1, RC, RS}
        assert int(row[row.index("passes") + 1]) == 2 * 2 * b[0] * 2 * 3, row
        ef, ed = float(row[row.index("err_f") + 1]), float(row[row.index("err_d") + 1])
        assert 0 < ef <= 2e-6 and 0 < ed <= 1e-13, row
    assert np.isfinite([float(row[-1]) for row in rows]).all()
