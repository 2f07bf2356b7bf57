"""One radius per fiber / per slice without a GPU: the segment index of csrc/seg_norm.h walked on the CPU, the host-side handling of the
radius vectors (broadcast, lengths, the l1 radius rule, what set_data takes) and the arguments of sipx.segment_norms.

tests/seg_radii/index_driver.cpp includes seg_norm.h and walks (tile, f) of every plan of tests/test_gpu_seg_norms.CASES with
seg_tile_index, the function the kernel loads rmin[s] / rmax[s] and stores the observed norms with.  hipcc compiles it (the header needs
the HIP headers); the program makes no HIP call."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import seg_norms_ref
from tests.test_device_io_cpu import FakeCuda
from tests.test_gpu_seg_norms import CASES, CLASSES
from tests.test_gpu_seg_radii import l2_counts, l2_radii, make_radii_input, radii_class_counts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "setintersectionprojection.jl_amd", "csrc")
TF = np.float32


# ---- the segment index on the CPU ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    hipcc = shutil.which("hipcc") or shutil.which("hipcc", path=os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin"))
    assert hipcc, "hipcc not found"
    exe = str(tmp_path_factory.mktemp("seg_radii") / "index_driver")
    r = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                        "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "seg_radii", "index_driver.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_every_segment_index_is_hit_once_and_dead_lanes_yield_none(driver):
    lines = []
    for n, mode in CASES:
        n3 = tuple(n) + (1,) * (3 - len(n))
        lines.append(f"shape {len(n)} {n3[0]} {n3[1]} {n3[2]} {1 if mode[0] == 'fiber' else 2} {seg_norms_ref.axis_of(n, mode)}")
    r = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True)
    out = r.stdout.splitlines()
    assert r.returncode == 0 and out and out[-1] == "ok", "\n".join(k for k in out if k.startswith("FAIL"))[:4000] + r.stderr
    rows = [k.split() for k in out if k.startswith("index ")]
    assert len(rows) == 2 * len(CASES)
    ragged = 0
    for i, (n, mode) in enumerate(CASES):
        for j, eb in enumerate((4, 8)):
            p = {rows[2 * i + j][q]: int(rows[2 * i + j][q + 1]) for q in range(1, len(rows[2 * i + j]), 2)}
            assert p["bytes"] == eb and p["nseg"] == len(seg_norms_ref.segment_indices(n, mode))
            assert p["dead"] == p["tiles"] * p["F"] - p["nseg"]
            ragged += p["dead"] > 0
    assert ragged >= 4          # ragged tiles with dead lanes were walked, in both element sizes


# ---- the inputs of the GPU tests, from the references alone -------------------------------------------------------------------------
def test_l1_inputs_mix_the_classes_with_respect_to_their_own_radii():
    for tf in (np.float32, np.float64):
        for n, mode in CASES:
            _, segs, radii = make_radii_input(n, mode, tf)
            assert radii.dtype == tf and len(radii) == len(segs) and set(np.unique(radii)) <= {2.0, 4.0, 8.0, 16.0}
            counts = radii_class_counts(n, mode, tf)
            assert set(counts) == set(CLASSES) | {"negzero"} and all(c >= 2 for c in counts.values()), (n, mode, counts)


def test_l2_inputs_have_segments_on_every_side_of_their_own_radii():
    for tf in (np.float32, np.float64):
        for n, mode in CASES:
            v, segs, lo_s, hi_s = l2_radii(n, mode, tf)
            assert np.all(lo_s < hi_s) and len(np.unique(hi_s)) == len(segs)
            for st in ("l2", "annulus"):
                cnt = l2_counts(v, segs, lo_s, hi_s, st)
                assert cnt["above"] >= 2 and cnt["inside"] >= 2 and cnt["zero"] >= 2 and (st == "l2" or cnt["below"] >= 2), (n, mode, st, cnt)


# ---- host side -----------------------------------------------------------------------------------------------------------------
G3 = ((25.0, 25.0, 25.0), (16, 12, 8))


def _setup(sipx, st, op, mn, mx, mode, grid=G3, tf=TF):
    g = sipx.compgrid(*grid)
    P, A, prop = sipx.setup_constraints([sipx.set_definitions(st, op, mn, mx, mode)], g, tf, segment_norms=True)
    return P[0], A[0], prop


def test_vectors_and_scalars_are_broadcast(sipx):
    r = np.linspace(1.0, 2.0, 192)                                   # fibers along z of (16, 12, 7): 16 * 12
    P, A, prop = _setup(sipx, "l1", "D_z", 0.0, r, ("fiber", "z"))
    assert P.seg_radii and P.kind == "l1" and P.lb is None and P.ub.dtype == TF and np.array_equal(P.ub, r.astype(TF))
    assert prop.ncvx == [False] and prop.TD_n == [(16, 12, 7)] and P.nseg(A) == 192 and P.data_len(A) == 192
    d = P.desc("D_z", False)
    assert d.ub and not d.lb and (d.mode, d.dir) == (1, 2)
    # slices orthogonal to z of D_x: one radius per z
    P, A, _ = _setup(sipx, "l2", "D_x", 0.0, list(range(1, 9)), ("slice", "z"))
    assert P.nseg(A) == 8 and np.array_equal(P.ub, np.arange(1, 9, dtype=TF))
    # the annulus: either side a vector, a scalar beside it repeated
    lo, hi = np.linspace(0.5, 1.0, 12), np.linspace(2.0, 3.0, 12)
    for mn, mx in ((lo, hi), (0.25, hi), (lo, 4.0)):
        P, A, prop = _setup(sipx, "annulus", "identity", mn, mx, ("slice", "y"))
        want_lo = lo.astype(TF) if np.ndim(mn) else np.full(12, 0.25, TF)
        want_hi = hi.astype(TF) if np.ndim(mx) else np.full(12, 4.0, TF)
        assert P.seg_radii and np.array_equal(P.lb, want_lo) and np.array_equal(P.ub, want_hi) and prop.ncvx == [False]
        d = P.desc("identity", False)
        assert d.lb and d.ub
    # scalars: as before, nothing replaceable
    P, A, _ = _setup(sipx, "l1", "D_z", 0.0, 3.0, ("fiber", "z"))
    assert not P.seg_radii and P.ub is None and P.data_len(A) is None and P.pmax == 3.0
    d = P.desc("D_z", False)
    assert not d.lb and not d.ub
    # a 2-D grid: fibers along z are indexed by x
    P, A, _ = _setup(sipx, "l2", "identity", 0.0, np.ones(40), ("fiber", "z"), grid=((1.0, 1.0), (40, 28)), tf=np.float64)
    assert P.nseg(A) == 40 and P.ub.dtype == np.float64
    # vector radii are data of the descriptor: such a list is not cached by its scalars
    g = sipx.compgrid(*G3)
    opt = sipx.PARSDMM_options(FL=TF)
    P1, A1, prop1 = sipx.setup_constraints([sipx.set_definitions("l2", "identity", 0.0, np.ones(12), ("slice", "y"))], g, TF, segment_norms=True)
    assert sipx.host._context_key(np.zeros(1, TF), None, A1, prop1, P1, g, opt, 0) is None


def test_a_wrong_length_names_nseg_and_the_segment(sipx):
    with pytest.raises(sipx.SipxError, match=r"max has 191 entries, nseg = 192 are needed.*fiber along dimension 3.*\(16, 12, 7\)"):
        _setup(sipx, "l1", "D_z", 0.0, np.ones(191), ("fiber", "z"))
    with pytest.raises(sipx.SipxError, match=r"max has 12 entries, nseg = 8 are needed.*slice orthogonal to dimension 3"):
        _setup(sipx, "l2", "D_x", 0.0, np.ones(12), ("slice", "z"))
    with pytest.raises(sipx.SipxError, match=r"min has 7 entries, nseg = 8"):
        _setup(sipx, "annulus", "identity", np.ones(7), 3.0, ("slice", "z"))
    with pytest.raises(sipx.SipxError, match="1-D vector"):
        _setup(sipx, "l2", "identity", 0.0, np.ones((4, 2)), ("slice", "z"))


def test_a_non_positive_l1_radius_is_the_reference_error(sipx):
    for bad in (0.0, -1.0, float("nan")):
        r = np.ones(8)
        r[5] = bad
        with pytest.raises(sipx.SipxError, match=r"Radius of L1 ball is negative \(segment 5"):
            _setup(sipx, "l1", "identity", 0.0, r, ("slice", "z"))
    r = np.ones(8)
    r[5] = 0.0
    _setup(sipx, "l2", "identity", 0.0, r, ("slice", "z"))          # the l2 ball of radius 0 is a set


@pytest.fixture
def solver(sipx, monkeypatch):
    """{bounds, l1 on D_x per slice z (vector radii), annulus per fiber x (vectors), l2 per fiber z (scalar)} on 12 x 10 x 4, and a
    library that must not be touched."""
    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(sipx.host, "lib", no_library)
    n = (12, 10, 4)
    g = sipx.compgrid((1.0, 1.0, 1.0), n)
    opt = sipx.PARSDMM_options(FL=TF, maxit=5)
    c = [sipx.set_definitions("bounds", "identity", 0.0, 1.0, ("tensor", "")),
         sipx.set_definitions("l1", "D_x", 0.0, np.ones(4), ("slice", "z")),
         sipx.set_definitions("annulus", "identity", np.ones(40), 2.0, ("fiber", "x")),
         sipx.set_definitions("l2", "identity", 0.0, 2.0, ("fiber", "z"))]
    P, A, prop = sipx.setup_constraints(c, g, TF, segment_norms=True)
    A, AtA, l, y = sipx.PARSDMM_precompute_distribute(A, prop, g, opt)
    return sipx.Solver(AtA, A, prop, P, g, opt, TF)


def test_solver_set_data_takes_radii_of_vector_built_sets_only(sipx, solver):
    assert [p.data_len(a) for p, a in zip(solver.P_sub, solver.TD_OP)] == [None, 4, 40, None]
    with pytest.raises(sipx.SipxError, match=r"set 3 \(l2 on identity\) holds no replaceable vectors.*build a new Solver"):
        solver.set_data(3, ub=np.ones(120, TF))
    with pytest.raises(sipx.SipxError, match="ub has 5 entries, 4 are needed"):
        solver.set_data(1, ub=np.ones(5, TF))
    with pytest.raises(sipx.SipxError, match="lb has 4 entries, 40 are needed"):
        solver.set_data(2, lb=FakeCuda(4))
    with pytest.raises(sipx.SipxError, match="ub has dtype float64: not the working precision"):
        solver.set_data(1, ub=np.ones(4))
    with pytest.raises(sipx.SipxError, match="only the annulus has inner radii"):
        solver.set_data(1, lb=np.ones(4, TF))
    with pytest.raises(sipx.SipxError, match=r"Radius of L1 ball is negative \(segment 2"):
        solver.set_data(1, ub=np.array([1, 1, 0, 1], TF))
    with pytest.raises(sipx.SipxError, match="both be numpy arrays or both be tensors"):
        solver.set_data(2, np.ones(40, TF), FakeCuda(40))
    solver.set_data(1)                          # nothing given: nothing to do, nothing loaded
    # accepted: every check passes and the call goes on to the library
    for args in ((1, None, np.ones(4, TF)), (2, np.ones(40, TF), np.full(40, 3.0, TF)), (2, None, FakeCuda(40))):
        with pytest.raises(AssertionError, match="the library was loaded|a pointer was taken"):
            solver.set_data(*args)
        solver.closed = False


def test_segment_norms_refuses_wrong_arguments_before_the_library(sipx, monkeypatch):
    def no_library():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(sipx.host, "lib", no_library)
    assert {"sipx_segment_norms", "sipx_segment_norms_dev"} <= set(sipx.EXPORTED_SYMBOLS) and sipx.segment_norms is sipx.host.segment_norms
    g3, g2 = sipx.compgrid(*G3), sipx.compgrid((25.0, 6.0), (16, 12))
    x3, x2 = np.zeros(16 * 12 * 8, TF), np.zeros(16 * 12, TF)
    f = sipx.segment_norms
    with pytest.raises(sipx.SipxError, match="norm must be 'l1' or 'l2'"):
        f(x3, g3, "identity", ("fiber", "x"), "linf")
    for op in ("TV", "DFT", "wavelet"):
        with pytest.raises(sipx.SipxError, match="one block"):
            f(x3, g3, op, ("fiber", "x"), "l1")
    with pytest.raises(sipx.SipxError, match="app_mode must be"):
        f(x3, g3, "identity", ("tensor", ""), "l1")
    with pytest.raises(sipx.SipxError, match="for 2D models"):
        f(x2, g2, "identity", ("slice", "z"), "l1")
    with pytest.raises(sipx.SipxError, match="direction"):
        f(x2, g2, "identity", ("fiber", "y"), "l1")
    with pytest.raises(sipx.SipxError, match="unknown transform domain operator"):
        f(x2, g2, "D_y", ("fiber", "x"), "l1")
    with pytest.raises(sipx.SipxError, match="x has 192 entries, 1536 are needed"):
        f(x2, g3, "identity", ("fiber", "x"), "l2")
    with pytest.raises(sipx.SipxError, match="Float32 or Float64"):
        f(np.zeros(1536, np.int32), g3, "identity", ("fiber", "x"), "l2")
    with pytest.raises(sipx.SipxError, match="x has 7 entries, 1536 are needed"):
        f(FakeCuda(7), g3, "D_z", ("slice", "z"), "l2")
    with pytest.raises(sipx.SipxError, match="x must live on a GPU"):
        import torch
        f(torch.zeros(1536), g3, "D_z", ("slice", "z"), "l2")
