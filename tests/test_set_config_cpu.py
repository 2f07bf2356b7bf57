"""What a set descriptor means on a grid (csrc/set_config.h), without a GPU: routes, rows, vector lengths and every refusal.

tests/set_config/config_driver.cpp includes set_config.h and answers one request per line with the SetConfig the engine would keep
for that descriptor, or with the refusal's text.  hipcc compiles it (the header needs the HIP headers); the program makes no HIP
call.  Expected values come from the oracle's sparse operators, from host.Projector, from numpy, or are literals: the refusals'
texts below are those of the engine before the rules left it."""
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import parsdmm_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "setintersectionprojection.jl_amd", "csrc")
HEADER = os.path.join(CSRC, "set_config.h")
OPS = {"identity": 0, "D_x": 1, "D_y": 2, "D_z": 3, "TV": 4, "custom": 5, "TV_xy": 6}                     # include/sipx.h
PROJ = {"bounds": 0, "bounds_vec": 1, "l1": 2, "l2": 3, "annulus": 4, "cardinality": 5, "prox_l1": 6, "l1_dft": 7, "rank": 8,
        "nuclear": 9, "histogram": 10, "subspace": 11, "bounds_dft": 12, "card_dft": 13, "l21": 14}
EXT = {"l1_dft": 1, "rank": 2, "nuclear": 3, "card_seg": 4, "histogram": 5, "subspace": 6, "dft_mask": 7, "dct": 8, "dwt": 9,
       "card_dft": 10, "l1_seg": 11, "l2_seg": 12, "annulus_seg": 13, "l21": 14, "l21_seg": 15}           # csrc/ext_proj.h
PX_EXT = 8
GRIDS = [(3, 4), (3, 4, 5), (4, 4, 1), (1, 4)]
SPACING = (25.0, 6.0, 3.0)                      # 1/h is not a float32 for two of them
TYPES = [("f", np.float32), ("d", np.float64)]


def _read(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    """ask(lines) -> per line a dict of the printed fields, or the refusal's text"""
    hipcc = shutil.which("hipcc") or shutil.which("hipcc", path=os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin"))
    assert hipcc, "hipcc not found"
    exe = str(tmp_path_factory.mktemp("set_config") / "config_driver")
    r = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                        "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "set_config", "config_driver.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(lines):
        lines = list(lines)
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines), out[-3:]
        answers = []
        for k in out:
            if k.startswith("error "):
                answers.append(k[len("error "):])
            else:
                assert k == "ok" or k.startswith("ok "), k
                answers.append(dict(t.split("=", 1) for t in k.split()[1:]))
        return answers
    return run


def req(n, tf="f", **kw):
    """a `set` request on the grid n with the spacings SPACING; lists become comma-separated fields"""
    def tok(v):
        if isinstance(v, (list, tuple, np.ndarray)):
            return ",".join(tok(x) for x in v)
        return float(v).hex() if isinstance(v, (float, np.floating)) else str(v)
    n3 = tuple(n) + (1,) * (3 - len(n))
    fields = dict(tf=tf, ndim=len(n), n=n3, h=SPACING, **kw)
    return "set " + " ".join(f"{k}={tok(v)}" for k, v in fields.items())


def ints(field):
    return [int(v) for v in field.split(",")] if field else []


# ---- header hygiene -------------------------------------------------------------------------------------------------------------------
MOVED = ("configure_op", "configure_proj", "configure_custom", "expand_fiber_bounds", "check_l1_radii", "check_mf_index_range",
         "default_ata_offsets", "data_len", "refuse_sharded_radii", "refuse_sharded_l21", "refuse_sharded_tv_xy")


def test_header_is_host_only_and_listed():
    head = _read(HEADER)
    assert not re.search(r"hip[A-Z]\w*\(", head)
    assert "set_config.h" in re.search(r"^HDRS\s*=(.*)$", _read(os.path.join(CSRC, "Makefile")), re.M).group(1).split()


def test_engine_defines_none_of_the_rules():
    eng = _read(os.path.join(CSRC, "engine.cpp"))
    assert '#include "set_config.h"' in eng
    for name in MOVED:             # moved, not copied: no definition at class scope ("  <type> name(...) ... {")
        assert not re.search(r"^  \S.*\b%s\([^;]*\{\s*$" % name, eng, re.M), name
    for name in ("seg_count", "dwt_levels", "dwt_check_grid"):      # one inline copy each, beside make_segmap and in dwt.h
        for unit in ("ext_segments.hip", "kernels_dwt.hip"):
            assert not re.search(r"^\w.*\b%s\(.*\{" % name, _read(os.path.join(CSRC, unit)), re.M), (name, unit)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
L1_RADIUS = "Radius of L1 ball is negative"
ONE_BLOCK_MODE = "fiber / slice modes need an operator with one block (identity, D_x, D_y, D_z)"
ONE_BLOCK_EXT = "this projector needs an operator with one block (identity, D_x, D_y, D_z)"
L21_NEEDS_TV = "the l2,1 ball acts on the range of the TV operator: TD_OP must be TV (D2D, D3D)"
FRAMES_Z = "the l2,1 ball on TV_xy: frames run along z -- the mode must be (slice, z), or tensor for the whole array"
DCT_DOMAIN = "sets behind the DCT act in their own domain: TD_OP must be the identity, mode matrix/tensor"
DWT_DOMAIN = "sets behind the wavelet transform act in their own domain: TD_OP must be the identity, mode matrix/tensor"
NEED_LB_UB = "per-element bounds need lb and ub"
TV_XY_NO_COMPONENT = "the TV_xy operator takes no Minkowski component"
SHARDED = {
    "radii": "per-fiber / per-slice l1, l2 and annulus sets with one radius per segment take single-process contexts only, this "
             "one has a communicator, a slab decomposition or set ownership: use a scalar radius, or a single process",
    "l21": "the l2,1 ball on the TV operator (isotropic total variation) takes single-process contexts only, this one "
           "has a communicator, a slab decomposition or set ownership: use the l1 ball on TV, or a single process",
    "tv_xy": "the TV_xy operator takes single-process contexts only, this one has a communicator, a slab decomposition "
             "or set ownership: use D_x and D_y sets, or a single process"}
G2, G3 = (3, 4), (3, 4, 5)
CSC_OK = "csc=2/0,1,1,2,2,2,2,2,2,2,2,2,2/0,1"             # 2 x 12: a (0, 0) and a (1, 2) entry
ONES12 = "fill:12:1"

# every throw of configure_op / configure_custom / configure_proj / configure_set, of grid_ctx and of what they call, by site:
# (the text, a request that reaches it).  The texts are literals.
BY_BRANCH = [
    # grid_ctx (the engine's constructor)
    ("ndim must be 2 or 3", "set ndim=4 n=3,4,5"),
    ("grid size must be positive", "set ndim=2 n=3,0,1"),
    ("grids of 2^31 points or more are not supported", "set ndim=2 n=65536,32768,1"),
    # configure_op
    ("D_y needs a 3-D grid", req(G2, op=2)),
    ("D_y needs a 3-D grid", req((4, 4, 1), op=2)),
    ("provided an unknown transform domain operator. check function get_TD_operator(comp_grid,TD_type,TF) "
     "for options (TV_xy is the in-plane gradient of a 3-D grid; on a 2-D grid TV is in-plane already)", req(G2, op=6)),
    ("unknown operator kind", req(G2, op=9)),
    ("difference operator along a dimension of size 1", req((1, 4), op=1)),
    ("difference operator along a dimension of size 1", req((1, 4), op=4)),
    # configure_custom
    ("custom operator: CSC arrays missing", req(G2, op=5, csc="missing")),
    ("custom operator: CSC arrays missing", req(G2, op=5, csc="0/0,0,0,0,0,0,0,0,0,0,0,0,0/")),
    ("custom operator: colptr must start at 0 (0-based arrays)", req(G2, op=5, csc="2/1,1,1,2,2,2,2,2,2,2,2,2,2/0,1")),
    ("custom operator: colptr must be non-decreasing", req(G2, op=5, csc="2/0,1,0,2,2,2,2,2,2,2,2,2,2/0,1")),
    ("custom operator: row index out of range", req(G2, op=5, csc="2/0,1,1,2,2,2,2,2,2,2,2,2,2/0,2")),
    ("custom operator: row index out of range", req(G2, op=5, csc="2/0,1,1,2,2,2,2,2,2,2,2,2,2/-1,1")),
    ("custom operator: rows must ascend inside a column", req(G2, op=5, csc="2/0,2,2,2,2,2,2,2,2,2,2,2,2/1,0")),
    ("custom operator: rows must ascend inside a column", req(G2, op=5, csc="2/0,2,2,2,2,2,2,2,2,2,2,2,2/1,1")),
    # configure_proj: component, mode, direction
    ("Minkowski component must be 0, 1, 2 or 3", req(G2, comp=4)),
    ("Minkowski component must be 0, 1, 2 or 3", req(G2, comp=-1)),
    ("unknown application mode", req(G2, mode=3)),
    ("application mode: direction out of range for this grid", req(G2, proj=2, pmax=1.0, mode=1, dir=2)),
    ("application mode: direction out of range for this grid", req((4, 4, 1), proj=2, pmax=1.0, mode=1, dir=2)),
    ("application mode: direction out of range for this grid", req(G3, proj=2, pmax=1.0, mode=2, dir=-1)),
    (FRAMES_Z, req(G3, op=6, proj=14, pmax=1.0, mode=1, dir=2)),
    (ONE_BLOCK_MODE, req(G3, op=4, proj=2, pmax=1.0, mode=1, dir=0)),
    (ONE_BLOCK_EXT, req(G3, op=4, proj=8, pmax=2.0)),
    # ... the l1 radius, site by site: per segment (scalar), behind the DCT, behind the wavelet transform, the whole array, behind the
    # DFT, the l2,1 ball (whole, per frame)
    (L1_RADIUS, req(G3, proj=2, pmax=0.0, mode=1, dir=0)),
    (L1_RADIUS, req(G2, proj=2, pmax=0.0, tr=1)),
    (L1_RADIUS, req((8, 8), proj=2, pmax=-1.0, tr=2)),
    (L1_RADIUS, req(G2, proj=2, pmax=float("nan"))),
    (L1_RADIUS, req(G2, proj=7, pmax=0.0)),
    (L1_RADIUS, req(G2, op=4, proj=14, pmax=0.0)),
    (L1_RADIUS, req(G3, op=6, proj=14, pmax=-2.0, mode=2, dir=2)),
    # ... transforms
    (DCT_DOMAIN, req(G2, op=1, tr=1)),
    (DCT_DOMAIN, req(G2, tr=1, mode=1, dir=0)),
    ("behind the DCT: bounds, the l1 ball and cardinality are built (l2 / annulus commute with it)", req(G2, proj=3, pmax=1.0, tr=1)),
    (NEED_LB_UB, req(G2, proj=1, tr=1, lb=ONES12)),
    (DWT_DOMAIN, req((8, 8), op=1, tr=2)),
    ("behind the wavelet transform: scalar bounds, the l1 ball and cardinality are built (l2 / annulus commute "
     "with it; per-element bounds would depend on the coefficient layout)", req((8, 8), proj=1, tr=2)),
    ("wavelet transform: the grid 8 x 12 has 3 levels (2^L divides the smallest dimension) but dimension 2 is not divisible by 2^3",
     req((8, 12), tr=2)),
    ("unknown transform", req(G2, tr=7)),
    # ... the kinds
    ("scalar bounds apply to the whole array (use per-fiber vectors)", req(G2, proj=0, mode=1, dir=0)),
    ("prox_l1 applies to the whole array", req(G2, proj=6, mode=1, dir=0)),
    (NEED_LB_UB, req(G2, proj=1, ub=ONES12)),
    ("bound constraints per slice of a tensor currently not implemented, yet...", req(G3, proj=1, mode=2, dir=0, lb="1,1,1", ub="2,2,2")),
    ("the DFT-l1 projector acts in its own domain: TD_OP must be the identity, mode matrix/tensor", req(G2, op=1, proj=7, pmax=1.0)),
    ("bounds in the DFT domain act in their own domain: TD_OP must be the identity, mode matrix/tensor", req(G2, proj=12, mode=1, dir=0)),
    ("bounds in the DFT domain need the mask vector (constraint.max)", req(G2, proj=12, lb=ONES12)),
    ("cardinality behind the DFT acts in its own domain: TD_OP must be the identity, mode matrix/tensor", req(G2, op=3, proj=13, pmax=2.0)),
    ("cardinality behind the DFT: k must be a non-negative integer", req(G2, proj=13, pmax=1.5)),
    ("cardinality behind the DFT: k must be a non-negative integer", req(G2, proj=13, pmax=-1.0)),
    (L21_NEEDS_TV, req(G2, op=1, proj=14, pmax=1.0)),
    ("the l2,1 ball takes no Minkowski component", req(G2, op=4, proj=14, pmax=1.0, comp=1)),
    (SHARDED["l21"], req(G2, op=4, proj=14, pmax=1.0, single=0)),
    (L1_RADIUS + " (segment 2)", req(G3, op=6, proj=14, mode=2, dir=2, ub="1,1,0,1,-1")),
    ("histogram constraints need sorted lb and ub vectors", req(G2, proj=10, lb=ONES12)),
    ("subspace constraints act on the model itself: TD_OP must be the identity", req(G2, op=1, proj=11, basis="12x2")),
    ("subspace constraints need the matrix A", req(G2, proj=11)),
    ("subspace constraints need the matrix A", req(G2, proj=11, basis="12x0")),
    ("unknown projector kind", req(G2, proj=99)),
    # ... vector radii
    (SHARDED["radii"], req(G2, proj=3, mode=1, dir=0, ub="1,1,1,1", single=0)),
    (L1_RADIUS + " (segment 1)", req(G2, proj=2, mode=1, dir=0, ub="1,0,1,-1")),
    # configure_set
    (SHARDED["tv_xy"], req(G3, op=6, proj=2, pmax=1.0, single=0)),
    (TV_XY_NO_COMPONENT, req(G3, op=6, proj=2, pmax=1.0, comp=1)),
    ("custom sparse operators (SIPX_OP_CSC): Minkowski components and library-backed projectors are not available; "
     "use one of the built-in operators for such a set", req(G2, op=5, comp=1) + " " + CSC_OK),
    ("custom sparse operators (SIPX_OP_CSC): Minkowski components and library-backed projectors are not available; "
     "use one of the built-in operators for such a set", req(G2, op=5, proj=8, pmax=1.0) + " " + CSC_OK),
    ("custom sparse operator (SIPX_OP_CSC) without its A'A: the matrix-free term of Q uses 32-bit indices and needs "
     "fewer than 2^31 columns, rows and stored entries (12, 2147483648, 5 given) -- split the operator into several sets", "mf 12 2147483648 5"),
    ("Minkowski sets use descriptor-generated AtA (pass ata_R = NULL)", req(G2, op=1, comp=1, ata="3:-1,0,1")),
    ("AtA band count out of range (1..9 bands per set)", req(G2, op=1, ata="0:")),
    ("AtA band count out of range (1..9 bands per set)", req(G2, op=1, ata="10:-5,-4,-3,-2,-1,0,1,2,3,4")),
]


def test_every_refusal_by_branch(ask):
    got = ask(line for _, line in BY_BRANCH)
    for (want, line), g in zip(BY_BRANCH, got):
        assert g == want, line
    # ... and no throw of the header is left without a case: the first literal of each is the start of a text above
    texts = {want for want, _ in BY_BRANCH}
    sources = _read(HEADER) + _read(os.path.join(CSRC, "dwt.h"))
    firsts = re.findall(r'throw std::runtime_error\(\s*(?:std::string\()?"((?:[^"\\]|\\.)*)"', sources)
    assert len(firsts) >= 50                              # (the pattern does find the throws)
    for lit in firsts:
        lit = lit.encode().decode("unicode_escape")
        if lit.startswith("wavelet transform: ") and lit != "wavelet transform: the grid ":      # dwt_check_grid's own: test_wavelet_grid_rule
            continue
        assert any(t.startswith(lit) for t in texts), lit


def test_refusals_the_gpu_tests_assert_come_back_verbatim(ask):
    """tests/test_gpu_l21.py, test_gpu_l21_frames.py, test_gpu_seg_radii.py and test_gpu_device_memory.py: the same descriptors"""
    TV, XY = OPS["TV"], OPS["TV_xy"]
    cases = []
    for n in ((16, 12), (16, 12, 8)):                                    # test_gpu_l21.test_engine_refusals
        cases += [(L21_NEEDS_TV, req(n, op=OPS[op], proj=14, pmax=1.0)) for op in ("identity", "D_x", "D_z")]
        cases += [(ONE_BLOCK_MODE, req(n, op=TV, proj=14, pmax=1.0, mode=1)), (L21_NEEDS_TV, req(n, op=0, proj=14, pmax=1.0, mode=1))]
        cases += [(L1_RADIUS, req(n, op=TV, proj=14, pmax=r)) for r in (0.0, -2.0, float("nan"))]
        cases += [(DCT_DOMAIN, req(n, op=TV, proj=14, pmax=1.0, tr=1)), (DWT_DOMAIN, req(n, op=TV, proj=14, pmax=1.0, tr=2)),
                  (ONE_BLOCK_EXT, req(n, op=TV, proj=PROJ["rank"], pmax=1.0))]
    n = (16, 12, 8)                                                      # test_gpu_l21_frames.test_engine_refusals
    cases += [(FRAMES_Z, req(n, op=XY, proj=14, pmax=1.0, mode=mode, dir=dr)) for mode, dr in ((2, 0), (2, 1), (1, 0), (1, 1), (1, 2))]
    cases += [(ONE_BLOCK_MODE, req(n, op=TV, proj=14, pmax=1.0, mode=2, dir=2))]
    cases += [(ONE_BLOCK_MODE, req(n, op=XY, proj=PROJ[p], pmax=1.0, mode=2, dir=2)) for p in ("l1", "l2", "annulus", "cardinality")]
    cases += [(L21_NEEDS_TV, req(n, op=OPS[op], proj=14, pmax=1.0, mode=2, dir=2)) for op in ("identity", "D_x", "D_z")]
    cases += [(ONE_BLOCK_EXT, req(n, op=XY, proj=PROJ["rank"], pmax=1.0))]
    for r in (0.0, -2.0, float("nan")):
        cases += [(L1_RADIUS, req(n, op=XY, proj=14, pmax=r)), (L1_RADIUS, req(n, op=XY, proj=14, pmax=r, mode=2, dir=2))]
    ub = np.ones(n[2], np.float32)
    ub[5] = 0
    cases += [(L1_RADIUS + " (segment 5)", req(n, op=XY, proj=14, pmax=1.0, mode=2, dir=2, ub=ub)),
              (TV_XY_NO_COMPONENT, req(n, op=XY, proj=PROJ["l1"], pmax=1.0, comp=1)),
              (DCT_DOMAIN, req(n, op=XY, proj=14, pmax=1.0, tr=1))]
    r = np.ones(16, np.float64)                                           # test_gpu_seg_radii: the 16 fibers along z of (16, 12), three bad radii
    r[[3, 5, 7]] = 0.0, -1.0, float("nan")
    cases += [(L1_RADIUS + " (segment 3)", req((16, 12), "d", proj=PROJ["l1"], mode=1, dir=1, ub=r))]
    m = 1 << 10                                                           # test_gpu_device_memory: the descriptors of its refused sipx_project calls
    cases += [(L1_RADIUS, req((m, 1), proj=PROJ["l1"], pmax=-1.0)), (NEED_LB_UB, req((m, 1), proj=PROJ["bounds_vec"], ub=f"fill:{m}:1"))]
    for (want, line), g in zip(cases, ask(line for _, line in cases)):
        assert g == want, line


def test_sharded_contexts_refuse_what_single_process_contexts_take(ask):
    sets = {"radii": [req(G3, proj=PROJ["l1"], mode=1, dir=0, ub=[1.0] * 20), req(G3, op=OPS["D_z"], proj=PROJ["l2"], mode=2, dir=2, ub=[1.0] * 4),
                      req(G3, op=OPS["D_x"], proj=PROJ["annulus"], mode=1, dir=1, ub=[2.0] * 10),
                      req(G3, proj=PROJ["annulus"], mode=2, dir=0, lb=[1.0] * 3, pmax=3.0)],
            "l21": [req(G2, op=4, proj=14, pmax=1.0), req(G3, op=4, proj=14, pmax=1.0)],
            # (the operator is looked at before the projector: the l2,1 ball on TV_xy is refused in the operator's words)
            "tv_xy": [req(G3, op=6, proj=PROJ[p], pmax=1.0) for p in ("bounds", "l1", "l2", "cardinality", "l21")] +
                     [req(G3, op=6, proj=14, pmax=1.0, mode=2, dir=2), req(G3, op=6, proj=14, mode=2, dir=2, ub=[1.0] * 5)]}
    for which, lines in sets.items():
        for g in ask(k + " single=0" for k in lines):
            assert g == SHARDED[which], which
        for g in ask(k + " single=1" for k in lines):
            assert isinstance(g, dict), (which, g)
    # scalar radii need no single process
    assert isinstance(ask([req(G3, proj=PROJ["l1"], pmax=1.0, mode=1, dir=0, single=0)])[0], dict)


# ---- rows, offsets, 1/h against the oracle's sparse operators -----------------------------------------------------------------------------
def _oracle_blocks(n, op, TF):
    """the operator's blocks in the engine's order (z[, y], x), as sparse matrices; None where a dimension has one point"""
    g = O.compgrid(SPACING[:len(n)], n)
    n2 = tuple(n[:2]) if len(n) == 3 and n[2] == 1 else tuple(n)
    names = {"D_x": ["D_x"], "D_y": ["D_y"], "D_z": ["D_z"], "TV": ["D_z", "D_y", "D_x"] if len(n2) == 3 else ["D_z", "D_x"],
             "TV_xy": ["D_y", "D_x"]}[op]
    return [O.get_TD_operator(g, k, TF)[0] for k in names], n2


@pytest.mark.parametrize("code,TF", TYPES)
def test_rows_offsets_and_spacing_equal_the_oracle(ask, code, TF):
    seen = 0
    for n in GRIDS:
        n2 = tuple(n[:2]) if len(n) == 3 and n[2] == 1 else tuple(n)
        N = int(np.prod(n))
        got = ask([req(n, code, op=OPS["identity"])])[0]
        assert int(got["ndim"]) == len(n2) and int(got["Mtrue"]) == int(got["Mpad"]) == N and ints(got["ata_off"]) == [0]
        assert int(got["nblk"]) == 0 and int(got["ident"]) == 1
        for op in ("D_x", "D_y", "D_z", "TV", "TV_xy"):
            got = ask([req(n, code, op=OPS[op])])[0]
            axes = {"D_x": [0], "D_y": [1], "D_z": [len(n2) - 1], "TV": list(range(len(n2)))[::-1], "TV_xy": [1, 0]}[op]
            if op in ("D_y", "TV_xy") and len(n2) == 2:
                assert isinstance(got, str) and ("3-D grid" in got), (n, op, got)
                continue
            if any(n2[a] < 2 for a in axes):           # the oracle's block has no rows: nothing to constrain
                assert got == "difference operator along a dimension of size 1", (n, op)
                continue
            blocks, _ = _oracle_blocks(n, op, TF)
            A = sp.vstack(blocks, format="csc")
            assert int(got["Mtrue"]) == A.shape[0] and A.shape[1] == N, (n, op)
            assert ints(got["blk_rows"])[:len(blocks)] == [b.shape[0] for b in blocks], (n, op)
            assert int(got["nblk"]) == len(blocks) and ints(got["dir"])[:len(blocks)] == axes and int(got["Mpad"]) == len(blocks) * N
            AtA = sp.csc_matrix(A.T @ A)
            AtA.eliminate_zeros()
            assert ints(got["ata_off"]) == list(O.mat2CDS(AtA, TF)[1]), (n, op)
            # the entries of block q are -+1/h of its direction, rounded as the oracle's operator rounds them
            ih = [float.fromhex(v) for v in got["ih"].split(",")]
            for q, b in enumerate(blocks):
                assert ih[q] == float(np.abs(b.data).max()) == float(TF(1) / TF(SPACING[axes[q]])), (n, op, q)
            seen += 1
    assert seen >= 9
    # a Minkowski sum set [A A]: the offsets of the 2N x 2N block matrix
    for n, op in ((G2, "D_x"), (G3, "TV"), (G2, "identity")):
        blocks = [sp.identity(int(np.prod(n)), dtype=TF, format="csc")] if op == "identity" else _oracle_blocks(n, op, TF)[0]
        A = sp.vstack(blocks, format="csc")
        B = sp.hstack([A, A], format="csc")
        BtB = sp.csc_matrix(B.T @ B)
        BtB.eliminate_zeros()
        got = ask([req(n, code, op=OPS[op], comp=3)])[0]
        assert ints(got["ata_off"]) == list(O.mat2CDS(BtB, TF)[1]), (n, op)
    # bands the caller supplies are kept as given
    got = ask([req(G2, code, op=1, ata="2:0,1")])[0]
    assert ints(got["ata_off"]) == [0, 1] and int(got["nata"]) == 2 * 12


# ---- vector lengths and segment counts against host.Projector --------------------------------------------------------------------------------
def test_data_len_and_segment_count_equal_the_host_projector(sipx, ask):
    host = sipx.host
    TF = np.float32
    lines, want = [], []
    for n in (G2, G3, (4, 4, 1)):
        g = sipx.compgrid(SPACING[:len(n)], n)
        n2 = host._grid(g)[0]
        letters = ("x", "z") if len(n2) == 2 else ("x", "y", "z")
        modes = [("matrix", "")] + [(m, d) for m in ("fiber", "slice") for d in letters]
        if len(n) == 3 and n[2] == 1:
            modes.remove(("slice", "z"))         # (the one plane of such a tensor: the front end's name for the whole array)
        for opname in ("identity", "D_x", "D_y", "D_z", "TV", "TV_xy"):
            if opname == "D_y" and len(n2) == 2:      # (refused where the front end builds operators, get_TD_operator, not in TDOperator)
                continue
            try:
                op = host.TDOperator(opname, g, TF)
            except host.SipxError:
                continue
            for mode in modes:
                def vec(count, value=1.0):
                    return np.full(count, value, TF)
                td_n = list(op.n)
                if opname in ("D_x", "D_y", "D_z"):
                    td_n[{"D_x": 0, "D_y": 1, "D_z": len(td_n) - 1}[opname]] -= 1
                axis = {"x": 0, "y": 1, "z": len(n2) - 1}.get(mode[1], 0)
                nseg = {"matrix": 1, "fiber": int(np.prod(td_n)) // td_n[axis], "slice": td_n[axis]}[mode[0]]
                rows = op.shape[0]
                sets = [("bounds", 0.0, 1.0), ("bounds", vec(rows if mode[0] == "matrix" else td_n[axis], 0.0), vec(rows if mode[0] == "matrix" else td_n[axis])),
                        ("l1", 0.0, 2.0), ("l2", 0.0, 2.0), ("annulus", 1.0, 2.0), ("cardinality", 0, 3), ("rank", 0, 2), ("nuclear", 0.0, 2.0),
                        ("histogram", vec(rows, 0.0), vec(rows)), ("l21", 0.0, 2.0)]
                if mode[0] != "matrix":          # one radius per segment
                    sets += [("l1", 0.0, vec(nseg, 2.0)), ("l2", 0.0, vec(nseg, 2.0)), ("annulus", vec(nseg), vec(nseg, 2.0)),
                             ("annulus", vec(nseg), 2.0), ("l21", 0.0, vec(n2[-1], 2.0))]
                for st, lo, hi in sets:
                    try:
                        P = host.Projector(sipx.set_definitions(st, opname, lo, hi, mode), g, TF)
                        P.check_rows(op)
                    except host.SipxError:
                        continue
                    d = P.desc(opname, False)
                    kw = dict(op=d.op, proj=d.proj, pmin=d.pmin, pmax=d.pmax, mode=d.mode, dir=d.dir, tr=d.transform)
                    if P.lb is not None:
                        kw["lb"] = P.lb
                    if P.ub is not None:
                        kw["ub"] = P.ub
                    lines.append(req(n, "f", **kw))
                    want.append((P.data_len(op), P.nseg(op), (st, opname, mode, n)))
    got = ask(lines)
    compared_len = compared_seg = 0
    refused = {}
    for g, (dl, ns, what) in zip(got, want):
        if isinstance(g, str):                 # the front end has no rule of its own for these: the engine's word is final
            refused.setdefault(g, []).append(what)
            continue
        if dl is not None:
            assert int(g["data_len"]) == dl, what
            compared_len += 1
        if ns and int(g["ext_kind"]):
            assert int(g["nseg"]) == ns, what
            compared_seg += 1
        if int(g["seg_radii"]):
            assert int(g["nub"]) == dl, what
    assert compared_len >= 60 and compared_seg >= 60, (compared_len, compared_seg)
    # what the engine refuses of the front end's descriptors is what the front end leaves to it, and nothing else
    assert set(refused) <= {ONE_BLOCK_MODE, ONE_BLOCK_EXT, "scalar bounds apply to the whole array (use per-fiber vectors)"}, refused


# ---- per-fiber bounds ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("code,TF", TYPES)
def test_fiber_bounds_expand_like_a_numpy_broadcast(ask, code, TF):
    n = G3
    rng = np.random.default_rng(3)
    for opname, cut in (("identity", None), ("D_x", 0), ("D_y", 1), ("D_z", 2)):
        td_n = [n[a] - (1 if a == cut else 0) for a in range(3)]
        for bdir in range(3):
            lb = rng.standard_normal(td_n[bdir]).astype(TF)
            ub = (lb + 1).astype(TF)
            got = ask([req(n, code, op=OPS[opname], proj=PROJ["bounds_vec"], mode=1, dir=bdir, lb=lb, ub=ub, dump=1)])[0]
            shape = [1, 1, 1]
            shape[bdir] = td_n[bdir]
            for name, v in (("host_lb", lb), ("host_ub", ub)):
                want = np.broadcast_to(v.reshape(shape), td_n).reshape(-1, order="F")
                have = np.array([float.fromhex(t) for t in got[name].split(",")])
                assert have.shape == want.shape and np.array_equal(have, want.astype(np.float64)), (opname, bdir, name)
            assert int(got["data_len"]) == td_n[bdir] and int(got["Mtrue"]) == int(np.prod(td_n)) and float.fromhex(got["plo"]) == 1.0
    # one bound per row: taken as given, clipped the other way round
    got = ask([req(n, code, op=OPS["D_x"], proj=PROJ["bounds_vec"], lb=[0.0] * 40, ub=[1.0] * 40)])[0]
    assert (int(got["nlb"]), int(got["nub"]), int(got["data_len"]), float.fromhex(got["plo"])) == (40, 40, 40, 0.0)


# ---- routes -------------------------------------------------------------------------------------------------------------------------------
def test_routes_and_scratch_flags(ask):
    n = G3
    N = 60
    rows = [  # request, prox, ext_kind, two_pass, needs_ext, needs_idx
        (req(n, proj=PROJ["bounds"], pmin=0.0, pmax=1.0), PROJ["bounds"], 0, 0, 0, 0),
        (req(n, proj=PROJ["prox_l1"], pmax=1.0), PROJ["prox_l1"], 0, 0, 0, 0),
        (req(n, op=4, proj=PROJ["l1"], pmax=1.0), PROJ["l1"], 0, 1, 0, 0),
        (req(n, proj=PROJ["l2"], pmax=1.0), PROJ["l2"], 0, 1, 0, 0),
        (req(n, proj=PROJ["annulus"], pmin=1.0, pmax=2.0), PROJ["annulus"], 0, 1, 0, 0),
        (req(n, proj=PROJ["cardinality"], pmax=3.0), PROJ["cardinality"], 0, 1, 0, 1),
        (req(n, proj=PROJ["cardinality"], pmax=3.0, mode=1, dir=0), PX_EXT, EXT["card_seg"], 0, 1, 0),
        (req(n, op=1, proj=PROJ["l1"], pmax=1.0, mode=1, dir=2), PX_EXT, EXT["l1_seg"], 0, 1, 0),
        (req(n, proj=PROJ["l2"], pmax=1.0, mode=2, dir=1), PX_EXT, EXT["l2_seg"], 0, 1, 0),
        (req(n, proj=PROJ["annulus"], pmin=1.0, pmax=2.0, mode=2, dir=2), PX_EXT, EXT["annulus_seg"], 0, 1, 0),
        (req(n, proj=PROJ["l1_dft"], pmax=1.0), PX_EXT, EXT["l1_dft"], 0, 1, 0),
        (req(n, proj=PROJ["bounds_dft"], ub=f"fill:{N}:1"), PX_EXT, EXT["dft_mask"], 0, 1, 0),
        (req(n, proj=PROJ["card_dft"], pmax=4.0), PX_EXT, EXT["card_dft"], 0, 1, 0),
        (req(n, proj=PROJ["rank"], pmax=2.0, mode=2, dir=2), PX_EXT, EXT["rank"], 0, 1, 0),
        (req(n, proj=PROJ["nuclear"], pmax=2.0, mode=2, dir=0), PX_EXT, EXT["nuclear"], 0, 1, 0),
        (req(n, op=3, proj=PROJ["histogram"], lb="fill:48:0", ub="fill:48:1"), PX_EXT, EXT["histogram"], 0, 1, 0),
        (req(n, proj=PROJ["subspace"], basis="60x3", orth=1), PX_EXT, EXT["subspace"], 0, 1, 0),
        (req(n, proj=PROJ["l1"], pmax=1.0, tr=1), PX_EXT, EXT["dct"], 0, 1, 0),
        (req((8, 8), proj=PROJ["cardinality"], pmax=5.0, tr=2), PX_EXT, EXT["dwt"], 0, 1, 0),
        (req(n, op=4, proj=PROJ["l21"], pmax=1.0), PX_EXT, EXT["l21"], 0, 1, 0),
        (req(n, op=6, proj=PROJ["l21"], pmax=1.0), PX_EXT, EXT["l21"], 0, 1, 0),
        (req(n, op=6, proj=PROJ["l21"], pmax=1.0, mode=2, dir=2), PX_EXT, EXT["l21_seg"], 0, 1, 0)]
    for (line, prox, ext, two, need_ext, need_idx), g in zip(rows, ask(r[0] for r in rows)):
        assert isinstance(g, dict), (line, g)
        assert [int(g[k]) for k in ("prox", "ext_kind", "two_pass", "needs_ext", "needs_idx")] == [prox, ext, two, need_ext, need_idx], line
    g = dict(zip((r[0] for r in rows), ask(r[0] for r in rows)))
    seg = g[rows[7][0]]                       # l1 per fiber along z behind D_x: TD_n = (2, 4, 5), 8 fibers
    assert (ints(seg["spec.dims"]), int(seg["spec.mode"]), int(seg["spec.dir"]), int(seg["nseg"]), int(seg["spec.nblk"])) == ([2, 4, 5], 1, 2, 8, 1)
    assert int(g[rows[17][0]]["spec.inner"]) == PROJ["l1"] and int(g[rows[18][0]]["spec.inner"]) == PROJ["cardinality"]
    frames = g[rows[21][0]]
    assert (int(frames["spec.nblk"]), ints(frames["spec.bdir"]), ints(frames["spec.dims"]), int(frames["nseg"])) == (2, [1, 0, 0], [3, 4, 5], 5)
    assert (int(g[rows[19][0]]["spec.nblk"]), ints(g[rows[19][0]]["spec.bdir"])) == (3, [2, 1, 0])
    assert (int(g[rows[15][0]]["nlb"]), int(g[rows[15][0]]["nub"]), int(g[rows[16][0]]["nbasis"])) == (48, 48, 180)
    # a custom operator: with its bands a set like any other, without them a matrix-free term of Q
    with_bands, without = ask([req(G2, op=5, proj=PROJ["l1"], pmax=1.0, ata="1:0") + " " + CSC_OK, req(G2, op=5, proj=PROJ["l1"], pmax=1.0) + " " + CSC_OK])
    assert [int(with_bands[k]) for k in ("custom", "mfree", "Mtrue", "Mpad", "nblk", "ident", "two_pass")] == [1, 0, 2, 2, 0, 0, 1]
    assert int(without["mfree"]) == 1 and without["ata_off"] == "" and ints(with_bands["ata_off"]) == [0]


def test_matrix_free_index_range_through_sizes_only(ask):
    lim = 1 << 31
    got = ask([f"mf {lim - 1} {lim - 1} {lim - 1}", f"mf {lim} 5 5", f"mf 5 {lim} 5", f"mf 5 5 {lim}"])
    assert got[0] == {} and all(isinstance(g, str) and "fewer than 2^31 columns, rows and stored entries" in g for g in got[1:])
    assert f"({lim}, 5, 5 given)" in got[1] and f"(5, {lim}, 5 given)" in got[2] and f"(5, 5, {lim} given)" in got[3]


# ---- the wavelet grid rule -----------------------------------------------------------------------------------------------------------------
def test_wavelet_grid_rule(ask):
    grids = [(8, 12), (6, 10), (8, 16), (16, 8, 24), (12, 8, 10), (7, 9), (4, 4, 1)]
    got = ask(f"dwt {len(n)} {n[0]} {n[1]} {n[2] if len(n) == 3 else 1}" for n in grids)
    for n, g in zip(grids, got):
        L = 0
        while min(n) % (2 ** (L + 1)) == 0:           # the largest L with 2^L dividing the smallest dimension
            L += 1
        bad = [a for a in range(len(n)) if n[a] % 2 ** L]
        if bad:
            assert g == (f"wavelet transform: the grid {' x '.join(str(v) for v in n)} has {L} levels (2^L divides the smallest "
                         f"dimension) but dimension {bad[0] + 1} is not divisible by 2^{L}"), n
        else:
            assert g == {"levels": str(L)}, n
    assert isinstance(got[0], str) and got[1] == {"levels": "1"}
    assert ask(["dwt 1 8 1 1", "dwt 2 8 0 1", "dwt 3 2048 2048 512"]) == [
        "wavelet transform: 2-D and 3-D grids only", "wavelet transform: empty grid",
        "wavelet transform: grids of 2^31 points and more are not supported"]
    # through a set: refused on (8, 12), taken on (6, 10); a 3-D grid of one plane is a 2-D grid
    a, b, c = ask([req((8, 12), proj=PROJ["l1"], pmax=1.0, tr=2), req((6, 10), proj=PROJ["l1"], pmax=1.0, tr=2), req((4, 4, 1), proj=PROJ["bounds"], tr=2)])
    assert isinstance(a, str) and a.startswith("wavelet transform: the grid 8 x 12 has 3 levels")
    assert int(b["ext_kind"]) == EXT["dwt"] and int(c["ext_kind"]) == EXT["dwt"] and int(c["ndim"]) == 2
