"""The l2,1 ball across the blocks of a stacked operator and the named operator "Hessian" without a GPU: the numpy reference
(tests/l21_stacked_ref.py) against the properties of a projection, csrc/l21_stacked.h on the CPU (tests/l21_stacked/rule_driver.cpp,
compiled by hipcc; the program makes no HIP call) against a numpy emulation of the contract bit for bit, the "Hessian" operator of the
front end entry by entry, the descriptor rules of csrc/set_config.h (tests/l21_stacked/config_driver.cpp), the front end's refusals
and the C ABI's appended field.

THE MIXED BLOCKS ON POLYNOMIALS.  The entries of a mixed block are +-w with w = fl(sqrt 2 ih_a ih_b), which is not a power of two: a
sparse product w x00 - w x10 - w x01 + w x11 rounds every term, so on integer data it is exact only up to a few ulp of w max|x| and
not "exactly zero" on an affine x.  What is exact is the stencil: the block with its entries divided by w (exactly +-1) applied to
integer data.  The tests therefore hold (a) every entry of the matrix to the dense reference bit for bit, (b) the pure blocks on
integer polynomials exactly, (c) the mixed blocks divided by w exactly, w itself to the correctly rounded product, and (d) the plain
product H x of the mixed blocks to 4 eps w max|x|, the bound of four rounded terms."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from tests import l1_exact
from tests import l21_stacked_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "setintersectionprojection.jl_amd", "csrc")
BLOCKS = [1, 2, 3, 6, 8]


def _heavy(rng, M):
    return rng.standard_normal(M) * np.exp(rng.standard_normal(M))


# ---- the reference is a projection -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("frac", [0.9, 0.5, 0.05])
def test_reference_is_the_projection(B, frac):
    TF = np.float64
    eps = float(np.finfo(TF).eps)
    G = 37
    rng = np.random.default_rng(11 + B)
    v = _heavy(rng, B * G).astype(TF)
    v.reshape(B, G)[:, 5] = 0.0      # (a zero group, as the last corner of the Hessian is: the cap of the search below never binds)
    b = TF(frac * R.norm21(v, B))
    y = R.project(v, B, b)
    assert y is not v
    assert float(b) * (1 - 4 * eps) <= R.norm21(y, B) <= float(b) * (1 + 4 * eps)
    for k in range(100):      # <v - y, z - y> <= 0 for every z of the ball, up to the rounding of y (tests/test_l21_cpu.py)
        z = _heavy(rng, B * G)
        if k % 4 == 0:
            z[rng.random(B * G) < 0.7] = 0.0
        z *= (1.0 if k % 5 == 0 else rng.random()) * float(b) * (1 - 8 * eps) / R.norm21(z, B)
        assert float(np.dot(v - y, z - y)) <= 64 * eps * np.linalg.norm(v - y) * np.linalg.norm(z - y)
    assert R.project(v, B, TF(2 * R.norm21(v, B))) is v, "a feasible input comes back itself"


def test_reference_keeps_the_cap_of_the_l1_search():
    """The threshold is that of the engine's l1 search, which keeps the reference's `rho + 1 < lv` (project_l1_Duchi!.jl): the active
    set never holds all entries, so where the exact projection would zero no group the smallest one is left out of the sum and theta
    comes out below the exact one (here clamped at 0: the point stays as it is).  On the Hessian the last corner has g = 0 and the cap
    never binds; on a caller-supplied operator without a zero group it can, as it can for the l1 ball on such an operator."""
    v = np.array([3.0, 4.0, 5.0, 0.0, 3.0, 12.0])      # B = 2, G = 3: g = (3, 5, 13), sum 21 > 20
    th, C, S = l1_exact.exact_theta(np.array([3.0, 5.0, 13.0]), 20.0)
    assert (th, C, S) == (0.0, 2, 18.0)                 # (18 - 20) / 2 < 0 -> 0, where the exact threshold is 1 / 3
    assert np.array_equal(R.project(v, 2, 20.0), v)
    v0 = np.concatenate([v[:3], [0.0], v[3:], [0.0]])   # with a zero group the threshold is the exact one
    y = R.project(v0, 2, 20.0).reshape(2, 4)
    assert np.allclose(np.sqrt((y ** 2).sum(axis=0)), [3 - 1 / 3, 5 - 1 / 3, 13 - 1 / 3, 0], rtol=1e-15)


def test_reference_with_one_block_is_the_l1_ball():
    v = _heavy(np.random.default_rng(3), 50)
    b = 0.3 * np.abs(v).sum()
    th, _, _ = l1_exact.exact_theta(np.abs(v), b)
    assert np.allclose(R.project(v, 1, b), np.sign(v) * np.maximum(np.abs(v) - th, 0), rtol=1e-14, atol=0)


# ---- csrc/l21_stacked.h on the CPU ---------------------------------------------------------------------------------------------------------
def _compile(tmp_path_factory, name):
    hipcc = shutil.which("hipcc") or shutil.which("hipcc", path=os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin"))
    assert hipcc, "hipcc not found"
    exe = str(tmp_path_factory.mktemp("l21_stacked") / name)
    r = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                        "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "l21_stacked", name + ".cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _compile(tmp_path_factory, "rule_driver")


def emulate(v, B, theta):
    """The contract of csrc/l21_stacked.h in numpy, in v's precision: (g, f, y) of the B blocks of v."""
    TF = v.dtype.type
    g = R.norms(v, B, TF)
    t = (g - TF(theta)).astype(TF)
    t = np.where(t > 0, t, TF(0)).astype(TF)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(g > 0, (t / g).astype(TF), TF(0)).astype(TF)
    y = (v.reshape(B, -1) * f[None, :]).astype(TF).reshape(-1)
    return g, f, y


def _rule_input(B, TF):
    """G = 64 groups: heavy-tailed, then an all-zero group (0), a group of -0.0 (1), one group holding most of the norm (2), scattered
    zeros of both signs, and integer ties (3, 4 -> 5)."""
    rng = np.random.default_rng(17 + B)
    G = 64
    v = _heavy(rng, B * G).astype(TF).reshape(B, G)
    v[:, 0] = 0.0
    v[:, 1] = -0.0
    v[:, 2] = TF(1e6) * (1 + np.arange(B))
    v[:, 10:20][rng.random((B, 10)) < 0.5] = -0.0
    v[:, 20:30][rng.random((B, 10)) < 0.5] = 0.0
    v[:, 3] = 0.0
    v[0, 3] = 3.0
    v[B - 1, 3] = 4.0 if B > 1 else 3.0
    return np.ascontiguousarray(v.reshape(-1))


@pytest.mark.parametrize("TF", [np.float32, np.float64])
@pytest.mark.parametrize("B", BLOCKS)
def test_header_rule_equals_the_emulation_bit_for_bit(driver, TF, B):
    v = _rule_input(B, TF)
    G = v.size // B
    tag = "f" if TF == np.float32 else "d"
    thetas = [TF(0.0), TF(0.75), TF(5.0), TF(2e6), TF(1e30)]      # nothing shrunk ... one group left ... everything zeroed
    lines = [f"{tag} {B} {G} {float(th).hex()} " + " ".join(float(x).hex() for x in v) for th in thetas]
    r = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True)
    out = r.stdout.splitlines()
    assert r.returncode == 0 and out and out[-1] == "ok", r.stdout[-2000:] + r.stderr
    rows = {k: [np.array([float.fromhex(w) for w in ln.split()[1:]]).astype(TF) for ln in out if ln.startswith(k + " ")] for k in "gfy"}
    assert [len(rows[k]) for k in "gfy"] == [len(thetas)] * 3
    for i, th in enumerate(thetas):
        g, f, y = emulate(v, B, th)
        assert l1_exact.same_bits(rows["g"][i], g) and l1_exact.same_bits(rows["f"][i], f) and l1_exact.same_bits(rows["y"][i], y), (B, th)
    g, f, y = emulate(v, B, TF(5.0))
    Y = y.reshape(B, G)
    assert g[0] == 0 and g[1] == 0 and f[0] == 0 and f[1] == 0
    assert np.all(np.signbit(Y[:, 1]) & (Y[:, 1] == 0)), "a group of -0.0 keeps the sign of its zeros"
    assert g[3] == (5 if B > 1 else 3) and f[3] == 0, "a group on the threshold is zeroed"
    g, f, y = emulate(v, B, TF(2e6))
    assert np.count_nonzero(f) == (1 if B > 1 else 0) or B == 1
    assert g[2] == np.max(g) and np.all(f[np.arange(G) != 2] == 0), "one group holds all of the norm that is left"
    assert np.all(emulate(v, B, TF(1e30))[2] == 0)


def test_float64_threshold_is_correctly_rounded(driver):
    """l21_theta_refined on the active set of a plain float64 evaluation of theta (tests/test_l21_cpu.py), on arrays without a zero
    entry -- a stacked operator has no last corner -- and the cap: every entry above the search's theta returns that theta."""
    rng = np.random.default_rng(23)
    cases = []
    for L, frac in ((60, 0.9), (60, 0.5), (660, 0.9), (660, 0.05), (5000, 0.97), (5000, 0.5), (12, 0.9)):
        g = np.abs(rng.standard_normal(L) * np.exp(rng.standard_normal(L))) + 1e-3
        b = frac * float(g.sum())
        th, C, S = l1_exact.exact_theta(g, b)
        act = g[g > th]
        plain = (float(np.sum(act[::-1])) - b) / len(act)
        if len(act) < L:
            cases.append((g, b, th, plain))
    lines = [f"theta {float(b).hex()} {float(p).hex()} {len(g)} " + " ".join(float(x).hex() for x in g) for g, b, _, p in cases]
    lines.append("theta " + float(1.0).hex() + " " + float(0.25).hex() + " 3 " + " ".join(float(x).hex() for x in (1.0, 2.0, 3.0)))
    r = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True)
    out = r.stdout.splitlines()
    assert r.returncode == 0 and out[-1] == "ok", r.stdout[-2000:] + r.stderr
    got = [float.fromhex(k.split()[1]) for k in out if k.startswith("theta ")]
    assert len(got) == len(cases) + 1 and len(cases) >= 5
    worse = 0
    for (g, b, th, plain), t in zip(cases, got):
        assert abs(t - th) <= 2.0 ** -52 * th, (len(g), t, th, plain)
        worse += abs(plain - th) > 2.0 ** -52 * th
    assert worse >= 2, "no case in which the plain evaluation is off: the inputs show nothing"
    assert got[-1] == 0.25, "every entry active: the search's threshold is applied"


def test_shape_rule(driver):
    lines = ["shape 12 3", "shape 12 5", "shape 12 0", "shape 18 9", "shape 8 8", "shape 7 1"]
    out = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True).stdout.splitlines()
    assert out[0] == "shape 4" and out[4] == "shape 1" and out[5] == "shape 7"
    assert "M = 12 rows, not a multiple of blocks = 5" in out[1]
    assert "blocks = 0, the number of equal-sized blocks of the operator must be 1 .. 8" in out[2]
    assert "blocks = 9, the number of equal-sized blocks of the operator must be 1 .. 8" in out[3]


# ---- the named operator "Hessian" ----------------------------------------------------------------------------------------------------------
HESSIAN_GRIDS = [(5, 4), (7, 3), (4, 3, 5)]


def _coords(n):
    return np.unravel_index(np.arange(int(np.prod(n))), n, order="F")


def _block_rows(n, blk):
    """(interior, border) masks over the grid points of one block of the Hessian (tests/l21_stacked_ref.py, hessian_blocks)."""
    c = _coords(n)
    if blk[0] == "pure":
        a = blk[1]
        inside = (c[a] >= 1) & (c[a] <= n[a] - 2)
    else:
        a, b = blk[1], blk[2]
        inside = (c[a] < n[a] - 1) & (c[b] < n[b] - 1)
    return inside, ~inside


@pytest.mark.parametrize("TF", [np.float32, np.float64])
@pytest.mark.parametrize("n", HESSIAN_GRIDS)
def test_hessian_operator(sipx, TF, n):
    N, nd = int(np.prod(n)), len(n)
    blocks = R.hessian_blocks(n)
    B = len(blocks)
    assert B == (3 if nd == 2 else 6)
    g1 = sipx.compgrid(tuple(1.0 for _ in n), n)
    H, AtA_diag, dense, TD_n, banded = sipx.get_TD_operator(g1, "Hessian", TF)
    assert H.kind == "custom" and H.shape == (B * N, N) and H.A.dtype == TF and not AtA_diag and not dense
    A = H.A.tocsr()
    assert np.array_equal(A.toarray().astype(np.float64), R.hessian_dense(n, (1.0,) * nd, TF)), "entry by entry"
    c = _coords(n)
    rng = np.random.default_rng(5)
    coef = {blk: int(k) for blk, k in zip(blocks, rng.integers(-4, 5, B))}
    x = np.zeros(N)
    for blk, k in coef.items():
        x = x + (k * c[blk[1]] ** 2 if blk[0] == "pure" else k * c[blk[1]] * c[blk[2]])
    lin = [int(k) for k in rng.integers(-5, 6, nd + 1)]
    affine = lin[0] + sum(k * c[a] for a, k in enumerate(lin[1:]))
    x = (x + affine).astype(TF)
    affine = affine.astype(TF)
    assert np.array_equal(x.astype(np.int64), x) and np.abs(x).max() < 2 ** 20
    eps = float(np.finfo(TF).eps)
    r2 = TF(np.sqrt(TF(2)))
    for q, blk in enumerate(blocks):
        rows = A[q * N:(q + 1) * N]
        inside, border = _block_rows(n, blk)
        assert np.all(np.diff(rows.indptr)[border] == 0), ("every border row is empty", blk)
        assert np.all(np.diff(rows.indptr)[inside] == (3 if blk[0] == "pure" else 4)), blk
        if blk[0] == "pure":
            assert np.array_equal((rows @ x)[inside], np.full(inside.sum(), 2 * coef[blk], TF)), blk
            assert np.all(rows @ affine == 0), blk
        else:
            w = rows.data[0]
            assert w == r2 and np.all(np.abs(rows.data) == w)
            unit = sp.csr_matrix((rows.data / w, rows.indices, rows.indptr), shape=rows.shape)
            assert np.array_equal(np.abs(unit.data), np.ones(unit.nnz, TF))
            assert np.array_equal((unit @ x)[inside], np.full(inside.sum(), coef[blk], TF)), blk       # the stencil, exactly
            assert np.all(unit @ affine == 0), blk
            # sqrt(2) c to 1 ulp: w is the correctly rounded sqrt(2), one more rounding for the product with the integer c
            want = np.sqrt(np.float64(2)) * coef[blk]
            assert abs(float(TF(w * TF(coef[blk]))) - want) <= eps * abs(want)
            # the plain product: four rounded terms
            assert np.all(np.abs((rows @ x)[inside].astype(np.float64) - want) <= 4 * eps * float(w) * float(np.abs(x).max()))
            assert np.all(np.abs(rows @ affine) <= 4 * eps * float(w) * float(np.abs(affine).max()))
    # non-unit spacing: the products of the fl(1 / h) factors D_xz uses
    h = (25.0, 6.0, 3.0)[:nd]
    Hh = sipx.get_TD_operator(sipx.compgrid(h, n), "Hessian", TF)[0]
    assert np.array_equal(Hh.A.toarray().astype(np.float64), R.hessian_dense(n, h, TF))
    ih = [TF(1) / TF(k) for k in h]
    Ah = Hh.A.tocsr()
    for q, blk in enumerate(blocks):
        rows = Ah[q * N:(q + 1) * N]
        if blk[0] == "pure":
            w = TF(ih[blk[1]] * ih[blk[1]])
            assert set(np.unique(rows.data)) == {w, TF(-2) * w}
        else:
            w = TF(r2 * TF(ih[blk[1]] * ih[blk[2]]))
            assert set(np.unique(rows.data)) == {w, -w}
    if nd == 2:      # the mixed block is sqrt(2) times the front end's own D_xz, zero-padded to the grid
        Dxz = sipx.get_TD_operator(sipx.compgrid(h, n), "D_xz", TF)[0].A.toarray()
        mixed = Ah[2 * N:].toarray().reshape(n[1], n[0], N)[:n[1] - 1, :n[0] - 1].reshape(-1, N)
        assert np.array_equal(mixed, (Dxz * r2).astype(TF))


def test_hessian_needs_three_points_per_dimension(sipx):
    for n in ((2, 5), (5, 2), (4, 2, 5), (2, 2)):
        with pytest.raises(sipx.SipxError, match="at least 3 grid points along every dimension"):
            sipx.get_TD_operator(sipx.compgrid(tuple(1.0 for _ in n), n), "Hessian", np.float32)
        with pytest.raises(sipx.SipxError, match="at least 3 grid points along every dimension"):
            sipx.setup_constraints([sipx.set_definitions("l21", "Hessian", 0.0, 1.0, ("matrix", ""))],
                                   sipx.compgrid(tuple(1.0 for _ in n), n), np.float32)


# ---- the front end -------------------------------------------------------------------------------------------------------------------------
def test_setup_constraints_takes_the_sets(sipx):
    TF = np.float32
    assert sipx.host.PROJ["l21_stacked"] == 23 and callable(sipx.l21_stacked_norm)
    assert "sipx_l21_stacked_norm" in sipx.EXPORTED_SYMBOLS and "sipx_l21_stacked_norm_dev" in sipx.EXPORTED_SYMBOLS
    for n, B in (((12, 9), 3), ((8, 6, 5), 6)):
        g = sipx.compgrid(tuple(1.0 for _ in n), n)
        N = int(np.prod(n))
        mode = ("matrix", "") if len(n) == 2 else ("tensor", "")
        c = [sipx.set_definitions("bounds", "identity", 1.0, 2.0, mode), sipx.set_definitions("l21", "Hessian", 0.0, 3.5, mode)]
        P, A, prop = sipx.setup_constraints(c, g, TF)
        assert prop.tag[1] == ("l21", "Hessian", mode[0], "") and prop.ncvx == [False, False]
        assert A[1].kind == "custom" and A[1].shape == (B * N, N)
        assert (P[1].kind, P[1].blocks, P[1].rows, P[1].mode, P[1].pmax, P[1].transform) == ("l21_stacked", B, B * N, 0, 3.5, 0)
        d = P[1].desc(A[1].kind, prop.ncvx[1])
        assert (d.op, d.proj, d.pmax, d.mode, d.transform, d.ncvx, d.blocks, d.reserved) == (5, 23, 3.5, 0, 0, 0, B, 0)
        assert d.lb is None and d.ub is None
        P[1].check_rows(A[1])
        assert P[1].data_len(A[1]) is None
        # more diagonals than one set hands over: the operator enters Q matrix-free
        opt = sipx.PARSDMM_options(FL=TF)
        A2, AtA, l, y = sipx.PARSDMM_precompute_distribute(A, prop, g, opt)
        assert A[1].ata_diagonals() == (13 if len(n) == 2 else 25) and AtA[1] is None and len(prop.AtA_offsets[1]) == 0
        assert [len(v) for v in y] == [N, B * N, N]
    # the caller-supplied form: a two-block operator, its A'A banded
    n = (12, 9)
    g = sipx.compgrid((1.0, 1.0), n)
    S = sp.vstack([sp.identity(108, format="csc"), 2 * sp.identity(108, format="csc")], format="csc")
    c = [sipx.set_definitions("l21_stacked", "anything", 0.0, 2.0, ("matrix", ""), custom_TD_OP=(S, False), blocks=2)]
    P, A, prop = sipx.setup_constraints(c, g, TF)
    assert (P[0].kind, P[0].blocks, P[0].rows) == ("l21_stacked", 2, 216) and A[0].kind == "custom"
    A2, AtA, l, y = sipx.PARSDMM_precompute_distribute(A, prop, g, sipx.PARSDMM_options(FL=TF))
    assert AtA[0] is not None and list(prop.AtA_offsets[0]) == [0]
    # ("l21_stacked", "Hessian") without an operator of the caller's is the named set
    P = sipx.setup_constraints([sipx.set_definitions("l21_stacked", "Hessian", 0.0, 2.0, ("matrix", ""))], g, TF)[0]
    assert (P[0].kind, P[0].blocks) == ("l21_stacked", 3)


def test_host_refusals(sipx):
    TF = np.float32
    n = (12, 9)
    g = sipx.compgrid((1.0, 1.0), n)
    H = sipx.host
    S = sp.identity(108, format="csc")

    def stacked(M=216, blocks=2, mode=("matrix", ""), mx=1.0, op="custom", custom=True, **kw):
        A = sp.vstack([S] * (M // 108) + ([S[:M % 108]] if M % 108 else []), format="csc")
        return sipx.set_definitions("l21_stacked", op, 0.0, mx, mode, custom_TD_OP=(A, False) if custom else ((), False), blocks=blocks, **kw)

    def refused(c, text, grid=g):
        with pytest.raises(sipx.SipxError) as e:
            sipx.setup_constraints([c], grid, TF)
        assert text in str(e.value), str(e.value)
    refused(stacked(M=216 + 54, blocks=4), "M = 270 rows, not a multiple of blocks = 4")
    refused(stacked(blocks=0), "blocks = 0, the number of equal-sized blocks of the operator must be 1 .. 8")
    refused(stacked(M=108 * 9, blocks=9), "blocks = 9, the number of equal-sized blocks of the operator must be 1 .. 8")
    refused(stacked(blocks=None), "needs blocks")
    for op in ("TV", "identity", "D_x"):
        refused(stacked(op=op, custom=False), H.L21S_NEEDS_CSC)
    for mode in (("fiber", "x"), ("fiber", "z"), ("slice", "x")):
        refused(stacked(mode=mode), H.L21S_WHOLE_ONLY)
        refused(sipx.set_definitions("l21", "Hessian", 0.0, 1.0, mode), H.L21S_WHOLE_ONLY)
    for mx in (0.0, -1.0, float("nan")):
        refused(stacked(mx=mx), "Radius of L1 ball is negative")
        refused(sipx.set_definitions("l21", "Hessian", 0.0, mx, ("matrix", "")), "Radius of L1 ball is negative")
    refused(sipx.set_definitions("l21", "Hessian", 0.0, 1.0, ("matrix", ""), weights=np.ones(108, TF)), H.L21S_NO_VECTORS)
    refused(sipx.set_definitions("l21", "Hessian", 0.0, 1.0, ("matrix", ""), blocks=2), "has 3 blocks, blocks = 2 was given")
    refused(stacked(op="DFT"), H.L21S_NO_TRANSFORM)
    # a descriptor never reaches an operator it was not made for
    P = sipx.Projector(sipx.set_definitions("l21", "Hessian", 0.0, 1.0, ("matrix", "")), g, TF)
    for kind in ("identity", "TV"):
        with pytest.raises(sipx.SipxError, match="the operator must be SIPX_OP_CSC"):
            P.check_rows(sipx.TDOperator(kind, g, TF))
    with pytest.raises(sipx.SipxError, match="M = 108 rows, not a multiple of blocks = 3") if 108 % 3 else pytest.raises(sipx.SipxError, match="M = 109 rows"):
        P.check_rows(sipx.host.CustomOperator(sp.vstack([S, S[:1]], format="csc"), g, TF))
    with pytest.raises(sipx.SipxError, match="the operator's range: 324 entries, 108 given"):
        P(np.zeros(108, TF))
    with pytest.raises(sipx.SipxError, match="the operator must be SIPX_OP_CSC"):
        sipx.l21_stacked_norm(np.zeros(108, TF), g, "TV")
    # a Minkowski component: custom operators have none (the operator's own refusal), and a component on the descriptor is refused
    class WithComponent(sipx.host.CustomOperator):
        component = 1
    with pytest.raises(sipx.SipxError, match="takes no Minkowski component"):
        P.check_rows(WithComponent(sipx.get_TD_operator(g, "Hessian", TF)[0].A, g, TF))


def test_multilevel_refuses_the_sets(sipx):
    TF = np.float32
    n = (32, 24)
    g = sipx.compgrid((1.0, 1.0), n)
    m = np.ones(32 * 24, TF)
    opt = sipx.PARSDMM_options(FL=TF)
    S = sp.vstack([sp.identity(768, format="csc")] * 2, format="csc")
    for c in (sipx.set_definitions("l21", "Hessian", 0.0, 1.0, ("matrix", "")),
              sipx.set_definitions("l21_stacked", "custom", 0.0, 1.0, ("matrix", ""), custom_TD_OP=(S, False), blocks=2)):
        with pytest.raises(sipx.SipxError, match="not built for PARSDMM_multi_level"):
            sipx.setup_multi_level_PARSDMM(m, 2, 2, g, [c], opt)
        with pytest.raises(sipx.SipxError, match="not built for PARSDMM_multi_level"):
            sipx.constraint2coarse([c], g, 2)
    P, A, prop = sipx.setup_constraints([sipx.set_definitions("l21", "Hessian", 0.0, 1.0, ("matrix", ""))], g, TF)
    A, AtA, l, y = sipx.PARSDMM_precompute_distribute(A, prop, g, opt)
    with pytest.raises(sipx.SipxError, match="not built for PARSDMM_multi_level"):
        sipx.PARSDMM_multi_level(m, [A], [AtA], [P], [prop], [g], opt)


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


def test_engine_takes_the_set(sipx, ask):
    for tf in "fd":
        for grid, N in ((G2, 108), (G3, 240)):
            for B in BLOCKS:
                a, b = ask([f"set tf={tf} {grid} op=5 proj=23 pmax=2.5 rows={B * N} blocks={B}",
                            f"set tf={tf} {grid} op=5 proj=23 pmax=2.5 rows={B * N} blocks={B} ata=5"])
                for r, mfree in ((a, "1"), (b, "0")):      # ata_R = NULL: the matrix-free term of Q; with bands: banded
                    assert isinstance(r, dict), r
                    assert (r["ext_kind"], r["prox"], r["custom"], r["mfree"]) == ("25", "8", "1", mfree)
                    assert (r["Mtrue"], r["Mpad"], r["spec.nblk"], r["spec.bstride"], r["spec.N"]) == (str(B * N), str(B * N), str(B), str(N), str(B * N))
                    assert (r["spec.mode"], r["needs_ext"], r["ncvx"], r["two_pass"]) == ("0", "1", "0", "0")
    # the entries set_data would take are those of every materialised set without vectors, ("l21", "TV") among them: the front end
    # holds none for either (Projector.data_len is None)
    tv, st = ask([f"set {G2} op=4 proj=14 pmax=1", f"set {G2} op=5 proj=23 pmax=1 rows=324 blocks=3"])
    assert tv["data_len"] == tv["Mtrue"] and st["data_len"] == st["Mtrue"] == "324"
    P = sipx.Projector(sipx.set_definitions("l21", "Hessian", 0.0, 1.0, ("matrix", "")), sipx.compgrid((1.0, 1.0), (12, 9)), np.float32)
    assert P.data_len(sipx.get_TD_operator(sipx.compgrid((1.0, 1.0), (12, 9)), "Hessian", np.float32)[0]) is None and P.rows == 324


def test_engine_refusals(sipx, ask):
    H = sipx.host
    base = f"set {G2} op=5 proj=23 pmax=1"
    cases = [
        (H.l21s_bad_rows(325, 3), base + " rows=325 blocks=3"),
        (H.l21s_bad_blocks(0), base + " rows=324 blocks=0"),
        (H.l21s_bad_blocks(9), base + " rows=324 blocks=9"),
        (H.l21s_bad_blocks(-1), base + " rows=324 blocks=-1"),
        (H.L21S_NEEDS_CSC, f"set {G2} op=4 proj=23 pmax=1 blocks=2"),
        (H.L21S_NEEDS_CSC, f"set {G2} op=0 proj=23 pmax=1 blocks=1"),
        (H.L21S_NEEDS_CSC, f"set {G3} op=6 proj=23 pmax=1 blocks=2"),
        (H.L21S_WHOLE_ONLY, base + " rows=324 blocks=3 mode=1 dir=0"),
        (H.L21S_WHOLE_ONLY, base + " rows=324 blocks=3 mode=1 dir=1"),
        (H.L21S_WHOLE_ONLY, base + " rows=324 blocks=3 mode=2 dir=0"),
        (H.L21S_NO_TRANSFORM, base + " rows=324 blocks=3 tr=1"),
        (H.L21S_NO_TRANSFORM, base + " rows=324 blocks=3 tr=2"),
        (H.L21S_NO_MINKOWSKI, base + " rows=324 blocks=3 comp=1"),
        (H.L21S_NO_MINKOWSKI, base + " rows=324 blocks=3 comp=3"),
        (H.L21S_NO_VECTORS, base + " rows=324 blocks=3 lb=108 reserved=108"),
        (H.L21S_NO_VECTORS, base + " rows=324 blocks=3 ub=108"),
        (H.L21S_SHARDED, base + " rows=324 blocks=3 single=0"),
        ("Radius of L1 ball is negative", f"set {G2} op=5 proj=23 pmax=0 rows=324 blocks=3"),
        ("Radius of L1 ball is negative", f"set {G2} op=5 proj=23 pmax=-2 rows=324 blocks=3"),
        ("Radius of L1 ball is negative", f"set {G2} op=5 proj=23 pmax=nan rows=324 blocks=3"),
    ]
    got = ask(line for _, line in cases)
    for (want, line), g in zip(cases, got):
        assert g == want, (line, g)
    # the other materialised projectors still refuse a custom operator
    for proj in (8, 9, 14, 16, 21):
        r = ask([f"set {G2} op=5 proj={proj} pmax=1 rows=324 mode={1 if proj == 16 else 0}"])[0]
        assert isinstance(r, str), (proj, r)


def test_old_style_descriptor_configures_every_existing_kind(ask):
    """A descriptor filled through the struct as it ended before `blocks` (zero behind it): every kind that takes a plain descriptor on a
    built-in operator is configured as with the new struct, and the new kind reads blocks = 0 there and refuses it."""
    takes = {0: "", 2: "pmax=1", 3: "pmax=1", 4: "pmin=1 pmax=2", 5: "pmax=3", 6: "pmax=1", 7: "pmax=1", 8: "pmax=2", 9: "pmax=1", 13: "pmax=4"}
    lines = []
    for proj, kw in takes.items():
        for old in (0, 1):
            lines.append(f"set {G2} op=0 proj={proj} {kw} old={old}")
    for op, proj, kw, grid in ((4, 14, "pmax=1", G2), (6, 14, "pmax=1", G3), (6, 15, "pmax=1", G3), (6, 17, "pmax=1", G3), (3, 16, "pmax=1 mode=1 dir=0", G2),
                               (3, 19, "pmin=0 pmax=1 mode=1 dir=0", G2), (3, 20, "pmax=2 mode=1 dir=0", G2), (4, 21, "pmax=5", G2), (6, 22, "pmax=5", G3),
                               (5, 2, "pmax=1 rows=50", G2), (5, 0, "rows=50", G2)):
        for old in (0, 1):
            lines.append(f"set {grid} op={op} proj={proj} {kw} old={old}")
    out = ask(lines)
    for k in range(0, len(out), 2):
        assert isinstance(out[k], dict) and out[k] == out[k + 1], (lines[k], out[k], out[k + 1])
    assert "blocks = 0" in ask([f"set {G2} op=5 proj=23 pmax=1 rows=324 old=1"])[0]


def test_c_abi_header_appends_the_field():
    src = open(os.path.join(ROOT, "include", "sipx.h")).read()
    body = src[src.index("typedef struct {\n  int32_t op;"):src.index("} sipx_set_desc;")]
    fields = [ln.split(";")[0].split()[-1] for ln in body.splitlines() if ln.startswith("  ") and ";" in ln and not ln.lstrip().startswith(("/*", "*"))
              and ln.lstrip().split()[0] in ("int32_t", "int64_t", "double", "const")]
    assert fields[-3:] == ["pad_", "blocks", "pad2_"], fields[-4:]
    assert "SIPX_PROJ_L21_STACKED = 23" in src
