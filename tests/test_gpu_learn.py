"""Constraint learning on the device (sipx.constraint_learning_by_obseration, csrc/learn.hip) against the numpy restatement
(tests/learn_ref.py), with the numerical contract of DESIGN.md "Constraint learning": exact TF values for the histograms and
slope extrema, one TF ulp for float64 sums (Float32; a summation-order bound for Float64), the transform and SVD tolerances,
and exact counts (+-1 only where the restatement's cumulative sum sits within the threshold's margin).  Then bit-reproducibility (calls, chunkings, layouts, key subsets), the TV
rows' bits, and the learned values fed back into the projectors and a PARSDMM solve."""
import numpy as np
import pytest

from oracle import parsdmm_oracle as O
from tests import learn_ref as R

pytestmark = pytest.mark.gpu

EXACT = ("hist_min", "hist_max", "hist_TV_min", "hist_TV_max", "D_x_min", "D_x_max", "D_z_min", "D_z_max")
SUMS = ("TV", "Dx_l1", "Dz_l1", "D_l2", "TV_annulus", "annulus")
COUNTS = ("rank_095", "DFT_card_095", "TV_card_095")
H = (25.0, 6.0)


def images(nt, n, TF, seed=0):
    rng = np.random.default_rng(1000 + 7 * seed + n[0] + 31 * n[1])
    z = np.linspace(0, 1, n[1])[None, :]
    x = np.linspace(0, 1, n[0])[:, None]
    out = [1500 + 2000 * z + 300 * np.sin(3 * x + k) + 150 * rng.standard_normal(n) for k in range(nt)]
    return np.stack(out).astype(TF)


def check(got, ref, TF, margins):
    f32 = TF == np.float32
    for k in R.KEYS:
        g, r = got[k], ref[k]
        assert g.dtype == r.dtype and g.shape == r.shape, k
        if k in EXACT:
            assert np.array_equal(g, r), k
        elif k in SUMS:
            # Float32: one rounding of a float64 sum.  Float64: TF is the accumulator, so two summation orders (a fixed tree here,
            # numpy's pairwise sum there) of N positive terms differ by up to ~log2(N) ulp
            assert np.all(np.abs(g.astype(np.float64) - r) <= (1 if f32 else 32) * np.spacing(np.abs(r))), k
        elif k in ("DFT_l1", "wavelet_l1"):
            assert np.allclose(g, r, rtol=2e-6 if f32 else 1e-12, atol=0), (k, g, r)
        elif k.startswith("DCT_"):
            scale = max(np.abs(ref["DCT" + k[3:5] + "_UB"]).max(), np.abs(ref["DCT" + k[3:5] + "_LB"]).max())
            assert np.all(np.abs(g.astype(np.float64) - r) <= (2e-6 if f32 else 1e-12) * scale), k
        elif k.startswith("nuclear"):
            assert np.allclose(g, r, rtol=1e-5 if f32 else 1e-11, atol=0), (k, g, r)
        else:
            d = np.abs(g.astype(np.int64) - r)
            near = margins[k] < (1e-6 if f32 else 1e-12)
            assert np.all((d == 0) | ((d == 1) & near)), (k, g, r, margins[k])


@pytest.mark.parametrize("TF", [np.float32, np.float64])
@pytest.mark.parametrize("n", [(16, 16), (17, 9), (64, 48), (128, 128), (256, 256)])
@pytest.mark.parametrize("nt", [1, 5, 33])
def test_parity_every_key(sipx, TF, n, nt):
    m = images(nt, n, TF)
    mg = {}
    ref = R.learn(m, H, mg)
    got = sipx.constraint_learning_by_obseration(sipx.compgrid(H, n), m)
    assert set(got) == set(R.KEYS)
    check(got, ref, TF, mg)


WAVELET_GRID = (200, 200)        # square (wavelet_l1 is 0 otherwise, as in the reference), L = 3, off the powers of two


@pytest.mark.parametrize("TF", [np.float32, np.float64])
def test_wavelet_l1_off_a_power_of_two(sipx, TF):
    """200 x 200 (L = 3): two levels of axis passes whose half-lengths 100 and 50 are no multiple of the strided run length, the
    second through the compact boxes, then the one-workgroup kernel on 50 x 50 -- per image, against the float64 restatement of
    the transform within check()'s bound for this key.  On 200 x 120 the key is 0: the reference observes it on square grids
    only (constraint_learning_by_observation.jl:67,113), and so does the learner."""
    from tests import dwt_ref
    n = WAVELET_GRID
    m = images(3, n, TF)
    got = sipx.constraint_learning_by_obseration(sipx.compgrid(H, n), m, keys=["wavelet_l1"])
    assert set(got) == {"wavelet_l1"} and got["wavelet_l1"].shape == (3,) and got["wavelet_l1"].dtype == TF
    ref = np.array([np.abs(dwt_ref.dwt_vec(img.reshape(-1, order="F"), n)).sum() for img in m])
    assert np.all(ref > 0)
    assert np.allclose(got["wavelet_l1"], ref, rtol=2e-6 if TF == np.float32 else 1e-12, atol=0), (got["wavelet_l1"], ref)
    n = (200, 120)
    got = sipx.constraint_learning_by_obseration(sipx.compgrid(H, n), images(3, n, TF), keys=["wavelet_l1"])
    assert np.array_equal(got["wavelet_l1"], np.zeros(3, TF))


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("TF", [np.float32, np.float64])
def test_determinism_chunking_and_layout(sipx, TF):
    n = (48, 48)
    m = images(7, n, TF, seed=1)
    g = sipx.compgrid(H, n)
    full = sipx.constraint_learning_by_obseration(g, m)
    _same(full, sipx.constraint_learning_by_obseration(g, m))
    for b in (1, 3, 7):
        _same(full, sipx.constraint_learning_by_obseration(g, m, max_batch=b))
    jl = np.asfortranarray(m)                    # Julia's m_train[i, :, :]: the image index fastest
    assert jl.strides[0] == jl.itemsize
    _same(full, sipx.constraint_learning_by_obseration(g, jl))
    _same(full, sipx.constraint_learning_by_obseration(g, jl, max_batch=3))
    view = np.ascontiguousarray(np.transpose(m, (1, 2, 0))).transpose(2, 0, 1)    # neither C nor F order
    _same(full, sipx.constraint_learning_by_obseration(g, view))
    one = sipx.constraint_learning_by_obseration(g, m[2])       # a 2-D m_train is one image
    for k in ("TV", "nuclear_norm", "DFT_card_095", "wavelet_l1"):
        assert one[k][0] == full[k][2], k


@pytest.mark.parametrize("TF", [np.float32, np.float64])
def test_key_subsets(sipx, TF):
    n = (40, 24)
    m = images(6, n, TF, seed=2)
    g = sipx.compgrid(H, n)
    full = sipx.constraint_learning_by_obseration(g, m)
    for keys in (["TV_card_095"], ["hist_min", "nuclear_Dz"], ["DFT_card_095", "wavelet_l1"], ["DCT_y_UB"], ["rank_095", "D_l2"],
                 ["hist_TV_max", "DCT_x_LB"]):
        part = sipx.constraint_learning_by_obseration(g, m, keys=keys, max_batch=4)
        assert set(part) == set(keys)
        for k in keys:
            assert np.array_equal(part[k], full[k]), k


@pytest.mark.parametrize("TF", [np.float32, np.float64])
def test_tv_rows_bit_identical(sipx, TF):
    n = (37, 29)
    img = images(1, n, TF, seed=3)[0] - TF(2500)
    g = sipx.compgrid(H, n)
    o = sipx.constraint_learning_by_obseration(g, img, keys=["hist_TV_max", "hist_TV_min"])
    tv = sipx.TDOperator("TV", g, TF) @ img.reshape(-1, order="F")
    assert np.array_equal(o["hist_TV_max"], np.maximum(TF(0), np.sort(tv)))
    assert np.array_equal(o["hist_TV_min"], np.minimum(1e8, np.sort(tv).astype(np.float64)))


@pytest.mark.parametrize("TF", [np.float32, np.float64])
def test_learned_values_against_the_projectors(sipx, TF):
    n = (64, 64)
    m = images(4, n, TF, seed=4)
    g = sipx.compgrid(H, n)
    o = sipx.constraint_learning_by_obseration(g, m)
    i = 2
    x = m[i].reshape(-1, order="F")
    P = sipx.setup_constraints([sipx.set_definitions("histogram", "identity", o["hist_min"].astype(TF), o["hist_max"],
                                                     ("matrix", ""))], g, TF)[0][0]
    assert np.array_equal(P(x.copy()), x)
    for kind, op, key in (("l1", "TV", "TV"), ("l1", "DFT", "DFT_l1"), ("l1", "wavelet", "wavelet_l1"),
                          ("nuclear", "identity", "nuclear_norm")):
        r = float(o[key][i])
        for fac, inside in ((1 + 1e-5, True), (0.99, False)):
            Pj, A, _ = sipx.setup_constraints([sipx.set_definitions(kind, op, 0.0, fac * r, ("matrix", ""))], g, TF)
            v = A[0] @ x
            w = Pj[0](v.copy())
            if inside:
                assert np.allclose(w, v, rtol=0, atol=1e-5 * np.abs(v).max()), (key, fac)
            else:
                assert np.linalg.norm(w.astype(np.float64) - v) > 1e-4 * np.linalg.norm(v), (key, fac)


def test_full_size_512(sipx):
    TF, n = np.float32, (512, 512)
    m = images(64, n, TF, seed=5)
    mg = {}
    ref = R.learn(m, H, mg)
    check(sipx.constraint_learning_by_obseration(sipx.compgrid(H, n), m), ref, TF, mg)


def _indonesia_list(mod, o, TF, n):
    # examples/Indonesia_desaturation/image_desaturation_by_constraint_learning.jl: bounds, relaxed histogram, and quantiles of
    # the nuclear norm, TV, D_l2 and DFT_l1 of the training images
    q = lambda k, p=0.5: float(np.quantile(o[k].astype(np.float64), p))
    return [mod.set_definitions("bounds", "identity", float(o["hist_min"].min()), float(o["hist_max"].max()), ("matrix", "")),
            mod.set_definitions("histogram", "identity", o["hist_min"].astype(TF), o["hist_max"].astype(TF), ("matrix", "")),
            mod.set_definitions("nuclear", "identity", 0.0, q("nuclear_norm"), ("matrix", "")),
            mod.set_definitions("l1", "TV", 0.0, q("TV"), ("matrix", "")),
            mod.set_definitions("l2", "TV", 0.0, q("D_l2"), ("matrix", "")),
            mod.set_definitions("l1", "DFT", 0.0, q("DFT_l1"), ("matrix", ""))]


def test_end_to_end_indonesia_list(sipx):
    TF, n = np.float32, (48, 40)
    train = images(12, n, TF, seed=6)
    g = sipx.compgrid(H, n)
    o = sipx.constraint_learning_by_obseration(g, train)
    obs = images(1, n, TF, seed=7)[0]
    obs = np.minimum(obs, np.quantile(obs, 0.8)).astype(TF).reshape(-1, order="F")      # a saturated observation

    def solve(mod):
        gg = mod.compgrid(H, n)
        opt = mod.PARSDMM_options(FL=TF, maxit=40)
        P, A, prop = mod.setup_constraints(_indonesia_list(mod, o, TF, n), gg, TF)
        A, AtA, l, y = mod.PARSDMM_precompute_distribute(A, prop, gg, opt)
        return mod.PARSDMM(obs.copy(), AtA, A, prop, P, gg, opt)

    xs = solve(sipx)[0]
    xo = solve(O)[0]
    assert np.all(np.isfinite(xs))
    assert np.linalg.norm(xs.astype(np.float64) - xo) / np.linalg.norm(xo) < 5e-4
