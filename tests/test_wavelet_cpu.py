"""Wavelet-domain sets (TD_OP = "wavelet", sipx.h SIPX_TRANSFORM_WAVELET) without a device: the numpy restatement of the
transform against PyWavelets' output (tests/golden/dwt_db4_periodization.npz, made by tests/golden/make_dwt_golden.py), and
the host-side setup of sets behind it."""
import os

import numpy as np
import pytest

from tests import dwt_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dwt_db4_periodization.npz")
SHAPES = [(16, 8), (32, 24), (128, 128), (8, 8, 4), (16, 16, 8), (9, 7)]


@pytest.mark.parametrize("n", SHAPES)
def test_restatement_matches_pywavelets(n):
    z = np.load(GOLDEN)
    key = "x".join(str(v) for v in n)
    x, c = z["x_" + key], z["c_" + key]
    assert x.shape == n and c.shape == n
    assert R.levels(n) == (0 if n == (9, 7) else {(16, 8): 3, (32, 24): 3, (128, 128): 7, (8, 8, 4): 2, (16, 16, 8): 3}[n])
    assert np.abs(R.dwt(x) - c).max() <= 1e-12 * max(1.0, np.abs(c).max())
    assert np.abs(R.dwt(c, inverse=True) - x).max() <= 1e-12 * max(1.0, np.abs(x).max())


def test_restatement_is_orthogonal():
    rng = np.random.default_rng(3)
    for n in ((8, 4), (4, 4, 2), (2, 2)):
        N = int(np.prod(n))
        W = np.stack([R.dwt_vec(e, n) for e in np.eye(N)], axis=1)
        assert np.allclose(W.T @ W, np.eye(N), atol=1e-13)
        v = rng.standard_normal(N)
        assert np.allclose(R.dwt_vec(v, n, inverse=True), W.T @ v, atol=1e-13)


def test_wavelet_setup_without_device(sipx):
    TF = np.float32
    g = sipx.compgrid((25.0, 6.0), (32, 24))
    A, AtA_diag, dense, TD_n, banded = sipx.get_TD_operator(g, "wavelet", TF)
    assert A.kind == "identity" and AtA_diag and dense and TD_n == (32, 24) and not banded
    c = [sipx.set_definitions("bounds", "identity", 1600.0, 3900.0, ("matrix", "")),
         sipx.set_definitions("l1", "wavelet", 0.0, 100.0, ("matrix", "")),
         sipx.set_definitions("cardinality", "wavelet", 0, 50, ("matrix", "")),
         sipx.set_definitions("bounds", "wavelet", 1.0, 5.0, ("matrix", "")),
         sipx.set_definitions("bounds", "wavelet", -1.0, 5.0, ("matrix", "")),
         sipx.set_definitions("l2", "wavelet", 0.0, 10.0, ("matrix", "")),
         sipx.set_definitions("annulus", "wavelet", 1.0, 10.0, ("matrix", ""))]
    P, A, prop = sipx.setup_constraints(c, g, TF)
    assert [p.transform for p in P] == [0, 2, 2, 2, 2, 0, 0]
    assert [p.kind for p in P] == ["bounds", "l1", "cardinality", "bounds", "bounds", "l2", "annulus"]
    assert prop.ncvx == [False, False, True, True, False, False, False]      # setup_constraints.jl:89-97
    assert all(a.kind == "identity" for a in A)
    d = P[1].desc("identity", False)
    assert d.transform == 2 and d.proj == sipx.host.PROJ["l1"] and d.pmax == 100.0 and d.op == 0
    assert sipx.host.TRANSFORMS["wavelet"] == 2
    # 3-D: L over all three dimensions
    g3 = sipx.compgrid((1.0, 1.0, 1.0), (16, 16, 8))
    P3, _, _ = sipx.setup_constraints([sipx.set_definitions("l1", "wavelet", 0.0, 1.0, ("tensor", ""))], g3, TF)
    assert P3[0].transform == 2
    # L = 0 grids take the identity
    P0, _, _ = sipx.setup_constraints([sipx.set_definitions("l1", "wavelet", 0.0, 1.0, ("matrix", ""))], sipx.compgrid((1.0, 1.0), (9, 7)), TF)
    assert P0[0].transform == 2


def test_wavelet_refusals_without_device(sipx):
    TF = np.float64
    g = sipx.compgrid((1.0, 1.0), (8, 12))           # L = 3 (min 8), 12 not divisible by 8
    with pytest.raises(sipx.SipxError, match="8 x 12"):
        sipx.setup_constraints([sipx.set_definitions("l1", "wavelet", 0.0, 1.0, ("matrix", ""))], g, TF)
    g = sipx.compgrid((1.0, 1.0), (32, 24))
    for st, lo, hi in (("nuclear", 0.0, 1.0), ("histogram", np.zeros(768), np.ones(768)), ("rank", 0, 3)):
        with pytest.raises(sipx.SipxError, match="wavelet"):
            sipx.setup_constraints([sipx.set_definitions(st, "wavelet", lo, hi, ("matrix", ""))], g, TF)
    with pytest.raises(sipx.SipxError, match="wavelet"):          # per-element bounds: the layout is not pinned
        sipx.setup_constraints([sipx.set_definitions("bounds", "wavelet", np.zeros(768), np.ones(768), ("matrix", ""))], g, TF)
    with pytest.raises(sipx.SipxError, match="whole array"):
        sipx.setup_constraints([sipx.set_definitions("cardinality", "wavelet", 0, 5, ("fiber", "x"))], g, TF)
    with pytest.raises(sipx.SipxError, match="8 x 12"):
        sipx.dwt(np.zeros(96), (8, 12))
    with pytest.raises(sipx.SipxError, match="unknown transform domain operator"):
        sipx.setup_constraints([sipx.set_definitions("l1", "curvelet", 0.0, 1.0, ("matrix", ""))], g, TF)
