"""Cardinality behind the DFT (TD_OP = "DFT", sipx.h SIPX_PROJ_CARD_DFT) without a device: the half-weight form the engine hands
the real inverse transform against the literal contract (tests/card_dft_ref.py), and the host-side setup of the set."""
import numpy as np
import pytest

from tests import card_dft_ref as R

GRIDS = [(6, 5), (3, 8), (2, 2, 4), (15, 12, 9), (16, 12, 8)]


def _ks(x, n):
    kc = R.pair_cutting_k(x, n, start=2)
    return [1, kc, kc + 1, int(np.prod(n)) - 1]


def _half_weight_form(x, n, k):
    """Re(F'(K .* Z)) as F'(w .* Z), w[e] = (keep[e] + keep[e*]) / 2: a Hermitian spectrum, so the inverse is real."""
    Z, keep = R.keep_mask(x, n, k)
    w = 0.5 * (keep.astype(np.float64) + keep[R.partner(n)])
    X = np.fft.ifftn((w * Z).reshape(n, order="F"), norm="ortho")
    return X, w


def _through_the_real_transform(x, n, k):
    """The engine's R2C route: only the planes k1 = 0 .. n1/2 of the spectrum exist, each stored bin is multiplied by w of its
    own natural index, the real inverse transform does the rest."""
    axes = tuple(range(len(n) - 1, -1, -1))                    # the real transform runs along the first (fastest) dimension
    Zh = np.fft.rfftn(np.asarray(x, np.float64).reshape(n, order="F"), axes=axes, norm="ortho")
    _, w = _half_weight_form(x, n, k)
    wh = w.reshape(n, order="F")[:n[0] // 2 + 1]
    return np.fft.irfftn(Zh * wh, s=tuple(n[a] for a in axes), axes=axes, norm="ortho").reshape(-1, order="F")


@pytest.mark.parametrize("n", GRIDS)
def test_half_weight_form_equals_the_literal_form(n):
    rng = np.random.default_rng(sum(n))
    N = int(np.prod(n))
    for x in (R.designed(n, 11, np.float64), rng.standard_normal(N)):
        ks = _ks(x, n)
        _, mag, order = R.spectrum(x, n)
        s = mag[order]
        assert s[ks[1] - 1] == s[ks[1]] and s[ks[2] - 1] != s[ks[2]]           # cuts a pair / does not
        for k in ks:
            want, _ = R.project(x, n, k)
            X, w = _half_weight_form(x, n, k)
            scale = np.abs(x).max()
            assert np.abs(X.imag).max() <= 1e-14 * scale, (n, k)
            assert np.abs(X.real.reshape(-1, order="F") - want).max() <= 1e-14 * scale, (n, k)
            assert set(np.unique(w)) <= {0.0, 0.5, 1.0} and w.sum() == k
            assert (0.5 in w) == (s[k - 1] == s[k])            # a half-weighted pair exactly when the cut separates one
            assert np.abs(_through_the_real_transform(x, n, k) - want).max() <= 1e-14 * scale, (n, k)


def test_helper_edges_and_margin():
    n = (6, 5)
    x = R.designed(n, 3, np.float64)
    p = R.partner(n)
    assert np.array_equal(p[p], np.arange(30)) and p[0] == 0 and p[3] == 3 and p[1] == 5 and p[6 + 1] == 6 * 4 + 5
    out, margin = R.project(x, n, 30)
    assert np.abs(out - x).max() <= 1e-14 and margin == np.inf
    out, margin = R.project(x, n, 0)
    assert not out.any() and margin == np.inf
    C = 30 // 2 + 1                                            # 2 self-conjugate bins on (6, 5): (30 - 2) / 2 + 2 classes
    for k in (1, 7, 8, 29):
        assert R.project(x, n, k)[1] >= 1 / (2 * C) - 1e-9
    for TF, (nn, bound) in ((np.float32, ((16, 12, 8), 6.4e-4)), (np.float64, ((30, 21), 1.5e-3))):
        v = R.designed(nn, 5, TF)
        assert v.dtype == TF and R.project(v, nn, int(np.prod(nn)) // 10)[1] >= bound


def test_card_dft_setup_without_device(sipx):
    for TF, n, h, mode in ((np.float32, (32, 24), (25.0, 6.0), ("matrix", "")), (np.float64, (16, 12, 8), (1.0, 1.0, 1.0), ("tensor", ""))):
        g = sipx.compgrid(h, n)
        c = [sipx.set_definitions("bounds", "identity", 1600.0, 3900.0, ("matrix", "")),
             sipx.set_definitions("cardinality", "DFT", 0, 77, mode)]
        P, A, prop = sipx.setup_constraints(c, g, TF)          # (SipxError before the set was built)
        assert P[1].kind == "card_dft" and P[1].pmax == 77.0 and P[1].pmin == 0.0 and P[1].transform == 0 and P[1].mode == 0
        assert prop.ncvx == [False, True] and A[1].kind == "identity" and prop.AtA_diag[1] and prop.TD_n[1] == n
        assert prop.tag[1] == ("cardinality", "DFT", mode[0], "")
        d = P[1].desc("identity", True)
        assert d.proj == sipx.host.PROJ["card_dft"] == 13 and d.pmax == 77.0 and d.op == 0 and d.mode == 0 and d.ncvx == 1
        P[1].check_rows(A[1])


def test_card_dft_refusals_without_device(sipx):
    import scipy.sparse as sp
    TF = np.float32
    g = sipx.compgrid((1.0, 1.0, 1.0), (8, 6, 4))
    for mode in (("fiber", "x"), ("slice", "z")):
        with pytest.raises(sipx.SipxError, match="whole array"):
            sipx.setup_constraints([sipx.set_definitions("cardinality", "DFT", 0, 5, mode)], g, TF)
    with pytest.raises(sipx.SipxError, match="InexactError"):
        sipx.setup_constraints([sipx.set_definitions("cardinality", "DFT", 0, 2.5, ("tensor", ""))], g, TF)
    with pytest.raises(sipx.SipxError, match="negative"):
        sipx.setup_constraints([sipx.set_definitions("cardinality", "DFT", 0, -3, ("tensor", ""))], g, TF)
    # a custom sparse operator takes the whole-array projectors of its own range only
    c = sipx.set_definitions("cardinality", "DFT", 0, 5, ("tensor", ""), (sp.identity(8 * 6 * 4, dtype=TF, format="csc"), False))
    P, A, _ = sipx.setup_constraints([c], g, TF)
    assert A[0].kind == "custom"
    with pytest.raises(sipx.SipxError, match="custom sparse operators"):
        P[0].check_rows(A[0])
    # the other set types behind the DFT stay refused, and the message names what is built
    with pytest.raises(sipx.SipxError, match="cardinality"):
        sipx.setup_constraints([sipx.set_definitions("histogram", "DFT", np.zeros(192, TF), np.ones(192, TF), ("tensor", ""))], g, TF)


def test_constraint2coarse_keeps_k(sipx):
    from sipx import multilevel
    g = sipx.compgrid((1.0, 1.0), (16, 12))
    c = [sipx.set_definitions("cardinality", "DFT", 0, 40, ("matrix", "")), sipx.set_definitions("l1", "DFT", 0.0, 8.0, ("matrix", ""))]
    out = multilevel.constraint2coarse(c, g, 2)
    assert out[0].max == 40 and out[1].max == 2.0              # k as on the fine grid (constraint2coarse.jl:21-25), the l1 radius / cf^2
    c = [sipx.set_definitions("cardinality", "DFT", 0, 400, ("matrix", ""))]
    assert multilevel.constraint2coarse(c, g, 2)[0].max == 192  # limited by the number of elements
