"""Constraint learning (sipx.constraint_learning_by_obseration) without a device: the numpy restatement against hand-worked
answers and the reference's quirks, and every refusal of the host function."""
import numpy as np
import pytest

from tests import learn_ref as R


def _rank_one(TF):
    # img[a, c] = (a + 1)(c + 1) on a 3 x 4 grid, h = (1, 1): rank one, D_x img = c + 1, D_z img = a + 1
    return np.outer(np.arange(1, 4), np.arange(1, 5)).astype(TF)


@pytest.mark.parametrize("TF", [np.float32, np.float64])
def test_restatement_hand_worked_3x4(TF):
    o = R.learn(_rank_one(TF)[None], (1.0, 1.0))
    TI = np.int32 if TF == np.float32 else np.int64
    close = lambda k, v: np.testing.assert_allclose(float(o[k][0]), v, rtol=1e-6 if TF == np.float32 else 1e-13)
    close("nuclear_norm", np.sqrt(14 * 30))          # |u| |v| with u = (1, 2, 3), v = (1, 2, 3, 4)
    close("nuclear_Dx", np.sqrt(2 * 30))             # rows (1 2 3 4) twice
    close("nuclear_Dz", np.sqrt(14 * 3))             # columns (1 2 3) three times
    close("Dx_l1", 20.0)
    close("Dz_l1", 18.0)
    close("TV", 38.0)
    close("D_l2", np.sqrt(102.0))
    close("TV_annulus", np.sqrt(102.0))
    close("annulus", np.sqrt(420.0))
    # unitary DFT of a separable image: |F3 u|_1 = 2 sqrt(3) + 2, |F4 v|_1 = 5 + 2 sqrt(2) + 1
    close("DFT_l1", (2 * np.sqrt(3) + 2) * (6 + 2 * np.sqrt(2)))
    assert o["D_x_min"][0] == 1 and o["D_x_max"][0] == 4 and o["D_z_min"][0] == 1 and o["D_z_max"][0] == 3
    assert o["rank_095"].dtype == TI and o["rank_095"][0] == 1
    # sorted |TV| = 1 x5, 2 x5, 3 x5, 4 x2; cumsum / 38 passes 0.05 at the 2nd entry: 17 - 2
    assert o["TV_card_095"][0] == 15
    # sorted |F| = 1, 1, sqrt2 x4, 2 sqrt3, 2 sqrt6 x2, 5 x2, 10 sqrt3; 0.05 of the total (48.2) is passed at the 3rd entry
    assert o["DFT_card_095"][0] == 9
    assert o["wavelet_l1"][0] == 0                   # n1 != n2
    assert np.array_equal(o["hist_min"], [1, 2, 2, 3, 3, 4, 4, 6, 6, 8, 9, 12])
    assert np.array_equal(o["hist_TV_max"], [1] * 5 + [2] * 5 + [3] * 5 + [4] * 2)
    # the DC row of the DCT along dim 1 is sqrt(3) * 2 (c + 1): min 2 sqrt3, max 8 sqrt3
    np.testing.assert_allclose(o["DCT_x_LB"][0], 2 * np.sqrt(3), rtol=1e-6)
    np.testing.assert_allclose(o["DCT_x_UB"][0], 8 * np.sqrt(3), rtol=1e-6)
    np.testing.assert_allclose(o["DCT_y_UB"][0], 3 * 5, rtol=1e-6)      # DC of (a + 1)(1 2 3 4) along dim 2: 10 (a + 1) / 2


@pytest.mark.parametrize("TF", [np.float32, np.float64])
def test_restatement_quirks(TF):
    TI = np.int32 if TF == np.float32 else np.int64
    neg = -_rank_one(TF)
    o = R.learn(np.stack([neg, np.zeros_like(neg)]), (1.0, 1.0))
    for k in ("hist_min", "hist_TV_min", "DCT_x_LB", "DCT_y_LB"):
        assert o[k].dtype == np.float64, k
    for k in ("hist_max", "hist_TV_max", "DCT_x_UB", "DCT_y_UB", "TV", "nuclear_norm"):
        assert o[k].dtype == TF, k
    for k in ("rank_095", "DFT_card_095", "TV_card_095"):
        assert o[k].dtype == TI and o[k][1] == 0, k      # all-zero image: 0, where the reference throws
    assert np.all(o["hist_max"] == 0)                    # starts at 0: an all-negative batch leaves it there
    assert o["hist_min"].max() == -1 and o["hist_min"].min() == -12
    # a single positive image: the minima keep 1e8 nowhere, the maxima keep 0 nowhere
    p = R.learn(_rank_one(TF)[None], (1.0, 1.0))
    assert np.all(p["hist_min"] < 1e8) and np.all(p["hist_max"] > 0)
    # one all-zero image: every minimum stays at 0 < 1e8 and the DCT bounds are 0
    z = R.learn(np.zeros((1, 3, 4), TF), (1.0, 1.0))
    assert np.all(z["DCT_x_LB"] == 0) and np.all(z["hist_min"] == 0)


def test_restatement_spacing_is_rounded_in_tf():
    img = np.arange(12, dtype=np.float32).reshape(3, 4)
    dx, dz = R.diffs(img, (3.0, 7.0))
    ih = np.float32(1) / np.float32(3.0)
    assert dx.dtype == np.float32 and dx[0, 0] == (-ih) * np.float32(0) + ih * np.float32(4)


def _grid(sipx, n, d=None):
    return sipx.compgrid(d or tuple(1.0 for _ in n), n)


def test_refusals_without_a_device(sipx):
    f = sipx.constraint_learning_by_obseration
    m = np.zeros((2, 4, 5), np.float32)
    with pytest.raises(sipx.SipxError, match="2-D"):
        f(_grid(sipx, (4, 5, 3)), np.zeros((2, 4, 5, 3), np.float32))
    with pytest.raises(sipx.SipxError, match="n1 >= 2"):
        f(_grid(sipx, (1, 5)), np.zeros((2, 1, 5), np.float32))
    with pytest.raises(sipx.SipxError, match="n1 >= 2"):
        f(_grid(sipx, (4, 1)), np.zeros((2, 4, 1), np.float32))
    with pytest.raises(sipx.SipxError, match="does not match"):
        f(_grid(sipx, (5, 4)), m)
    with pytest.raises(sipx.SipxError, match="does not match"):
        f(_grid(sipx, (4, 5)), np.zeros(20, np.float32))
    with pytest.raises(sipx.SipxError, match="real"):
        f(_grid(sipx, (4, 5)), m.astype(np.complex64))
    with pytest.raises(sipx.SipxError, match="real"):
        f(_grid(sipx, (4, 5)), m.astype(np.int32))
    with pytest.raises(sipx.SipxError, match="unknown key"):
        f(_grid(sipx, (4, 5)), m, keys=["curvelet_l1"])


def test_alias_and_exports(sipx):
    assert sipx.constraint_learning_by_observation is sipx.constraint_learning_by_obseration
    assert "sipx_learn_observations" in sipx.EXPORTED_SYMBOLS
    assert tuple(sipx.LEARN_KEYS) == R.KEYS
    assert [f for f, _ in sipx.host._Observations._fields_] == list(R.KEYS)
