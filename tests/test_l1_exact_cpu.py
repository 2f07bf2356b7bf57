"""tests/l1_exact.py pinned against the oracle and closed forms, and proof that its checker bites: every wrong "engine
output" below is one a 2e-5 comparison in norm lets through."""
import numpy as np
import pytest

from oracle import parsdmm_oracle as O
from tests import l1_exact as X


def heavy(n, TF, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * np.exp(rng.standard_normal(n))).astype(TF)


# ---- pins -----------------------------------------------------------------------------------------------------------------
# (radii up to 0.9 ||v||_1: the oracle forms sv - b in float64, whose cancellation error 2^-53 sv / (sv - b) is the oracle's
#  own and passes 1e-13 from about 0.999 ||v||_1 on)
@pytest.mark.parametrize("n,frac,seed", [(1000, 0.3, 1), (4099, 0.01, 2), (4099, 0.6, 3), (257, 0.9, 4), (64, 0.5, 5)])
def test_exact_theta_agrees_with_the_oracle_in_float64(n, frac, seed):
    a = np.abs(heavy(n, np.float64, seed))
    b = frac * a.sum()
    th, C, S = X.exact_theta(a, b)
    ref = float(O.l1ball_theta_duchi(a, b))
    assert abs(th - ref) <= 1e-13 * ref
    # what is returned with it: the active set and its sum
    assert C == int((a > th).sum()) and abs(S - a[a > th].sum()) <= 1e-12 * S


def test_exact_theta_on_ties_and_on_a_single_entry():
    a = np.abs(np.array([3, 3, 3, 3, -3, 1, 0, 0], np.float64))
    th, C, S = X.exact_theta(a, 5.0)
    assert (th, C, S) == (2.0, 5, 15.0)
    assert abs(th - float(O.l1ball_theta_duchi(a, 5.0))) <= 1e-13 * th
    th, C, S = X.exact_theta(np.array([7.0]), 2.0)            # lv = 1: the scan never starts, rho = max(1, 0)
    assert (th, C, S) == (5.0, 1, 7.0)
    assert abs(th - float(O.l1ball_theta_duchi(np.array([7.0]), 2.0))) <= 1e-13 * th


@pytest.mark.parametrize("M", [5, 64])
def test_exact_theta_all_active_closed_form(M):
    """Magnitudes in [2, 3], b = 0.8 ||v||_1: nothing would be zeroed, so the scan stops at lv - 1 (the reference's quirk)."""
    a = 2.0 + np.random.default_rng(M).random(M)
    b = 0.8 * a.sum()
    th, C, S = X.exact_theta(a, b)
    assert C == M - 1
    want = (a.sum() - a.min() - b) / (M - 1)
    assert abs(th - want) <= 1e-14 * want
    assert th < a.min()                                        # ... although every entry stays active
    assert abs(th - float(O.l1ball_theta_duchi(a, b))) <= 1e-13 * th


def test_soft_is_the_arithmetic_of_the_device_function():
    v = np.array([3.0, -3.0, 0.25, -0.25, 0.5, 0.0, -0.0], np.float32)
    y = X.soft(v, np.float32(0.5))
    assert X.same_bits(y, np.array([2.5, -2.5, 0.0, -0.0, 0.0, 0.0, -0.0], np.float32))
    assert y.dtype == np.float32


def test_theta_tol_is_the_stated_formula():
    th = 0.37
    for TF in (np.float32, np.float64):
        assert X.theta_tol(100, 50.0, 7.0, th, TF) == 0.5 * float(np.spacing(TF(th))) + 4 * 2.0 ** -53 * 57.0


# ---- the checker: the correct output passes, every wrong one is rejected ---------------------------------------------------
TF = np.float32
V = heavy(4099, TF, 11)
ABS = np.abs(V.astype(np.float64))
B = float(TF(0.3 * ABS.sum()))
TH, C_ACT, S_ACT = X.exact_theta(ABS, B)
# the all-active companion: theta* about half the smallest magnitude
B_ALL = float(TF(ABS.sum() - 0.5 * len(V) * ABS.min()))
TH_ALL, C_ALL, _ = X.exact_theta(ABS, B_ALL)


def both_modes_reject(v, y, b, theta):
    with pytest.raises(AssertionError):
        X.check_l1_output(v, y, b, theta)
    with pytest.raises(AssertionError):
        X.check_l1_output(v, y, b)


def test_the_correct_output_passes():
    for b, th in ((B, TH), (B_ALL, TH_ALL)):
        y = X.soft(V, TF(th))
        r = X.check_l1_output(V, y, b, float(TF(th)))
        assert r is not None and r <= 1.0
        X.check_l1_output(V, y, b)
    assert C_ALL == len(V) - 1 and TH_ALL < ABS.min()
    # float64: more than four TF numbers lie within the bound, the element-wise form of the check
    v = heavy(4099, np.float64, 12)
    b = 0.3 * np.abs(v).sum()
    th = X.exact_theta(np.abs(v), b)[0]
    X.check_l1_output(v, X.soft(v, th), b)
    X.check_l1_output(v, X.soft(v, th), b, th)
    # feasible input: bit for bit
    w = (V * TF(1e-3)).astype(TF)
    X.check_l1_output(w, w.copy(), B)
    X.check_l1_output(w, w.copy(), B, 0.0)
    with pytest.raises(AssertionError):
        X.check_l1_output(w, X.soft(w, TF(1e-9)), B)


def test_rejects_a_gather_that_drops_the_magnitude_on_the_upper_bracket_edge():
    """Bracket (lo, hi] with hi an actual magnitude 0.1 % above theta*; a gather written `lo < |v| < hi` beside a sum of
    what lies `> hi` loses that one entry: theta moves by (hi - theta*) / C, a few Float32 ulps."""
    j = int(np.argmin(np.abs(ABS - TH * 1.001) + np.where(ABS > TH, 0, np.inf)))
    th_bug = X.exact_theta(np.delete(ABS, j), B)[0]
    assert 0 < abs(th_bug - TH) < 1e-5 * TH                       # far inside the old 2e-5-in-norm acceptance
    both_modes_reject(V, X.soft(V, TF(th_bug)), B, float(TF(th_bug)))


def test_rejects_a_pad_counted_as_an_element():
    """All entries active: one extra zero (a pad of the padded layout) becomes min|v| and makes lv one larger."""
    th_bug = X.exact_theta(np.append(ABS, 0.0), B_ALL)[0]
    assert abs(th_bug - TH_ALL) < 1e-3 * TH_ALL
    both_modes_reject(V, X.soft(V, TF(th_bug)), B_ALL, float(TF(th_bug)))


def test_rejects_the_all_active_case_solved_with_lv():
    th_bug = (float(np.sum(ABS)) - B_ALL) / len(V)                # Michelot's fixed point: every entry active, rho = lv
    assert abs(th_bug - TH_ALL) < 1e-3 * TH_ALL
    both_modes_reject(V, X.soft(V, TF(th_bug)), B_ALL, float(TF(th_bug)))


@pytest.mark.parametrize("up", [True, False])
def test_rejects_theta_two_ulps_off(up):
    t = TF(TH)
    for _ in range(2):
        t = np.nextafter(t, TF(np.inf if up else -np.inf))
    both_modes_reject(V, X.soft(V, t), B, float(t))


def test_rejects_an_entry_flushed_to_zero_next_to_theta():
    t = TF(TH)
    y = X.soft(V, t)
    j = int(np.argmin(np.where(y != 0, np.abs(V), np.inf)))        # the smallest survivor
    assert y[j] != 0 and abs(float(y[j])) < 1e-2 * TH
    y[j] = 0
    both_modes_reject(V, y, B, float(t))


def test_rejects_a_subtraction_in_float64_rounded_afterwards():
    y = (np.sign(V) * np.maximum(ABS - TH, 0.0)).astype(TF)
    assert np.linalg.norm(y - X.soft(V, TF(TH))) < 1e-6 * np.linalg.norm(y)
    both_modes_reject(V, y, B, float(TF(TH)))
