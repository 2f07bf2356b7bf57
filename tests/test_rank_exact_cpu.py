"""tests/rank_exact.py on the CPU: the two measures sit at rounding level for a correct truncation -- ties included -- and
stand far above the bound for the errors a rank projector can make."""
import numpy as np
import pytest

from oracle import parsdmm_oracle as O
from tests import rank_exact as R

SHAPE = (72, 76)


def _batch(TF, r, seed=3, nsl=5):
    rng = np.random.default_rng(seed)
    n = SHAPE + (nsl,)
    x = R.stack([R.gapped(SHAPE, r + 2, rng) for _ in range(nsl)]).astype(TF)     # sigma_{r+1}, sigma_{r+2} are large too
    return x, n


@pytest.mark.parametrize("TF", [np.float32, np.float64])
@pytest.mark.parametrize("family", ["gapped", "flat", "rank2", "tied", "single"])
def test_a_rounded_float64_truncation_stays_at_the_floor(TF, family):
    rng = np.random.default_rng(5)
    r = 3
    X = {"gapped": lambda: R.gapped(SHAPE, r, rng), "flat": lambda: R.flat(SHAPE, rng), "rank2": lambda: R.exact_rank2(SHAPE, rng),
         "tied": lambda: R.tied(SHAPE, rng, r), "single": lambda: R.single_entry(SHAPE, rng)}[family]()
    X = X.astype(TF).astype(np.float64)
    Y = R.truncate(X, r).astype(TF)
    u = R.unit_roundoff(TF)
    # rounding moves every entry of T_r(X) by at most u of itself: ||delta||_F <= u ||T_r(X)||_F <= u ||X||_F bounds both
    # measures; the float64 decomposition itself adds a few 2^-53 (visible in the Float64 case only)
    slack = 64 * 2.0 ** -53
    assert R.excess(X, Y, r) <= u + slack and R.rankdefect(X, Y, r) <= u + slack
    assert R.excess(X, Y, r) >= -(u + slack)
    if family == "tied":                 # the tie is exact: sigma_r = sigma_{r+1} to the last bit of the float64 SVD's rounding
        s = np.linalg.svd(X, compute_uv=False)
        assert abs(s[r - 1] - s[r]) <= 1e-13 * s[0] and s[r - 2] > 1.2 * s[r - 1] and R.gap(X, r) < 1e-13
        Z = X.copy()                     # the other way to break the tie is as good
        U, sv, Vt = np.linalg.svd(X, full_matrices=False)
        Z = (U[:, [0, 1, 3]] * sv[[0, 1, 3]]) @ Vt[[0, 1, 3], :]
        assert R.defect(X, Z.astype(TF), r) <= u + slack
    if family == "rank2":
        assert np.linalg.norm(Y - X) <= (u + slack) * np.linalg.norm(X)


def test_zero_slices_must_come_back_as_zeros():
    Z = np.zeros(SHAPE)
    assert R.excess(Z, Z, 2) == 0.0 and R.rankdefect(Z, Z, 2) == 0.0
    W = Z.copy(); W[3, 4] = 1e-30
    assert R.excess(Z, W, 2) == float("inf") and R.rankdefect(Z, W, 2) == float("inf")
    x = np.zeros(72 * 76 * 2, np.float32)
    y = x.copy(); y[5] = 1e-30
    with pytest.raises(AssertionError, match="zero slice"):
        R.check_rank_output(x, y, x, 2, SHAPE + (2,), ("slice", "z"), np.float32)


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("TF", [np.float32, np.float64])
def test_planted_errors_stand_far_above_the_bound(TF, strict):
    r = 4
    x, n = _batch(TF, r)
    mode = ("slice", "z")
    yo = O.project_rank(x.copy(), r, n, mode)
    recs = R.check_rank_output(x, yo, yo, r, n, mode, TF, strict)              # the oracle itself passes its own bound
    assert all(rec["gap"] < 0.1 or rec["to_oracle"] == 0.0 for rec in recs)
    Xs, Yo = R.slices_of(x, n, mode), R.slices_of(yo, n, mode)
    taus = [R.tau(X, Y, r, TF, strict) for X, Y in zip(Xs, Yo)]
    assert max(taus) <= 4 * 4 * R.unit_roundoff(TF)                            # (the oracle's own defect is of the floor's size)

    def planted(fun):
        out = []
        for X, t in zip(Xs, taus):
            Y = np.asarray(fun(X), np.float64).astype(TF)
            out.append((R.excess(X, Y, r), R.rankdefect(X, Y, r), t))
        return out

    # 1. a rank r - 1 output: excess
    for e, d, t in planted(lambda X: R.truncate(X, r - 1)):
        assert e > 100 * t and d <= t
    # 2. the top r - 1 directions plus direction r + 1 (a missed large direction): rank r, but too far away
    def wrong_direction(X):
        U, s, Vt = np.linalg.svd(X, full_matrices=False)
        k = list(range(r - 1)) + [r]
        return (U[:, k] * s[k]) @ Vt[k, :]
    for e, d, t in planted(wrong_direction):
        assert e > 100 * t and d <= t
    # 3. two slices swapped: each is an optimal truncation -- of another slice
    ys = [Yo[1], Yo[0]] + Yo[2:]
    for i in (0, 1):
        assert R.excess(Xs[i], ys[i], r) > 100 * taus[i]
    with pytest.raises(AssertionError):
        R.check_rank_output(x, R.stack(ys).astype(TF), yo, r, n, mode, TF, strict)
    # 4. a correct subspace applied without its last rounding-level care: an output of rank r + 1 by a direction at 1e-4
    for e, d, t in planted(lambda X: R.truncate(X, r) + 1e-4 * (R.truncate(X, r + 1) - R.truncate(X, r))):
        assert d > 100 * t


def test_slices_follow_the_reference_order():
    n = (3, 4, 5)
    x = np.arange(60, dtype=np.float64)
    X = x.reshape(n, order="F")
    for d, ax in (("x", 0), ("y", 1), ("z", 2)):
        sl = R.slices_of(x, n, ("slice", d))
        assert len(sl) == n[ax] and all(np.array_equal(s, np.take(X, i, axis=ax)) for i, s in enumerate(sl))
        assert np.array_equal(R.stack(sl, d), x)
    assert np.array_equal(R.slices_of(x[:12], (3, 4), ("matrix", ""))[0], x[:12].reshape((3, 4), order="F"))
