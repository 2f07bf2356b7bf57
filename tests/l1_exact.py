"""Exact reference of the l1-ball threshold (pure numpy, no GPU) and the checks an engine output is held to.

The engine claims (csrc/kernels_proj.hip, header, step 4) that theta is the exact fixed point of
f(theta) = sum(max(|v| - theta, 0)) - b, evaluated in float64 and rounded once to the working precision TF, and that
the projection then is one TF subtraction per element (soft_thr, csrc/sipx_device.h).  `exact_theta` is the rule of
src/projectors/project_l1_Duchi!.jl:33-46 as oracle.l1ball_theta_duchi states it, in float64 with an extended-precision
cumulative sum; `check_l1_output` holds an output to that threshold with the bound derived in `theta_tol`."""
import numpy as np

_WIDE = np.longdouble if np.finfo(np.longdouble).nmant > np.finfo(np.float64).nmant else np.float64


def exact_theta(absv, b):
    """(theta64, C, S_act): threshold, size of the active set and its sum of magnitudes.

    Descending sort; scan `u[j] > (sv[j] - b) / (j + 1)` that stops at the first failure and never goes past lv - 1 (the
    reference's `&& rho + 1 < lv`: when nothing would be zeroed, theta = (||v||_1 - min|v| - b) / (lv - 1));
    rho = max(1, rho); theta = max(0, .).  lv = len(absv): the rows of the operator, never a padded length."""
    u = np.sort(np.asarray(absv, np.float64))[::-1]
    lv = len(u)
    if lv == 0:
        raise ValueError("empty vector")
    b = float(b)
    sv = np.cumsum(u.astype(_WIDE))
    kk = np.arange(1, lv + 1)
    cond = (u.astype(_WIDE) > (sv - _WIDE(b)) / kk.astype(_WIDE)) & (kk < lv)
    stop = np.nonzero(~cond)[0]
    rho = int(stop[0]) if len(stop) else lv
    rho = max(1, rho)
    S_act = float(sv[rho - 1])
    theta = float((sv[rho - 1] - _WIDE(b)) / _WIDE(rho))
    return max(0.0, theta), rho, S_act


def soft(v, theta_TF):
    """soft_thr of csrc/sipx_device.h in v's precision: t = |v| - theta; t = t > 0 ? t : 0; the sign of v; v == 0 returns v
    itself (so -0.0 stays -0.0)."""
    v = np.asarray(v)
    TF = v.dtype.type
    t = (np.abs(v) - TF(theta_TF)).astype(TF)
    t = np.where(t > 0, t, TF(0)).astype(TF)
    return np.where(v > 0, t, np.where(v < 0, -t, v)).astype(TF)


def ulp(x, TF):
    return float(np.spacing(np.abs(TF(x))))


def theta_tol(C, S_act, b, theta64, TF):
    """ulp_TF(theta*) / 2 + 4 * 2^-53 * (S_act + b).

    First term: the one rounding of the float64 theta to TF.  Second term: a float64 sum of C terms in any order is off by
    at most (C - 1) 2^-53 S_act; divided by C that leaves at most 2^-53 S_act; the subtraction of b and the division add a
    relative 2 * 2^-53 of (S_act + b) / C; once for the engine and once for this reference.  This is the bound of an exact
    fixed point: k_l1_solve iterates until the active count stops changing (no stopping tolerance), so nothing is added."""
    return 0.5 * ulp(theta64, TF) + 4.0 * 2.0 ** -53 * (float(S_act) + float(b))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool(np.array_equal(_bits(a), _bits(b)))


def feasibility(v, b):
    """+1: ||v||_1 <= b away from the rounding of a TF asum, -1: > b away from it, 0: too close to call."""
    TF = np.asarray(v).dtype.type
    a = float(np.sum(np.abs(np.asarray(v, np.float64)).astype(_WIDE)))
    b = float(b)
    margin = 4.0 * float(np.finfo(TF).eps) * b
    return 1 if a <= b - margin else (-1 if a > b + margin else 0)


def _candidates(theta64, tol, TF):
    """TF numbers in [theta* - tol, theta* + tol]; the enumeration stops at five (the caller asks whether there are at most four)."""
    lo, hi = theta64 - tol, theta64 + tol
    t = TF(lo)
    if float(t) < lo:
        t = np.nextafter(t, TF(np.inf))
    out = []
    while float(t) <= hi and len(out) <= 4:
        out.append(t)
        t = np.nextafter(t, TF(np.inf))
    return out


def check_l1_output(v, y, b, theta_engine=None):
    """Raise AssertionError unless y is the projection of v onto the l1 ball of radius b (a TF number) the engine claims.
    Returns |theta_e - theta*| / theta_tol when theta_engine is given and the input is infeasible, else None."""
    v, y = np.asarray(v), np.asarray(y)
    TF = v.dtype.type
    assert y.dtype == v.dtype and y.shape == v.shape, "output of another type or shape"
    assert float(TF(b)) == float(b), "the radius is a number of the working precision"
    fz = feasibility(v, b)
    if fz > 0 or (fz == 0 and same_bits(y, v)):
        assert same_bits(y, v), "a feasible input must come back bit for bit"
        return None
    absv = np.abs(v.astype(np.float64))
    th, C, S = exact_theta(absv, b)
    tol = theta_tol(C, S, b, th, TF)
    if theta_engine is not None:
        te = float(theta_engine)
        assert float(TF(te)) == te, "theta is handed out as a TF number"
        err = abs(te - th)
        assert err <= tol, f"theta {te!r} misses the exact {th!r} by {err:.3e} > tol {tol:.3e} (C = {C})"
        ref = soft(v, TF(te))
        if not same_bits(y, ref):
            bad = np.nonzero(_bits(y) != _bits(ref))[0]
            raise AssertionError(f"y is not soft(v, theta) bit for bit at {len(bad)} entries, first {bad[0]}: "
                                 f"v {v[bad[0]]!r} y {y[bad[0]]!r} expected {ref[bad[0]]!r}")
        return err / tol
    cand = _candidates(th, tol, TF)
    if len(cand) <= 4:
        assert any(same_bits(y, soft(v, t)) for t in cand), \
            f"y is soft(v, t) for none of the {len(cand)} TF numbers within {tol:.3e} of theta* = {th!r}"
        return None
    y64 = y.astype(np.float64)
    assert np.isfinite(y64).all(), "non-finite output"
    zero = v == 0
    assert same_bits(y[zero], v[zero]), "zeros (and their signs) must come back as they are"
    assert np.array_equal(np.signbit(y[~zero]), np.signbit(v[~zero])), "signs are those of v"
    d = absv - th
    clear_in, clear_out = d > tol, d < -tol
    assert np.all(y64[clear_out] == 0), "an entry clearly below theta* survived"
    assert np.all(y64[clear_in] != 0), "an entry clearly above theta* was zeroed"
    sup = y64 != 0
    slack = tol + np.spacing(np.abs(v[sup])).astype(np.float64)
    miss = np.abs(np.abs(y64[sup]) - d[sup])
    assert np.all(miss <= slack), f"|y| misses |v| - theta* by up to {float((miss - slack).max()):.3e} beyond the bound"
    return None
