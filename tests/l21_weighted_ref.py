"""Reference of the weighted l2,1 ball { v : sum_p w_p g_p <= tau } (csrc/l21_weighted.h), pure numpy in np.longdouble, built on the
groups and norms of tests/l21_ref.py (TV), tests/l21_frames_ref.py (TV_xy, whole array) and tests/l21_joint_ref.py (one group per pixel).

theta is exact: the breakpoints g_p / w_p are sorted (stable, descending; a group of weight 0 is never active), and theta is
(S_k - tau) / C_k for the longest prefix whose last breakpoint lies above it.  `emulate_search` is the contract of the header --
Michelot's iteration with its sums in twice the working precision, serially in index order -- in Python floats, bit for bit."""
import math
from fractions import Fraction

import numpy as np

from tests import l1_exact, l21_frames_ref, l21_joint_ref, l21_ref

W = l1_exact._WIDE
KINDS = ("TV", "TV_xy", "joint")


def rows(n, kind):
    return l21_ref.rows(n) if kind == "TV" else l21_frames_ref.rows(n)


def ngroups(n, kind):
    return int(n[0]) * int(n[1]) if kind == "joint" else int(np.prod(n))


def norms(v, n, kind, TF):
    """g of the contract, one per group, in TF: exactly the unweighted sets' norms."""
    if kind == "TV":
        return l21_ref.norms(v, n, TF)
    if kind == "TV_xy":
        return l21_frames_ref.norms(v, n, TF).reshape(-1, order="F")
    return l21_joint_ref.norms(v, n, TF)


def exact_norms(v, n, kind):
    """The unrounded group norms in float64."""
    if kind == "TV":
        return np.sqrt(l21_ref.sumsq(v, n))
    if kind == "TV_xy":
        return np.sqrt(l21_frames_ref.sumsq(v, n)).reshape(-1, order="F")
    return l21_joint_ref.exact_norms(v, n)


def members(n, kind):
    """(groups, m) int64: the M-vector indices of every group's members, -1 where there is none."""
    if kind == "TV":
        return l21_ref.groups(n)
    if kind == "TV_xy":
        return l21_frames_ref.groups(n)
    G = l21_joint_ref._members(n)
    return G.reshape(G.shape[0], -1)


def norm(v, n, kind, w):
    """sum_p w_p g_p of the TF group norms (what the projector compares with tau), in extended precision."""
    v = np.asarray(v)
    g = norms(v, n, kind, v.dtype.type)
    return float(np.sum(np.asarray(w).astype(W) * g.astype(W)))


def exact_theta(g, w, tau):
    """theta of the weighted ball on the numbers g with weights w >= 0, exact up to the rounding of extended precision; 0.0 inside."""
    g, w = np.asarray(g).astype(W), np.asarray(w).astype(W)
    tau = W(tau)
    if np.sum(w * g) <= tau:
        return 0.0
    pos = (w > 0) & (g > 0)
    gp, wp = g[pos], w[pos]
    r = gp / wp
    order = np.argsort(-r, kind="stable")
    gp, wp, r = gp[order], wp[order], r[order]
    S, C = np.cumsum(wp * gp), np.cumsum(wp * wp)
    th = (S - tau) / C
    ok = np.nonzero(r > th)[0]
    k = int(ok[-1]) if len(ok) else 0
    return max(float(th[k]), 0.0)


def feasibility(g, w, tau):
    """+1: sum w g <= tau away from the rounding of a TF asum, -1: > tau away from it, 0: too close to call."""
    TF = np.asarray(g).dtype.type
    a = float(np.sum(np.asarray(w).astype(W) * np.asarray(g).astype(W)))
    margin = 4.0 * float(np.finfo(TF).eps) * float(tau)
    return 1 if a <= float(tau) - margin else (-1 if a > float(tau) + margin else 0)


def project(v, n, kind, w, tau):
    """The projection of v onto { sum_p w_p g_p <= tau } in float64: the exact theta of the TF group norms (the array the engine
    iterates on), the factors max(g - theta w, 0) / g from the unrounded norms; groups of weight 0 keep their entries.  v itself
    comes back when `feasibility` says inside."""
    v = np.asarray(v)
    TF = v.dtype.type
    g = norms(v, n, kind, TF)
    if feasibility(g, w, tau) > 0:
        return v
    theta = exact_theta(g, w, tau)
    g64 = exact_norms(v, n, kind)
    w64 = np.asarray(w, np.float64)
    f = np.ones_like(g64)
    act = w64 > 0
    pos = act & (g64 > 0)
    f[act] = 0.0
    f[pos] = np.maximum(g64[pos] - theta * w64[pos], 0.0) / g64[pos]
    G = members(n, kind)
    y = np.asarray(v, np.float64).copy()
    for q in range(G.shape[1]):
        has = (G[:, q] >= 0) & act
        y[G[has, q]] = y[G[has, q]] * f[has]
    return y


# ---- the contract of csrc/l21_weighted.h in Python floats -------------------------------------------------------------------------------
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _fma_err(x, y, p):
    """fma(x, y, -p) for p = fl(x y): the product's rounding error, which is a float64."""
    return float(Fraction(x) * Fraction(y) - Fraction(p))


class _Sum:
    def __init__(self):
        self.hi = self.lo = 0.0

    def add_product(self, x, y, double):
        p = x * y
        s, e = _two_sum(self.hi, p)
        self.hi = s
        self.lo += e
        if double:
            self.lo += _fma_err(x, y, p)


def _theta_of(S, C, tau):
    d, e = _two_sum(S.hi, -tau)
    nlo = e + S.lo
    if C.hi == 0.0 or not math.isfinite(d + nlo):      # (x / 0, then fma(inf, 0, d): the header returns NaN, which never raises theta)
        return math.nan
    q = (d + nlo) / C.hi
    r = float(Fraction(-q) * Fraction(C.hi) + Fraction(d))      # fma(-q, C.hi, d): the exact value rounded once
    r = (r + nlo) - q * C.lo
    return q + r / C.hi


def clean(w):
    w = np.asarray(w)
    return np.where((w > 0) & np.isfinite(w), w, w.dtype.type(0)).astype(w.dtype)


def emulate_search(g, w, tau):
    """(need, theta in TF, (TF)asum, passes) of l21w_search_serial on the TF arrays g, w and the TF radius tau."""
    TF = g.dtype.type
    double = TF == np.float64
    gl, wl = [float(x) for x in g], [float(x) for x in clean(w)]
    tau = float(TF(tau))

    def sums(theta):
        S, C, cnt = _Sum(), _Sum(), 0
        for a, b in zip(gl, wl):
            if theta is None or a > theta * b:
                S.add_product(b, a, double)
                C.add_product(b, b, double)
                cnt += 1
        return S, C, cnt
    S, C, prev = sums(None)
    asum = S.hi + S.lo
    passes = 1
    if TF(asum) <= TF(tau):
        return 0, TF(0), TF(asum), passes
    theta = _theta_of(S, C, tau)
    while True:
        S, C, cnt = sums(theta)
        passes += 1
        if cnt > 0:
            th = _theta_of(S, C, tau)
            theta = th if th > theta else theta
        if cnt == 0 or cnt == prev:
            return 1, TF(theta if theta > 0 else 0.0), TF(asum), passes
        prev = cnt
        assert passes <= len(gl) + 2


def emulate_apply(v, g, w, theta):
    """v (groups, m) with every member multiplied by l21w_factor(g, w, theta) in TF; groups of weight 0 keep their bits."""
    TF = v.dtype.type
    wc = clean(w)
    t = (g - (TF(theta) * wc).astype(TF)).astype(TF)
    t = np.where(t > 0, t, TF(0)).astype(TF)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(g > 0, (t / g).astype(TF), TF(0)).astype(TF)
    return np.where((wc > 0)[:, None], (v * f[:, None]).astype(TF), v).astype(TF), f
