"""Reference of group cardinality { v = A x : at most k segments of v are non-zero } (csrc/card_groups.h), pure numpy.  v is the M-vector
of the range of A (identity, D_x, D_y, D_z) in the reference's row order: the array of shape TD_n in column-major order.  Segments and
their order come from tests/l21_groups_ref.py (the order of sipx.segment_norms and sipx.group_norms).

The projection keeps the k first segments of the stable descending order of the selection key g -- magnitude descending, ties to the lower
segment index -- bit for bit and writes +0 over the others; with at most k non-zero keys it returns v itself.  The key is the exactly
summed l2 norm of a segment rounded once to the precision of v, or an array the caller hands in (the device's own norms)."""
import math
from fractions import Fraction

import numpy as np

from tests import l21_groups_ref as G

segments, nseg, rows, td_n = G.segments, G.nseg, G.rows, G.td_n


def exact_sumsq(v, n, op, mode):
    """sum of squares per segment as exact rationals (every float is a dyadic rational)."""
    v = np.asarray(v, np.float64)
    out = []
    for idx in segments(n, op, mode):
        x = v[idx][v[idx] != 0]
        if not len(x):
            out.append(Fraction(0))
            continue
        m, e = np.frexp(x)                                   # x = m 2^e, |m| in [0.5, 1): m 2^53 is an integer
        mi = [int(q) for q in np.ldexp(m, 53)]
        e0 = int(e.min())
        S = sum((q << (int(ei) - e0)) ** 2 for q, ei in zip(mi, e))      # big integers: exact
        out.append(Fraction(S) * Fraction(2) ** (2 * (e0 - 53)))
    return out


def exact_norms(v, n, op, mode):
    """The segment norms in float64 from math.fsum of the squares: in Float32 the squares are exact in float64 and fsum rounds their sum
    once; in Float64 the squares themselves round (half a unit each), which the 1-unit bound of the test on Float64 norms has room for only
    through the exact route -- see norm_error_units, which compares against the rational sum."""
    v = np.asarray(v, np.float64)
    return np.array([math.sqrt(math.fsum(float(x) * float(x) for x in v[idx])) for idx in segments(n, op, mode)], np.float64)


def norm_error_units(g, v, n, op, mode):
    """max over the segments of |g_s - sqrt(exact sum of squares)| / (eps_T sqrt(...)), the comparison made in exact arithmetic on the
    squares: (g_s (1 -+ r eps))^2 against the rational sum, bisected on r to 1/64."""
    g = np.asarray(g)
    eps = Fraction(float(np.finfo(g.dtype).eps))
    worst = 0.0
    for gs, S in zip(g, exact_sumsq(v, n, op, mode)):
        gs = Fraction(float(gs))
        if S == 0:
            assert gs == 0, "a zero segment with a non-zero norm"
            continue
        lo, hi = Fraction(0), Fraction(8)          # |g - sqrt(S)| <= r eps sqrt(S)  <=>  S (1 - r eps)^2 <= g^2 <= S (1 + r eps)^2
        ok = lambda r: S * (1 - r * eps) ** 2 <= gs * gs <= S * (1 + r * eps) ** 2
        if not ok(hi):
            return float("inf")
        for _ in range(9):
            mid = (lo + hi) / 2
            lo, hi = (lo, mid) if ok(mid) else (mid, hi)
        worst = max(worst, float(hi))
    return worst


def norms(v, n, op, mode, TF):
    """g of the contract: the exactly summed segment norms rounded once to TF."""
    return exact_norms(v, n, op, mode).astype(TF)


def kept(g, k):
    """Boolean mask of the segments the stable selection on the key g keeps; all of them where at most k keys are non-zero."""
    g = np.asarray(g)
    k = int(k)
    if k >= len(g) or int(np.count_nonzero(g > 0)) <= k:
        return np.ones(len(g), bool)
    keep = np.zeros(len(g), bool)
    keep[np.argsort(-g.astype(np.float64), kind="stable")[:k]] = True
    return keep


def project(v, n, op, mode, k, g=None):
    """The projection of v (same dtype); v itself when nothing is dropped.  g: the selection key, default norms(v)."""
    v = np.asarray(v)
    g = norms(v, n, op, mode, v.dtype.type) if g is None else np.asarray(g)
    keep = kept(g, k)
    if keep.all():
        return v
    y = v.copy()
    for s, idx in enumerate(segments(n, op, mode)):
        if not keep[s]:
            y[idx] = 0
    return y


def gap(g, k):
    """(g_(k) - g_(k+1)) / g_(k) of the descending order: how far the selection is from a flip (inf where nothing is dropped)."""
    s = np.sort(np.asarray(g, np.float64))[::-1]
    k = int(k)
    if k >= len(s) or s[k - 1] == 0:
        return float("inf")
    return float((s[k - 1] - s[k]) / s[k - 1])
