"""Reference of the simplex sets { v : v_i >= 0, smin <= sum_i v_i <= smax } per fiber / slice (csrc/seg_simplex.h), no GPU.

exact_segment  the projection of one segment in rational arithmetic on the float values: the sort-based threshold
               rho = max{ j : u_j - (sum_{r<=j} u_r - b) / j > 0 },  theta* = (sum_{r<=rho} u_r - b) / rho  on the face sum = b the segment
               goes to, every entry max(v_i - theta*, 0) rounded once to float64.  The floats are scaled to integers by a common power of
               two, so every sum is a sum of Python ints.
project        ... of every segment of the M-vector of the range of A (identity, D_x, D_y, D_z) in the reference's row order, segments in the
               order of tests/seg_norms_ref.segment_indices (that of sipx.segment_norms and sipx.segment_sums).
emulate        the rule of the header step by step in IEEE arithmetic (Python floats are float64, nothing is fused): the pair sums of
               csrc/l21.h, simplex_theta with its exact remainder, Michelot's loop, the apply in TF -- the bits of simplex_project_serial."""
from fractions import Fraction

import numpy as np

from tests import seg_norms_ref

KEEP, CLIP, SHIFT = 0, 1, 2


def td_n(n, op):
    """TD_n: the shape of the range of `op` on the grid n."""
    n = [int(v) for v in n]
    if op != "identity":
        n[{"D_x": 0, "D_y": 1, "D_z": len(n) - 1}[op]] -= 1
    return tuple(n)


def rows(n, op):
    return int(np.prod(td_n(n, op)))


def segments(n, op, mode):
    """One index array into the M-vector per segment, in the order of segment_sums()."""
    return seg_norms_ref.segment_indices(td_n(n, op), mode)


def _ints(values):
    """Integers k and D, a power of two, with values[i] == k[i] / D exactly."""
    fr = [float(x).as_integer_ratio() for x in values]
    D = max(d for _, d in fr)
    return [p * (D // d) for p, d in fr], D


def exact_segment(v, smin, smax):
    """(x, theta*, case): the exact projection of the finite segment v rounded once to float64, the threshold as a Fraction (0 unless
    the segment is shifted) and KEEP / CLIP / SHIFT."""
    k, D = _ints(list(v) + [smin, smax])
    kv, kmin, kmax = k[:-2], k[-2], k[-1]
    spos = sum(a for a in kv if a > 0)
    if kmin <= spos <= kmax:
        x = np.array([float(a) if a > 0 else 0.0 for a in np.asarray(v, np.float64)])
        return x, Fraction(0), (CLIP if any(a < 0 for a in kv) else KEEP)
    b = kmax if spos > kmax else kmin
    cs, rho, csr = 0, 0, 0
    for j, u in enumerate(sorted(kv, reverse=True), 1):
        cs += u
        if u * j > cs - b:
            rho, csr = j, cs
    th = Fraction(csr - b, rho)                     # in units of 1 / D
    x = np.array([float(Fraction(a - th) / D) if a > th else 0.0 for a in kv])
    return x, th / D, SHIFT


def project(v, n, op, mode, smin, smax):
    """(y, theta): the exact projection of the M-vector v (float64) and |theta*| of every entry's segment."""
    v = np.asarray(v)
    y = np.asarray(v, np.float64).copy()
    theta = np.zeros(len(y))
    for idx in segments(n, op, mode):
        y[idx], th, _ = exact_segment(v[idx], smin, smax)
        theta[idx] = abs(float(th))
    return y, theta


def sums(v, n, op, mode, TF):
    """(TF) sum of the positive parts of every segment, from the exact sum."""
    out = []
    for idx in segments(n, op, mode):
        k, D = _ints(list(np.asarray(v)[idx]) + [1.0])
        out.append(TF(Fraction(sum(a for a in k[:-1] if a > 0), D)))
    return np.array(out, TF)


def is_feasible(x, smin, smax):
    """Exactly: every entry >= 0 and the sum in [smin, smax]."""
    k, _ = _ints(list(x) + [smin, smax])
    return all(a >= 0 for a in k[:-2]) and k[-2] <= sum(k[:-2]) <= k[-1]


# ---- the header's arithmetic -----------------------------------------------------------------------------------------------------------------
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _add(acc, x):               # l21_sum_add
    s, e = _two_sum(acc[0], x)
    return (s, acc[1] + e)


def _fma(a, b, c):              # one rounding of a * b + c
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _theta(S, C, b):            # simplex_theta
    d, e = _two_sum(S[0], -b)
    q = d / C
    r = _fma(-q, C, d)
    return q + (r + (e + S[1])) / C


def emulate(v, smin, smax):
    """(case, theta_T, spos_T, steps, y) of simplex_project_serial on the finite TF vector v."""
    v = np.asarray(v)
    TF = v.dtype.type
    L = len(v)
    x = [float(a) for a in v]
    spos, sall, nneg = (0.0, 0.0), (0.0, 0.0), 0
    for a in x:
        sall = _add(sall, a)
        spos = _add(spos, 0.0 if a < 0 else a)
        nneg += a < 0
    sp = TF(spos[0] + spos[1])
    y = v.copy()
    if TF(smin) <= sp <= TF(smax):
        if nneg:
            y[v < 0] = 0.0
        return (CLIP if nneg else KEEP), TF(0), sp, 0, y
    b = float(TF(smax)) if sp > TF(smax) else float(TF(smin))
    theta, cprev, steps, done = _theta(sall, float(L), b), -1.0, 0, False
    while not done and steps <= L + 1:
        S, C = (0.0, 0.0), 0.0
        for a in x:
            if a > theta:
                S, C = _add(S, a), C + 1.0
        tn = _theta(S, C, b) if C > 0 else theta
        done = C == cprev or not C > 0
        theta = tn if tn > theta else theta
        cprev = C
        steps += 1
    th = TF(theta)
    t = (v - th).astype(TF)
    return SHIFT, th, sp, steps, np.where(t > 0, t, TF(0)).astype(TF)
