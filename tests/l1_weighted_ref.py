"""Reference of the weighted l1 ball { v : sum_i w_i |v_i| <= tau } on the rows of an operator (csrc/l1_weighted.h), pure numpy.

The search of the header is the rule of csrc/l21_weighted.h on the pairs (|v|, w): `exact_theta`, `feasibility`, `emulate_search` and
`clean` of tests/l21_weighted_ref.py are its reference and its emulation too, and are used from there.  What is new here: the rows of
the operators and where they lie in the padded layout, the threshold of a LARGE vector (`theta_star`: a running sum in np.longdouble
is good to n 2^-64 only, far from "well under eps" at 10^6 Float64 entries), the projection itself, and the emulation of the apply."""
import math
from fractions import Fraction

import numpy as np

from tests.l21_weighted_ref import W, clean, emulate_search, exact_theta, feasibility      # noqa: F401  (re-exported)

OPS = ("identity", "D_x", "D_y", "D_z", "TV", "TV_xy")


def block_dirs(n, op):
    """The difference directions of the operator's blocks in the reference's block order (get_discrete_Grad.jl: vcat(D_z[, D_y], D_x))."""
    nd = len(n)
    if op == "identity":
        return []
    if op == "D_y" and nd == 2:
        raise ValueError("D_y needs a 3-D grid")
    if op == "TV_xy":
        if nd != 3:
            raise ValueError("TV_xy needs a 3-D grid")
        return [1, 0]
    if op in ("TV", "D2D", "D3D"):
        return [1, 0] if nd == 2 else [2, 1, 0]
    return [{"D_x": 0, "D_y": 1, "D_z": nd - 1}[op]]


def rows(n, op):
    """Mtrue: the rows of the operator, the entries of A @ x, y_i, l_i and of the weights."""
    N = int(np.prod(n))
    d = block_dirs(n, op)
    return N if not d else sum(N // n[a] * (n[a] - 1) for a in d)


def members(n, op):
    """(Mtrue,) int64: where row r lies in the padded layout -- max(nblk, 1) full grids side by side, block q at q N, the rows of a block
    column-major over its own extents.  Every padded entry that is not listed is a pad (weight 0 on the device)."""
    N = int(np.prod(n))
    d = block_dirs(n, op)
    if not d:
        return np.arange(N, dtype=np.int64)
    full = np.arange(N, dtype=np.int64).reshape(n, order="F")
    out = []
    for q, a in enumerate(d):
        sl = [slice(None)] * len(n)
        sl[a] = slice(0, n[a] - 1)
        out.append(q * N + full[tuple(sl)].reshape(-1, order="F"))
    return np.concatenate(out)


def norm(v, w):
    """sum_i w_i |v_i| in extended precision."""
    return float(np.sum(np.asarray(w).astype(W) * np.abs(np.asarray(v)).astype(W)))


# ---- the threshold of a large vector -------------------------------------------------------------------------------------------------
def _two_prod(x, y):
    """x * y = p + e exactly (Dekker's product on Veltkamp's split), float64 arrays."""
    p = x * y
    c = 134217729.0
    t = c * x
    xh = t - (t - x)
    xl = x - xh
    t = c * y
    yh = t - (t - y)
    yl = y - yh
    e = ((xh * yh - p) + xh * yl + xl * yh) + xl * yl
    return p, e


def _fsum_products(x, y):
    """sum x_i y_i as a Fraction good to 2^-105: math.fsum rounds the exact sum of the error-free products once; the same sum with that
    value taken away gives what the rounding lost, rounded once."""
    p, e = _two_prod(x, y)
    terms = np.concatenate([p, e]).tolist()
    hi = math.fsum(terms)
    return Fraction(hi) + Fraction(math.fsum(terms + [-hi]))


def theta_star(a, w, tau):
    return theta_star_parts(a, w, tau)[0]


def theta_star_parts(a, w, tau):
    """(theta*, S, C) of the weighted ball on the TF numbers a >= 0 with TF weights w >= 0 as Fractions ((0, S_all, 0) inside): the prefix
    of the sorted breakpoints a / w is CHOSEN from cumulative sums in np.longdouble, its defining condition is CHECKED (and the prefix
    moved where the running sums misplaced it), and its S = sum w a, C = sum w^2 are EVALUATED with math.fsum over error-free products,
    with the quotient formed in Fraction."""
    a64, w64 = np.asarray(a, np.float64), np.asarray(clean(np.asarray(w)), np.float64)
    tau_f = Fraction(float(tau))
    S_all = _fsum_products(w64, a64)
    if S_all <= tau_f:
        return Fraction(0), S_all, Fraction(0)
    pos = (w64 > 0) & (a64 > 0)
    ap, wp = a64[pos], w64[pos]
    r = ap.astype(W) / wp.astype(W)
    order = np.argsort(-r, kind="stable")
    ap, wp, r = ap[order], wp[order], r[order]
    S, C = np.cumsum(wp.astype(W) * ap.astype(W)), np.cumsum(wp.astype(W) * wp.astype(W))
    th = (S - W(float(tau))) / C
    ok = np.nonzero(r > th)[0]
    k = int(ok[-1]) if len(ok) else 0

    def theta_of(k):
        Sk, Ck = _fsum_products(wp[:k + 1], ap[:k + 1]), _fsum_products(wp[:k + 1], wp[:k + 1])
        return (Sk - tau_f) / Ck, Sk, Ck
    theta, Sk, Ck = theta_of(k)
    for _ in range(64):            # the prefix condition: its last breakpoint lies above theta, the next one does not
        if k + 1 < len(ap) and Fraction(float(ap[k + 1])) > theta * Fraction(float(wp[k + 1])):
            k += 1
        elif k > 0 and not Fraction(float(ap[k])) > theta * Fraction(float(wp[k])):
            k -= 1
        else:
            break
        theta, Sk, Ck = theta_of(k)
    else:
        raise AssertionError("theta_star: the prefix did not settle")
    return max(theta, Fraction(0)), Sk, Ck


def _wide_of(fr):
    """A Fraction in extended precision: its float64 rounding plus the float64 rounding of what is left."""
    hi = float(fr)
    return W(hi) + W(float(fr - Fraction(hi)))


def project(v, w, tau):
    """The projection of v onto { sum_i w_i |v_i| <= tau }: theta* of the TF arrays (|v|, w), y = sign(v) max(|v| - theta* w, 0); rows of
    weight 0 keep their entries.  v itself comes back when `feasibility` says inside.  The result is float64 for Float32 input and
    np.longdouble for Float64 input (a float64 product and difference would carry as much rounding as the code under test)."""
    v = np.asarray(v)
    TF = v.dtype.type
    a = np.abs(v)
    wc = clean(np.asarray(w, TF))
    if feasibility(a, wc, tau) > 0:
        return v
    theta = _wide_of(theta_star(a, wc, TF(tau)))
    out = np.float64 if TF == np.float32 else W
    t = np.maximum(a.astype(W) - theta * wc.astype(W), W(0))
    y = np.where(wc > 0, np.copysign(t, v.astype(W)), v.astype(W))
    return y.astype(out)


# ---- the apply of csrc/l1_weighted.h in TF arithmetic -------------------------------------------------------------------------------------
def emulate_apply(v, w, theta):
    """l1w_shrink on every entry whose cleaned weight is > 0, in TF, bit for bit; the others keep their bits."""
    v = np.asarray(v)
    TF = v.dtype.type
    wc = clean(np.asarray(w, TF))
    with np.errstate(invalid="ignore", over="ignore"):
        p = (TF(theta) * wc).astype(TF)
        t = (np.abs(v) - p).astype(TF)
        y = np.where(t > 0, np.copysign(t, v), np.copysign(TF(0), v)).astype(TF)
    return np.where(wc > 0, y, v).astype(TF)


def emulate_project(v, w, tau):
    """(need, theta, (TF)asum, passes, y) of l1w_project_serial for FINITE v: the search of l21w_search_serial on (|v|, w), the apply."""
    v = np.asarray(v)
    need, theta, asum, passes = emulate_search(np.abs(v), np.asarray(w, v.dtype), tau)
    return need, theta, asum, passes, (emulate_apply(v, w, theta) if need else v.copy())
