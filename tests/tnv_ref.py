"""Reference of total nuclear variation, the nuclear-norm ball on the 2 x n3 Jacobians of the pixels on the range of TV_xy = vcat(D_y, D_x)
(csrc/tnv.h), pure numpy, built on tests/l21_joint_ref.py's members and plan and on tests/l1_exact.py.

Two things live here.  `gram` / `svals` follow the contract of csrc/tnv.h step by step -- its order of additions, its chunks, for Float64
its sums and its a b - c^2 in twice the working precision (the fma errors reproduced by Dekker's exact product) -- and give the rounded
singular values s the engine's search runs on.  `exact_svd` does not follow the contract: it diagonalises every J_p by one-sided Jacobi
rotations of its two rows in extended precision, and `project` takes its factors and rotation from there.  The code under test is never the
reference."""
import math

import numpy as np

from tests import l1_exact
from tests.l21_joint_ref import _members, plan, rows  # noqa: F401

# The bound of the tests, in eps(TF) ||J_p||_F per member of pixel p: max(4, 2 x the worst error of the CPU rule (tests/test_tnv_cpu.py,
# test_rule_meets_the_reference_within_the_bound prints it) rounded up to an integer).  Measured on the CPU rule over all grids, radii and
# both precisions of tests/test_gpu_tnv.py: Float32 1.54, Float64 2.84.
BOUND = {np.float32: 4, np.float64: 6}
MEASURED = {np.float32: 1.54, np.float64: 2.84}


def jacobians(v, n, dtype=np.float64):
    """(L, 2, n3): J_p, row 0 the D_y members of pixel p over the frames, row 1 the D_x members; a missing block is a row of zeros."""
    G = _members(n)
    vv = np.asarray(v).astype(dtype)
    assert vv.shape == (rows(n),)
    J = np.zeros((G.shape[0], 2, G.shape[1]), dtype)
    for q in range(2):
        has = G[:, :, q] >= 0
        J[:, q, :][has] = vv[G[:, :, q][has]]
    return J


def scatter(Y, n):
    """The M-vector of the (L, 2, n3) array Y: the inverse of `jacobians` on the existing members."""
    G = _members(n)
    out = np.zeros(rows(n), Y.dtype)
    for q in range(2):
        has = G[:, :, q] >= 0
        out[G[:, :, q][has]] = Y[:, q, :][has]
    return out


# ---- the contract's sums -------------------------------------------------------------------------------------------------------------
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(x, y):
    """(p, e): p = fl(x y) and e = x y - p exactly (Dekker / Veltkamp): the value fma(x, y, -p) returns."""
    p = x * y
    c = 134217729.0
    xh = c * x - (c * x - x)
    xl = x - xh
    yh = c * y - (c * y - y)
    yl = y - yh
    return p, ((xh * yh - p) + xh * yl + xl * yh) + xl * yl


class _Sum:
    """L21Sum of csrc/l21.h on arrays: hi + lo, the low word keeps the rounding errors."""

    def __init__(self, L):
        self.hi, self.lo = np.zeros(L), np.zeros(L)

    def add_product(self, x, y, wide):
        p, e = _two_prod(x, y) if wide else (x * y, 0.0)
        if wide:
            s, err = _two_sum(self.hi, p)
            self.hi, self.lo = s, (self.lo + err) + e
        else:
            self.hi = self.hi + p

    def merge(self, o, wide):
        if wide:
            s, err = _two_sum(self.hi, o.hi)
            self.hi, self.lo = s, self.lo + (err + o.lo)
        else:
            self.hi = self.hi + o.hi


def gram(v, n, TF):
    """(a, b, c), each a _Sum over the L pixels, in the contract's order: chunks of the plan from zero, frames ascending, the chunk sums
    merged in ascending order from zero.  Float32: plain float64 sums (lo stays 0); Float64: the pairs of csrc/tnv.h."""
    J = jacobians(v, n)
    L, n3 = J.shape[0], J.shape[2]
    wide = np.dtype(TF).itemsize == 8
    nchunk, zc = plan(L, n3, np.dtype(TF).itemsize)
    tot = [_Sum(L) for _ in range(3)]
    for c in range(nchunk):
        part = [_Sum(L) for _ in range(3)]
        for k in range(c * zc, min((c + 1) * zc, n3)):
            y, x = J[:, 0, k], J[:, 1, k]
            part[0].add_product(y, y, wide)
            part[1].add_product(x, x, wide)
            part[2].add_product(y, x, wide)
        for t, p in zip(tot, part):
            t.merge(p, wide)
    return tot


def decompose(v, n, TF):
    """(s1, s2, cs, sn) of the contract, each L entries of TF."""
    A, B, C = gram(v, n, TF)
    wide = np.dtype(TF).itemsize == 8
    a, b, c = A.hi + A.lo, B.hi + B.lo, C.hi + C.lo
    d = 0.5 * (a - b)
    r = np.hypot(d, c)
    l1 = 0.5 * (a + b) + r
    safe = np.where(l1 > 0, l1, 1.0)
    if wide:
        ah, al = _two_sum(A.hi, A.lo)
        bh, bl = _two_sum(B.hi, B.lo)
        ch, cl = _two_sum(C.hi, C.lo)
        p, pe = _two_prod(ah, bh)
        pe = pe + (ah * bl + al * bh)
        q, qe = _two_prod(ch, ch)
        qe = qe + 2.0 * (ch * cl)
        s, se = _two_sum(p, -q)
        dh, dl = _two_sum(s, se + (pe - qe))
        q1 = dh / safe
        t, te = _two_prod(q1, safe)
        l2 = q1 + (((dh - t) - te) + dl) / safe      # (dh - t is exact: fma(-q1, l1, dh) rounds (dh - t) - te once)
        l2 = np.where(dh > 0, l2, 0.0)
    else:
        det = a * b - c * c
        l2 = np.where(det > 0, det, 0.0) / safe
    l2 = np.where(l1 > 0, l2, 0.0)
    x = np.where(d >= 0, d + r, c)
    y = np.where(d >= 0, c, r - d)
    nn = np.hypot(x, y)
    ok = nn > 0
    nn = np.where(ok, nn, 1.0)
    cs = np.where(ok, x / nn, 1.0).astype(TF)
    sn = np.where(ok, y / nn, 0.0).astype(TF)
    return np.sqrt(l1).astype(TF), np.sqrt(l2).astype(TF), cs, sn


def svals(v, n, TF):
    """The contract's rounded s = [sigma1 of all pixels; sigma2 of all pixels], 2 L entries of TF."""
    s1, s2, _, _ = decompose(v, n, TF)
    return np.concatenate([s1, s2])


# ---- the reference proper ------------------------------------------------------------------------------------------------------------
def exact_svd(v, n):
    """(s1, s2, U, R) in extended precision (l1_exact._WIDE): R = U J has orthogonal rows with |R_0| = s1 >= |R_1| = s2, U (L, 2, 2)
    orthogonal.  One-sided Jacobi rotations of the two rows, six sweeps (the second already leaves the rows orthogonal to the precision
    of the type).  Where the platform has no wider type: float64 with math.fsum for the row norms."""
    W = l1_exact._WIDE
    R = jacobians(v, n, W)
    L = R.shape[0]
    U = np.zeros((L, 2, 2), W)
    U[:, 0, 0] = U[:, 1, 1] = 1
    for _ in range(6):
        a, b, g = (R[:, 0] ** 2).sum(1), (R[:, 1] ** 2).sum(1), (R[:, 0] * R[:, 1]).sum(1)
        d = (a - b) / 2
        r = np.hypot(d, g)
        x, y = np.where(d >= 0, d + r, g), np.where(d >= 0, g, r - d)
        nn = np.hypot(x, y)
        z = nn == 0
        nn = np.where(z, 1, nn)
        cs, sn = np.where(z, 1, x / nn), np.where(z, 0, y / nn)
        R = np.stack([cs[:, None] * R[:, 0] + sn[:, None] * R[:, 1], -sn[:, None] * R[:, 0] + cs[:, None] * R[:, 1]], 1)
        Q = np.zeros((L, 2, 2), W)
        Q[:, 0, 0], Q[:, 0, 1], Q[:, 1, 0], Q[:, 1, 1] = cs, sn, -sn, cs
        U = np.einsum("lij,ljk->lik", Q, U)
    if np.finfo(W).eps >= np.finfo(np.float64).eps:
        s1 = np.array([math.sqrt(math.fsum((R[p, 0] ** 2).tolist())) for p in range(L)])
        s2 = np.array([math.sqrt(math.fsum((R[p, 1] ** 2).tolist())) for p in range(L)])
    else:
        s1, s2 = np.sqrt((R[:, 0] ** 2).sum(1)), np.sqrt((R[:, 1] ** 2).sum(1))
    return s1, s2, U, R


def norm(v, n):
    """sum over the pixels of ||J_p||_*, in extended precision."""
    s1, s2, _, _ = exact_svd(v, n)
    return float(np.sum(s1) + np.sum(s2))


def frob(v, n):
    """||J_p||_F per pixel, float64: the scale of the error bound."""
    return np.sqrt((jacobians(v, n, l1_exact._WIDE) ** 2).sum((1, 2))).astype(np.float64)


def prepare(v, n):
    """What `inside` and `project` need of v whatever the radius, for callers that ask at several radii: (svals, exact_svd)."""
    v = np.asarray(v)
    return svals(v, n, v.dtype.type), exact_svd(v, n)


def inside(v, n, tau, pre=None):
    """l1_exact.feasibility of the contract's TF singular values against tau: +1 inside, -1 outside, 0 too close to call."""
    v = np.asarray(v)
    return l1_exact.feasibility(pre[0] if pre else svals(v, n, v.dtype.type), tau)


def project(v, n, tau, pre=None):
    """The projection of v onto { sum_p ||J_p||_* <= tau } in float64: the exact l1 threshold of the TF-rounded s of the contract, the
    factors max(sigma - theta, 0) / sigma and the rotation from the unrounded decomposition.  v itself comes back when
    l1_exact.feasibility says inside.  pre: prepare(v, n), computed once."""
    v = np.asarray(v)
    s = pre[0] if pre else svals(v, n, v.dtype.type)
    if l1_exact.feasibility(s, tau) > 0:
        return v
    theta, _, _ = l1_exact.exact_theta(s.astype(np.float64), tau)
    W = l1_exact._WIDE
    s1, s2, U, R = pre[1] if pre else exact_svd(v, n)
    th = W(theta)
    f1 = np.where(s1 > 0, np.maximum(s1 - th, 0) / np.where(s1 > 0, s1, 1), 0)
    f2 = np.where(s2 > 0, np.maximum(s2 - th, 0) / np.where(s2 > 0, s2, 1), 0)
    Rn = np.stack([f1[:, None] * R[:, 0], f2[:, None] * R[:, 1]], 1)
    return scatter(np.einsum("lji,ljk->lik", U, Rn), n).astype(np.float64)


def error(y, ref, v, n):
    """The metric of the tests: the worst |y - ref| / ||J_p||_F over the members of pixel p, per pixel (L entries; in units of 1, divide
    by eps); pixels with J_p = 0 must come back zero and report 0 (inf otherwise)."""
    E = np.abs(jacobians(np.asarray(y, np.float64) - np.asarray(ref, np.float64), n)).max((1, 2))
    fn = frob(v, n)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(fn > 0, E / np.where(fn > 0, fn, 1.0), np.where(E > 0, np.inf, 0.0))
