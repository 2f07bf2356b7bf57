"""Reference of the l2,inf ball -- every group norm at most c_p (csrc/l2inf.h) -- pure numpy, for the three layouts of its groups.

A layout is an int64 array `idx` of shape (groups, m): row p holds the indices into the M-vector of the members of group p in the
order the contract adds their squares, -1 where there is none.  TV / TV_xy: the M-vector in the reference's row order, the groups of
tests/l21_ref.py / tests/l21_frames_ref.py (one per grid point).  Joint: the groups of tests/l21_joint_ref.py (one per pixel, frames
ascending and within a frame D_y then D_x).  Stacked: B blocks of G entries, group p = { v[q G + p] }.
Group norms in float64; the decision g_p > c_p is taken on the norms rounded to the working precision, as the contract takes it; the
factor c_p / g_p is exact float64 arithmetic on the unrounded norm."""
import numpy as np

from tests import l21_frames_ref, l21_joint_ref, l21_ref


def layout_tv(n):
    return l21_ref.groups(n)


def layout_tv_xy(n):
    return l21_frames_ref.groups(n)


def layout_joint(n):
    G = l21_joint_ref._members(n)
    return np.ascontiguousarray(G.reshape(G.shape[0], -1))


def layout_stacked(M, B):
    assert M % B == 0
    return np.ascontiguousarray(np.arange(M, dtype=np.int64).reshape(B, M // B).T)


def sumsq(v, idx):
    """The float64 sums of squares of the groups, members added in the order of the layout."""
    v64 = np.asarray(v, np.float64)
    ss = np.zeros(idx.shape[0], np.float64)
    for q in range(idx.shape[1]):
        has = idx[:, q] >= 0
        t = v64[idx[has, q]]
        ss[has] = ss[has] + t * t
    return ss


def norms(v, idx, TF, joint_n=None):
    """g of the contract in TF.  joint_n: the grid of the joint set, whose sum of squares follows the chunk plan of l21_joint.h."""
    if joint_n is not None:
        return l21_joint_ref.norms(v, joint_n, TF)
    return np.sqrt(sumsq(v, idx)).astype(TF)


def max_norm(v, idx, TF, joint_n=None):
    g = norms(v, idx, TF, joint_n)
    return TF(g.max()) if g.size else TF(0)


def bounds(c, groups, TF):
    """c as one TF bound per group."""
    c = np.asarray(c, TF)
    return np.full(groups, c, TF) if c.ndim == 0 else c


def project(v, idx, c, joint_n=None):
    """The projection of v onto { g_p <= c_p } in float64; v itself when no group is clipped."""
    v = np.asarray(v)
    TF = v.dtype.type
    g = norms(v, idx, TF, joint_n)
    cv = bounds(c, idx.shape[0], TF)
    clip = g > cv
    if not clip.any():
        return v
    g64 = np.sqrt(sumsq(v, idx))
    f = np.ones(idx.shape[0], np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        f[clip] = cv[clip].astype(np.float64) / g64[clip]
    y = v.astype(np.float64)
    for q in range(idx.shape[1]):
        has = (idx[:, q] >= 0) & clip
        y[idx[has, q]] = y[idx[has, q]] * f[has]
    return y


def excess_units(TF, m):
    """l2inf_excess_units of csrc/l2inf.h: what the observed norm of a projected group of m members may exceed c by, in units of
    (eps / 2) c."""
    kg = 1.0 + m / 268435456.0 if np.dtype(TF).itemsize == 4 else 1.0 + 0.5 * m
    return 2.0 * kg + 2.0 + 0.01
