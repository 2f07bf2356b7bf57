"""Reference of the joint (vectorial) l2,1 ball across frames on the range of TV_xy = vcat(D_y, D_x) (csrc/l21_joint.h), pure numpy,
built on tests/l21_frames_ref.py's groups / rows and tests/l1_exact.py.

The group of pixel (i, j) holds, for every frame k, the D_y difference that starts at (i, j, k) if j < n2 - 1 and the D_x difference if
i < n1 - 1: 0 to 2 n3 members, the last corner pixel has none.  Pixel p = i + n1 j of frame k is grid point p + k n1 n2."""
import math

import numpy as np

from tests import l1_exact
from tests.l21_frames_ref import groups, rows  # noqa: F401

FILL_THREADS, MIN_CHUNK = 131072, 8           # csrc/l21_joint.h: L21J_FILL_THREADS, L21J_MIN_CHUNK


def plan(L, n3, elem_bytes):
    """(nchunk, zc) of l21_joint_plan: chunk c covers the frames [c zc, min((c + 1) zc, n3))."""
    threads = max(L * elem_bytes // 16, 1)
    nc = max(min(-(-FILL_THREADS // threads), n3 // MIN_CHUNK), 1)
    zc = max(-(-n3 // nc), 1)
    return max(-(-n3 // zc), 1), zc


def _members(n):
    """(L, n3, 2) int64: the M-vector indices of pixel p's members in frame k, block order (D_y, D_x), -1 where there is none."""
    return groups(n).reshape(int(n[0]) * int(n[1]), int(n[2]), 2, order="F")


def sumsq(v, n, TF):
    """The contract's float64 sums of squares: per chunk of the plan from 0.0, frames ascending and D_y then D_x, the chunk sums
    added in ascending order from 0.0."""
    G = _members(n)
    v64 = np.asarray(v, np.float64)
    assert v64.shape == (rows(n),)
    L, n3 = G.shape[0], G.shape[1]
    nchunk, zc = plan(L, n3, np.dtype(TF).itemsize)
    ss = np.zeros(L, np.float64)
    for c in range(nchunk):
        sc = np.zeros(L, np.float64)
        for k in range(c * zc, min((c + 1) * zc, n3)):
            for q in range(2):
                has = G[:, k, q] >= 0
                t = v64[G[has, k, q]]
                sc[has] = sc[has] + t * t
        ss = ss + sc
    return ss


def norms(v, n, TF):
    """g of the contract, given the plan's chunking: sqrt of the float64 sum of squares, rounded once to TF; L entries."""
    return np.sqrt(sumsq(v, n, TF)).astype(TF)


def exact_norms(v, n):
    """The unrounded group norms in float64: sums of squares and the root in extended precision (l1_exact._WIDE), rounded once --
    math.fsum per pixel where the platform has no wider type."""
    G = _members(n)
    W = l1_exact._WIDE
    if np.finfo(W).eps >= np.finfo(np.float64).eps:
        v64 = np.asarray(v, np.float64)
        return np.array([math.sqrt(math.fsum((v64[G[p][G[p] >= 0]] ** 2).tolist())) for p in range(G.shape[0])])
    vw = np.asarray(v).astype(W)
    ss = np.zeros(G.shape[0], W)
    for k in range(G.shape[1]):
        for q in range(2):
            has = G[:, k, q] >= 0
            t = vw[G[has, k, q]]
            ss[has] = ss[has] + t * t
    return np.sqrt(ss).astype(np.float64)


def norm21(v, n):
    """sum over the pixels of the float64 group norms, in extended precision."""
    return float(np.sum(exact_norms(v, n).astype(l1_exact._WIDE)))


def inside(v, n, tau):
    """l1_exact.feasibility of the TF group norms against tau: +1 inside, -1 outside, 0 too close to call."""
    v = np.asarray(v)
    return l1_exact.feasibility(norms(v, n, v.dtype.type), tau)


def project(v, n, tau):
    """The projection of v onto { sum_p g_p <= tau } in float64: the exact l1 threshold of the TF group norms, the weights
    max(g - theta, 0) / g from the unrounded float64 norms.  v itself comes back when l1_exact.feasibility says inside."""
    v = np.asarray(v)
    TF = v.dtype.type
    g = norms(v, n, TF)
    if l1_exact.feasibility(g, tau) > 0:
        return v
    theta, _, _ = l1_exact.exact_theta(g.astype(np.float64), tau)
    g64 = exact_norms(v, n)
    f = np.zeros_like(g64)
    pos = g64 > 0
    f[pos] = np.maximum(g64[pos] - theta, 0.0) / g64[pos]
    G = _members(n)
    y = np.asarray(v, np.float64).copy()
    for q in range(2):
        for k in range(G.shape[1]):
            has = G[:, k, q] >= 0
            y[G[has, k, q]] = y[G[has, k, q]] * f[has]
    return y
