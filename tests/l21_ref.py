"""Reference of the l2,1 ball on the range of the TV operator (isotropic total variation; csrc/l21.h), pure numpy.

The M-vector is in the reference's row order: vcat(D_z[, D_y], D_x) (get_discrete_Grad.jl:31-33,69-72), the rows of a block in
column-major order of its own TD_n.  The group of grid point p holds the forward differences that start at p, one per direction in
which p has a successor, listed in block order (D_z first)."""
import functools

import numpy as np

from tests import l1_exact


def block_dirs(n):
    """Direction of every block of the M-vector, in its order: z (the last dimension) first, x last."""
    return list(range(len(n) - 1, -1, -1))


def groups(n):
    """int64 array (N, ndim): row p (column-major grid index) holds the M-vector indices of the members of p's group in block
    order, -1 where the block has no row for p (p on the far face along that direction).  Computed once per grid: read only."""
    G = _groups(tuple(int(k) for k in n))
    G.flags.writeable = False
    return G


@functools.lru_cache(maxsize=None)
def _groups(n):
    N = int(np.prod(n))
    coords = np.unravel_index(np.arange(N), n, order="F")
    out = np.full((N, len(n)), -1, np.int64)
    base = 0
    for q, d in enumerate(block_dirs(n)):
        tdn = list(n)
        tdn[d] -= 1
        has = coords[d] < n[d] - 1
        idx = np.ravel_multi_index(tuple(c[has] for c in coords), tuple(tdn), order="F")
        out[has, q] = base + idx
        base += int(np.prod(tdn))
    return out


def rows(n):
    n = tuple(int(k) for k in n)
    return sum(int(np.prod(n)) // n[d] * (n[d] - 1) for d in range(len(n)))


def sumsq(v, n):
    """The float64 sums of squares of the groups, added in block order."""
    G = groups(n)
    v64 = np.asarray(v, np.float64)
    assert v64.shape == (rows(n),)
    ss = np.zeros(G.shape[0], np.float64)
    for q in range(G.shape[1]):
        has = G[:, q] >= 0
        t = v64[G[has, q]]
        ss[has] = ss[has] + t * t
    return ss


def norms(v, n, TF):
    """g of the contract: sqrt of the float64 sum of squares, rounded once to TF."""
    return np.sqrt(sumsq(v, n)).astype(TF)


def norm21(v, n):
    """||v||_2,1 in extended precision from the float64 group norms."""
    return float(np.sum(np.sqrt(sumsq(v, n)).astype(l1_exact._WIDE)))


def project(v, n, b):
    """The projection of v onto { sum_p g_p <= b } in float64: theta is the exact l1 threshold of the TF group norms g (the array
    the engine searches), the weights max(g - theta, 0) / g come from the unrounded float64 norms.  v itself comes back when g lies
    inside the l1 ball away from rounding (l1_exact.feasibility)."""
    v = np.asarray(v)
    TF = v.dtype.type
    g = norms(v, n, TF)
    if l1_exact.feasibility(g, b) > 0:
        return v
    theta, _, _ = l1_exact.exact_theta(g.astype(np.float64), b)
    g64 = np.sqrt(sumsq(v, n))
    f = np.zeros_like(g64)
    pos = g64 > 0
    f[pos] = np.maximum(g64[pos] - theta, 0.0) / g64[pos]
    G = groups(n)
    y = np.zeros(v.shape, np.float64)
    for q in range(G.shape[1]):
        has = G[:, q] >= 0
        y[G[has, q]] = v[G[has, q]].astype(np.float64) * f[has]
    return y
