"""Reference of the l2,1 ball on the range of TV_xy = vcat(D_y, D_x), the in-plane gradient of a 3-D grid, for the whole array and
per z-slice (csrc/l21_seg.h), pure numpy, in the manner of tests/l21_ref.py.

The M-vector holds the rows of D_y first, column-major over (n1, n2 - 1, n3), then the rows of D_x over (n1 - 1, n2, n3).  The group
of grid point p = (i, j, k) holds the D_y difference that starts at p (j < n2 - 1) and the D_x difference (i < n1 - 1), in that
order; the last corner of every frame has none.  Frame k is the n1 n2 points (., ., k)."""
import functools

import numpy as np

from tests import l1_exact

BLOCK_DIRS = (1, 0)


def groups(n):
    """int64 array (N, 2): row p (column-major grid index) holds the M-vector indices of the members of p's group in block order
    (D_y, D_x), -1 where the block has no row for p.  Computed once per grid: read only."""
    G = _groups(tuple(int(k) for k in n))
    G.flags.writeable = False
    return G


@functools.lru_cache(maxsize=None)
def _groups(n):
    assert len(n) == 3
    N = int(np.prod(n))
    coords = np.unravel_index(np.arange(N), n, order="F")
    out = np.full((N, 2), -1, np.int64)
    base = 0
    for q, d in enumerate(BLOCK_DIRS):
        tdn = list(n)
        tdn[d] -= 1
        has = coords[d] < n[d] - 1
        out[has, q] = base + np.ravel_multi_index(tuple(c[has] for c in coords), tuple(tdn), order="F")
        base += int(np.prod(tdn))
    return out


def rows(n):
    n1, n2, n3 = (int(k) for k in n)
    return n1 * (n2 - 1) * n3 + (n1 - 1) * n2 * n3


def sumsq(v, n):
    """The float64 sums of squares of the groups, added in block order."""
    G = groups(n)
    v64 = np.asarray(v, np.float64)
    assert v64.shape == (rows(n),)
    ss = np.zeros(G.shape[0], np.float64)
    for q in range(2):
        has = G[:, q] >= 0
        t = v64[G[has, q]]
        ss[has] = ss[has] + t * t
    return ss


def norms(v, n, TF):
    """g of the contract: sqrt of the float64 sum of squares, rounded once to TF; (n1 n2, n3), one column per frame."""
    return np.sqrt(sumsq(v, n)).astype(TF).reshape(int(n[0]) * int(n[1]), int(n[2]), order="F")


def frame_norms(v, n, TF=None):
    """The n3 per-frame norms in extended precision: from the float64 group norms, or (TF given) from the TF-rounded ones, the
    values the engine sums."""
    g = np.sqrt(sumsq(v, n)) if TF is None else norms(v, n, TF).reshape(-1, order="F")
    g = g.reshape(int(n[0]) * int(n[1]), int(n[2]), order="F")
    return np.array([float(np.sum(g[:, k].astype(l1_exact._WIDE))) for k in range(g.shape[1])])


def norm21(v, n):
    return float(np.sum(frame_norms(v, n).astype(l1_exact._WIDE)))


def _scale(v, n, f):
    """y = v with every member of group p multiplied by f[p] (float64); groups with f[p] = nan keep their entries."""
    G = groups(n)
    y = np.asarray(v, np.float64).copy()
    keep = np.isnan(f)
    for q in range(2):
        has = (G[:, q] >= 0) & ~keep
        y[G[has, q]] = y[G[has, q]] * f[has]
    return y


def _weights(g64, theta):
    f = np.zeros_like(g64)
    pos = g64 > 0
    f[pos] = np.maximum(g64[pos] - theta, 0.0) / g64[pos]
    return f


def project(v, n, b):
    """The projection of v onto { sum_{p in frame k} g_p <= b_k for every k } in float64; b a scalar or n3 radii.  Per frame theta is
    the exact l1 threshold of the TF group norms, the weights max(g - theta, 0) / g come from the unrounded float64 norms.  A frame
    inside its ball away from rounding (l1_exact.feasibility) keeps its entries; v itself comes back when every frame is."""
    v = np.asarray(v)
    TF = v.dtype.type
    n3 = int(n[2])
    b = np.broadcast_to(np.asarray(b, TF), (n3,))
    g = norms(v, n, TF)
    g64 = np.sqrt(sumsq(v, n)).reshape(g.shape, order="F")
    f = np.full(g.shape, np.nan)
    for k in range(n3):
        if l1_exact.feasibility(g[:, k], b[k]) > 0:
            continue
        theta, _, _ = l1_exact.exact_theta(g[:, k].astype(np.float64), b[k])
        f[:, k] = _weights(g64[:, k], theta)
    if np.isnan(f).all():
        return v
    return _scale(v, n, f.reshape(-1, order="F"))


def inside(v, n, b):
    """Per frame: l1_exact.feasibility of its TF group norms against its radius (+1 inside, -1 outside, 0 too close to call)."""
    v = np.asarray(v)
    TF = v.dtype.type
    b = np.broadcast_to(np.asarray(b, TF), (int(n[2]),))
    g = norms(v, n, TF)
    return np.array([l1_exact.feasibility(g[:, k], b[k]) for k in range(g.shape[1])])


def frame_rows(n, k):
    """M-vector indices of the members of the groups of frame k."""
    G = groups(n).reshape(int(n[0]) * int(n[1]), int(n[2]), 2, order="F")[:, k, :]
    return np.sort(G[G >= 0])


def project_whole(v, n, b):
    """The same with one group set that spans all frames: the whole-array ("l21", "TV_xy") in tensor mode."""
    v = np.asarray(v)
    TF = v.dtype.type
    g = norms(v, n, TF).reshape(-1, order="F")
    if l1_exact.feasibility(g, b) > 0:
        return v
    theta, _, _ = l1_exact.exact_theta(g.astype(np.float64), b)
    return _scale(v, n, _weights(np.sqrt(sumsq(v, n)), theta))
