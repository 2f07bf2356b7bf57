"""Reference of the l2,0 sets on total variation { v = TV x : at most k grid points carry a non-zero gradient vector } (csrc/l20.h), pure
numpy.  v is the M-vector of the range of TV or TV_xy in the reference's row order; the groups and their membership come from
tests/l21_ref.py (op "TV"), tests/l21_frames_ref.py (op "TV_xy") and tests/l21_joint_ref.py (form "joint").

form "whole": one budget k over the N grid points, index = the column-major point index.
form "frames" (TV_xy): every z-slice has its own budget, k one integer or n3 of them, index = the in-frame pixel index.
form "joint"  (TV_xy): one budget over the n1 n2 pixels, a pixel's group spans the frames, index = the pixel index.

The projection keeps the k first groups of the stable descending order of the selection key g -- magnitude descending, ties to the lower
index -- bit for bit and writes +0 over every member of the others; with at most k non-zero keys (in a frame) it returns v (leaves the
frame) as it is.  The key is the contract's group norm, or an array the caller hands in (the device's own norms)."""
import numpy as np

from tests import l21_frames_ref, l21_joint_ref, l21_ref
from tests.card_groups_ref import gap, kept  # noqa: F401

FORMS = ("whole", "frames", "joint")


def rows(n, op):
    return l21_ref.rows(n) if op == "TV" else l21_frames_ref.rows(n)


def members(n, op):
    """int64 (N, nblk): the M-vector indices of the members of grid point p's group in block order, -1 where there is none."""
    return l21_ref.groups(n) if op == "TV" else l21_frames_ref.groups(n)


def ngroups(n, op, form):
    """Groups that compete for one budget: N, the n1 n2 pixels of a frame, or the n1 n2 pixels."""
    return int(np.prod(n)) if form == "whole" else int(n[0]) * int(n[1])


def norms(v, n, op, form, TF):
    """g of the contract in the order of sipx.tv_group_norms: N entries in point order (whole, frames), n1 n2 entries (joint)."""
    if form == "joint":
        return l21_joint_ref.norms(v, n, TF)
    return (l21_ref.norms(v, n, TF) if op == "TV" else l21_frames_ref.norms(v, n, TF).reshape(-1, order="F"))


def kept_points(g, n, op, form, k):
    """Boolean mask over the N grid points: does the group of point p stay?  g as norms() returns it."""
    g = np.asarray(g)
    N = int(np.prod(n))
    if form == "whole":
        return kept(g, k)
    L, n3 = int(n[0]) * int(n[1]), int(n[2])
    if form == "joint":
        return np.tile(kept(g, k), n3)
    ks = np.broadcast_to(np.asarray(k), (n3,))
    return np.concatenate([kept(g[f * L:(f + 1) * L], int(ks[f])) for f in range(n3)]) if N else np.ones(0, bool)


def project(v, n, op, form, k, g=None):
    """The projection of v (same dtype); v itself when nothing is dropped.  g: the selection key, default norms(v)."""
    v = np.asarray(v)
    assert form in FORMS and (op == "TV_xy" or form == "whole")
    g = norms(v, n, op, form, v.dtype.type) if g is None else np.asarray(g)
    keep = kept_points(g, n, op, form, k)
    if keep.all():
        return v
    M = members(n, op)[~keep]
    y = v.copy()
    y[M[M >= 0]] = 0
    return y


def brute_force(v, n, op, form, k):
    """The same projection from the definition, group by group, without argsort: group p stays iff fewer than k groups come before it
    in the order (key descending, index ascending) -- or nothing is dropped at all.  For tiny grids."""
    v = np.asarray(v)
    G = members(n, op)
    N, L = G.shape[0], int(n[0]) * int(n[1])
    key = np.zeros(N)
    for p in range(N):
        key[p] = np.sqrt(sum(float(v[i]) ** 2 for i in G[p] if i >= 0))
    key = key.astype(v.dtype)
    if form == "joint":
        ss = np.zeros(L)
        for p in range(N):
            ss[p % L] += sum(float(v[i]) ** 2 for i in G[p] if i >= 0)
        key = np.sqrt(ss).astype(v.dtype)
    y = v.copy()
    pools = [range(N)] if form == "whole" else ([range(L)] if form == "joint" else [range(f * L, (f + 1) * L) for f in range(int(n[2]))])
    ks = np.broadcast_to(np.asarray(k), (len(pools),))
    for pool, kk in zip(pools, ks):
        pool = list(pool)
        if sum(1 for p in pool if key[p] > 0) <= kk:
            continue
        for a, p in enumerate(pool):
            before = sum(1 for b, q in enumerate(pool) if key[q] > key[p] or (key[q] == key[p] and b < a))
            if before >= kk:
                pts = [p] if form != "joint" else [p + f * L for f in range(int(n[2]))]
                for t in pts:
                    for i in G[t]:
                        if i >= 0:
                            y[i] = 0
    return y
