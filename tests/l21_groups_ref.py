"""Reference of the l2,1 ball over fibers or slices { v = A x : sum_s w_s ||v[segment s]||_2 <= tau } (csrc/l21_groups.h), pure numpy in
np.longdouble.  v is the M-vector of the range of A (identity, D_x, D_y, D_z) in the reference's row order: the array of shape TD_n in
column-major order.  Segments and their order come from tests/seg_norms_ref.segment_indices (the order of sipx.segment_norms), the exact
threshold, the feasibility margin and the emulation of the search from tests/l21_weighted_ref.py; the factors are taken from the
unrounded norms."""
import numpy as np

from tests import l1_exact, seg_norms_ref
from tests import l21_weighted_ref as R

W = l1_exact._WIDE


def td_n(n, op):
    """TD_n: the shape of the range of `op` on the grid n."""
    n = [int(v) for v in n]
    if op != "identity":
        n[{"D_x": 0, "D_y": 1, "D_z": len(n) - 1}[op]] -= 1
    return tuple(n)


def rows(n, op):
    return int(np.prod(td_n(n, op)))


def segments(n, op, mode):
    """One index array into the M-vector per segment, in the order of segment_norms()."""
    return seg_norms_ref.segment_indices(td_n(n, op), mode)


def nseg(n, op, mode):
    return len(segments(n, op, mode))


def exact_norms(v, n, op, mode):
    """The unrounded segment norms, in extended precision."""
    v = np.asarray(v).astype(W)
    return np.array([np.sqrt(np.sum(v[idx] * v[idx])) for idx in segments(n, op, mode)], W)


def norms(v, n, op, mode, TF):
    """g of the contract: the segment norms rounded once to TF."""
    return exact_norms(v, n, op, mode).astype(TF)


def ones(n, op, mode, TF):
    return np.ones(nseg(n, op, mode), TF)


def norm(v, n, op, mode, w=None):
    """sum_s w_s g_s of the TF segment norms (what the projector compares with tau), in extended precision."""
    v = np.asarray(v)
    g = norms(v, n, op, mode, v.dtype.type)
    w = ones(n, op, mode, v.dtype.type) if w is None else np.asarray(w)
    return float(np.sum(w.astype(W) * g.astype(W)))


def project(v, n, op, mode, w, tau):
    """The projection of v in float64: the exact theta of the TF segment norms, the factors max(g - theta w, 0) / g from the unrounded
    norms; segments of weight 0 keep their entries.  v itself comes back when `feasibility` says inside."""
    v = np.asarray(v)
    TF = v.dtype.type
    w = ones(n, op, mode, TF) if w is None else np.asarray(w)
    g = norms(v, n, op, mode, TF)
    if R.feasibility(g, w, tau) > 0:
        return v
    theta = W(R.exact_theta(g, w, tau))
    gx = exact_norms(v, n, op, mode)
    y = np.asarray(v, np.float64).copy()
    for s, idx in enumerate(segments(n, op, mode)):
        if not w[s] > 0:
            continue
        f = max(gx[s] - theta * W(w[s]), W(0)) / gx[s] if gx[s] > 0 else W(0)
        y[idx] = (v[idx].astype(W) * f).astype(np.float64)
    return y
