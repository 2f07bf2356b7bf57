"""Reference of the per-fiber / per-slice norm sets with one radius per segment (pure numpy, no GPU): the oracle's whole-vector
projector applied to every segment with that segment's own scalars.  Segments, their order and the order of their elements are those
of tests/seg_norms_ref.segment_indices (SegMap, csrc/ext_family.h): radius s belongs to segment s."""
import numpy as np

from oracle import parsdmm_oracle as O
from tests import seg_norms_ref


def nseg(TD_n, mode):
    return len(seg_norms_ref.segment_indices(TD_n, mode))


def project_segments(v, TD_n, mode, st, rmin, rmax):
    """v <- the projection of every fiber / slice onto its own l1 ball / l2 ball / annulus (in place, and returned).  rmin, rmax:
    one number of v's type per segment (rmin is read by the annulus only)."""
    segs = seg_norms_ref.segment_indices(TD_n, mode)
    assert len(rmax) == len(segs) and (st != "annulus" or len(rmin) == len(segs))
    for s, ind in enumerate(segs):
        x = np.ascontiguousarray(v[ind])
        if st == "l1":
            v[ind] = O.project_l1_Duchi(x, rmax[s])
        elif st == "l2":
            v[ind] = O.project_l2(x, rmax[s])
        elif st == "annulus":
            v[ind] = O.project_annulus(x, rmin[s], rmax[s])
        else:
            raise ValueError(st)
    return v


def norms(s, TD_n, mode, norm):
    """float64 norms of the segments of the array s (of shape TD_n, flattened in Fortran order)."""
    s = np.asarray(s, np.float64)
    segs = seg_norms_ref.segment_indices(TD_n, mode)
    if norm == "l1":
        return np.array([np.abs(s[ind]).sum() for ind in segs])
    return np.array([np.sqrt((s[ind] ** 2).sum()) for ind in segs])
