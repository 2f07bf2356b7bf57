"""Reference of the per-fiber / per-slice norm sets (pure numpy, no GPU): the oracle's whole-vector projector applied to every
segment of the array of shape TD_n, segments and their elements in the order of SegMap (csrc/ext_family.h): a fiber's elements
along its direction, a slice's with the lower remaining dimension fastest; segments with the lower remaining dimension fastest.
For the norm sets the order inside a segment only fixes the order of the reference's sums."""
import numpy as np

AXES3 = {"x": 0, "y": 1, "z": 2}


def axis_of(TD_n, mode):
    """0-based array axis of mode = (kind, letter): on a 2-D grid z is the second axis (host.Projector)."""
    if len(TD_n) == 2:
        return {"x": 0, "z": 1}[mode[1]]
    return AXES3[mode[1]]


def segment_indices(TD_n, mode):
    """List of flat (Fortran-order) index arrays, one per segment."""
    TD_n = tuple(int(v) for v in TD_n)
    if mode[0] not in ("fiber", "slice"):
        raise ValueError("mode must be a fiber or slice mode")
    if len(TD_n) == 2 and mode[0] == "slice":
        raise ValueError("for 2D models the mode needs to be (fiber,x) or (fiber,z)")
    d3 = TD_n + (1,) * (3 - len(TD_n))
    idx = np.arange(int(np.prod(d3))).reshape(d3, order="F")
    ax = axis_of(TD_n, mode)
    a, b = (1 if ax == 0 else 0), (1 if ax == 2 else 2)
    out = []
    if mode[0] == "fiber":
        for ib in range(d3[b]):
            for ia in range(d3[a]):
                sel = [0, 0, 0]
                sel[a], sel[b], sel[ax] = ia, ib, slice(None)
                out.append(idx[tuple(sel)].copy())
    else:
        for i in range(d3[ax]):
            out.append(np.take(idx, i, axis=ax).reshape(-1, order="F"))      # remaining axes a < b, a fastest
    return out


def project_segments(v, TD_n, mode, fun):
    """v <- fun applied to every fiber / slice (in place, and returned).  fun takes a contiguous vector of v's type and returns its
    projection (oracle.project_l1_Duchi, project_l2, project_annulus with their scalars bound)."""
    for ind in segment_indices(TD_n, mode):
        v[ind] = fun(np.ascontiguousarray(v[ind]))
    return v
