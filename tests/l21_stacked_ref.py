"""Reference of the l2,1 ball across the equal-sized blocks of a stacked operator (csrc/l21_stacked.h), pure numpy, and of the named
operator "Hessian" of the front end.

The M-vector has B blocks of G = M / B entries; the group of p < G is { v[q G + p] : q < B }: every position is a member, there are no
coordinates and no pads.  Group norms in float64, added in block order; the threshold is the exact sort-based l1 threshold of the TF
group norms (tests/l1_exact.py), the array the engine searches.  The pattern of tests/l21_ref.py."""
import numpy as np

from tests import l1_exact


def sumsq(v, B):
    """The float64 sums of squares of the G groups, added in block order q = 0 .. B - 1."""
    v64 = np.asarray(v, np.float64)
    assert v64.ndim == 1 and v64.size % B == 0
    blocks = v64.reshape(B, v64.size // B)
    ss = np.zeros(blocks.shape[1], np.float64)
    for q in range(B):
        ss = ss + blocks[q] * blocks[q]
    return ss


def norms(v, B, TF):
    """g of the contract: sqrt of the float64 sum of squares, rounded once to TF."""
    return np.sqrt(sumsq(v, B)).astype(TF)


def norm21(v, B):
    """sum_p g_p in extended precision from the float64 group norms."""
    return float(np.sum(np.sqrt(sumsq(v, B)).astype(l1_exact._WIDE)))


def project(v, B, b):
    """The projection of v onto { sum_p g_p <= b } in float64: theta is the exact l1 threshold of the TF group norms, the weights
    max(g - theta, 0) / g come from the unrounded float64 norms.  v itself comes back when g lies inside the l1 ball away from
    rounding (l1_exact.feasibility)."""
    v = np.asarray(v)
    TF = v.dtype.type
    g = norms(v, B, TF)
    if l1_exact.feasibility(g, b) > 0:
        return v
    theta, _, _ = l1_exact.exact_theta(g.astype(np.float64), b)
    g64 = np.sqrt(sumsq(v, B))
    f = np.zeros_like(g64)
    pos = g64 > 0
    f[pos] = np.maximum(g64[pos] - theta, 0.0) / g64[pos]
    return (v.astype(np.float64).reshape(B, -1) * f[None, :]).reshape(-1)


# ---- the named operator "Hessian": the stencils, entry by entry, without a sparse product --------------------------------------------------
def hessian_blocks(n):
    """The blocks of the Hessian of a grid of shape n, in order: ("pure", a) for D_aa, ("mixed", a, b) for sqrt(2) D_ab."""
    nd = len(n)
    return [("pure", a) for a in range(nd)] + [("mixed", a, b) for a in range(nd) for b in range(a + 1, nd)]


def hessian_dense(n, h, TF):
    """The (B N, N) matrix of the contract as a dense float64 array whose entries are the TF values: row q N + p is entry q of the
    Hessian at grid point p (column-major), a zero row where the stencil leaves the grid.  Pure second differences are centred at p:
    (x[p - e_a] - 2 x[p] + x[p + e_a]) ih_a^2; the mixed one starts at p: the forward difference along a of the forward difference
    along b, times sqrt(2); ih_a = fl(1 / h_a) in TF, products and the factor sqrt(2) rounded in TF as the front end forms them."""
    TF = np.dtype(TF).type
    n = tuple(int(k) for k in n)
    N = int(np.prod(n))
    ih = [TF(1) / TF(hk) for hk in h]
    st = [int(np.prod(n[:a])) for a in range(len(n))]
    coords = np.unravel_index(np.arange(N), n, order="F")
    blocks = hessian_blocks(n)
    H = np.zeros((len(blocks) * N, N), np.float64)
    r2 = TF(np.sqrt(TF(2)))
    for q, blk in enumerate(blocks):
        if blk[0] == "pure":
            a = blk[1]
            w = TF(ih[a] * ih[a])
            for p in np.nonzero((coords[a] >= 1) & (coords[a] <= n[a] - 2))[0]:
                H[q * N + p, p - st[a]] = w
                H[q * N + p, p] = TF(-2) * w
                H[q * N + p, p + st[a]] = w
        else:
            a, b = blk[1], blk[2]
            w = TF(r2 * TF(ih[a] * ih[b]))
            for p in np.nonzero((coords[a] < n[a] - 1) & (coords[b] < n[b] - 1))[0]:
                H[q * N + p, p] = w
                H[q * N + p, p + st[a]] = -w
                H[q * N + p, p + st[b]] = -w
                H[q * N + p, p + st[a] + st[b]] = w
    return H
