"""Float64 numpy restatement of the wavelet transform behind TD_OP = "wavelet" (joDWT(n1, n2, wavelet(WT.db4);
L = maxtransformlevels(min(n))), reference src/get_TD_operator.jl:86-88): orthonormal, periodic, multilevel, separable db4.

One level along an axis of length m:  a[k] = sum_j lo[j] x[(2k + 4 - j) mod m],  d[k] = sum_j hi[j] x[(2k + 4 - j) mod m],
a to [0, m/2), d to [m/2, m).  Level l transforms every axis of the box n / 2^(l-1) in place (Mallat layout, as
pywt.coeffs_to_array(pywt.wavedecn(x, "db4", mode="periodization"))).  Arrays are Fortran-ordered grids (dim 0 fastest)."""
import numpy as np

LO = np.array([-0.010597401785069032, 0.0328830116668852, 0.030841381835560764, -0.18703481171909309,
               -0.027983769416859854, 0.6308807679298589, 0.7148465705529157, 0.2303778133088965])
HI = np.array([(-1) ** (j + 1) * LO[7 - j] for j in range(8)])


def levels(n):
    """maxtransformlevels(min(n)): the largest L with 2^L dividing min(n)."""
    m, L = int(min(n)), 0
    while m > 0 and m % 2 == 0:
        m //= 2
        L += 1
    return L


def _axis_matrix(m):
    """The m x m orthogonal matrix of one level along one axis (rows: a then d)."""
    W = np.zeros((m, m))
    for k in range(m // 2):
        for j in range(8):
            i = (2 * k + 4 - j) % m
            W[k, i] += LO[j]
            W[m // 2 + k, i] += HI[j]
    return W


def _apply(x, W, axis):
    return np.moveaxis(np.tensordot(W, x, axes=([1], [axis])), 0, axis)


def dwt(x, inverse=False):
    """W x (or W' x) of an n-dimensional float64 array, same shape."""
    x = np.array(x, dtype=np.float64, copy=True)
    n = x.shape
    L = levels(n)
    lev = range(L, 0, -1) if inverse else range(1, L + 1)
    for l in lev:
        box = tuple(slice(0, s >> (l - 1)) for s in n)
        b = x[box]
        axes = range(x.ndim - 1, -1, -1) if inverse else range(x.ndim)
        for a in axes:
            W = _axis_matrix(b.shape[a])
            b = _apply(b, W.T if inverse else W, a)
        x[box] = b
    return x


def dwt_vec(v, n, inverse=False):
    """The same on a column-major vector of the grid n."""
    return dwt(np.asarray(v, np.float64).reshape(n, order="F"), inverse).reshape(-1, order="F")
