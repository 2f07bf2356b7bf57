"""Operators and problems of the matrix-free tests (tests/test_gpu_matrix_free.py, tests/test_matrix_free_cpu.py): sparse
TD_OPs whose A'A has more diagonals than Q keeps bands, and the constraint lists solved on them.  `mod` is either the product
package or the oracle: both mirror the reference's setup functions."""
import functools

import numpy as np
import scipy.sparse as sp

from oracle import parsdmm_oracle as O

RAGGED_HEAD = [0, 0, 1, 2, 63, 64, 65, 127, 128, 129, 130]     # both sides of every lane-group size, empty rows


def model(n, TF, seed=0):
    rng = np.random.default_rng(20240601 + seed)
    z = np.linspace(0, 1, n[-1]).reshape((1,) * (len(n) - 1) + (-1,))
    return (1500 + 2500 * z + 150 * rng.standard_normal(n)).astype(TF).reshape(-1, order="F")


def ragged(n, M=300):
    """M rows over prod(n) columns: the lengths of RAGGED_HEAD, then integers(0, 12); columns without replacement, U(-1, 1)."""
    N = int(np.prod(n))
    rng = np.random.default_rng(11)
    lens = RAGGED_HEAD + [int(v) for v in rng.integers(0, 12, M - len(RAGGED_HEAD))]
    rows, cols, vals = [], [], []
    for r, L in enumerate(lens):
        L = min(L, N)
        cols.append(rng.choice(N, L, replace=False))
        vals.append(rng.uniform(-1, 1, L))
        rows.append(np.full(L, r))
    A = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(M, N))
    A.sort_indices()
    return A


def tall(n):
    A = ragged(n)
    T = sp.vstack([A, 0.5 * sp.identity(A.shape[1])]).tocsc()
    T.sort_indices()
    return T


def blur(n=(64, 40), bkl=25):
    """mask * kron(I, Bx) of the reference's deblurring example (motion blur along x of length bkl: the diagonals 0 and
    2 .. bkl of weight 1 / bkl, the last bkl rows dropped); the mask zeroes one row in five, explicit zeros eliminated."""
    n1, n2 = n
    Bx = sp.identity(n1, format="csc") / bkl
    for i in range(2, bkl + 1):
        Bx = Bx + sp.diags([np.ones(n1 - i)], [i], shape=(n1, n1)) / bkl
    Bx = Bx.tocsr()[:n1 - bkl, :]
    BF = sp.kron(sp.identity(n2), Bx).tocsc()
    mask = np.ones(BF.shape[0])
    mask[::5] = 0.0
    A = (sp.diags(mask) @ BF).tocsc()
    A.eliminate_zeros()
    A.sort_indices()
    return A


def psf(n, k):
    """k x k box point-spread function on a 2-D grid (valid part): k^2 taps per row."""
    n1, n2 = n

    def box(m):
        return sp.diags([np.ones(m - k + 1)] * k, list(range(k)), shape=(m - k + 1, m)) / k
    A = sp.kron(box(n2), box(n1)).tocsc()
    A.sort_indices()
    return A


def dxz(n, h, TF):
    Og = O.compgrid(h, n)
    Dx = O.get_TD_operator(Og, "D_x", TF)[0]
    Dz1 = O.get_TD_operator(O.compgrid(h, (n[0] - 1, n[1])), "D_z", TF)[0]
    A = sp.csc_matrix(Dz1 @ Dx, dtype=TF)
    A.sort_indices()
    return A


def uniform_rows(n, L, M=150, seed=5):
    """Every row with L entries (the lane group of the forward product follows L), columns without replacement."""
    N = int(np.prod(n))
    rng = np.random.default_rng(seed + L)
    cols = np.concatenate([rng.choice(N, L, replace=False) for _ in range(M)])
    A = sp.csc_matrix((rng.uniform(-1, 1, M * L), (np.repeat(np.arange(M), L), cols)), shape=(M, N))
    A.sort_indices()
    return A


def diagonals(A):
    P = sp.csc_matrix((np.ones(A.nnz), A.indices, A.indptr), shape=A.shape)
    c = (P.T @ P).tocoo()
    return len(np.unique(c.col.astype(np.int64) - c.row.astype(np.int64)))


def custom_set(mod, kind, A, lo, hi):
    sd = mod.set_definitions(kind, "identity", lo, hi, ("matrix", ""))
    sd.custom_TD_OP = (A, False)
    return sd


# ---- the problems of the solve tests: (grid, spacing, m, constraint list, options) ---------------------------------------------
def ragged_problem(mod, TF, n=(23, 17), h=(1.0, 1.0), **opt):
    m = model(n, TF)
    A = ragged(n).astype(TF)
    TV = O.get_TD_operator(O.compgrid(h, n), "TV", TF)[0]
    c = [mod.set_definitions("bounds", "identity", 1600.0, 3900.0, ("matrix", "")),
         mod.set_definitions("l1", "TV", 0.0, float(0.5 * np.abs(TV @ m).sum()), ("matrix", "")),
         custom_set(mod, "l2", A, 0.0, float(0.7 * np.linalg.norm((A @ m).astype(np.float64))))]
    return n, h, m, c, dict(maxit=300, **opt)


def blur_problem(mod, TF, **opt):
    n, h = (64, 40), (1.0, 1.0)
    truth = model(n, TF, seed=1)
    A = blur(n).astype(TF)
    d = (A @ truth).astype(TF)
    m = (truth.astype(np.float64) + 200.0 * np.random.default_rng(5).standard_normal(truth.size)).astype(TF)
    c = [mod.set_definitions("bounds", "identity", 1400.0, 4100.0, ("matrix", "")),
         mod.set_definitions("bounds", "D_z", -60.0, 400.0, ("matrix", "")),
         custom_set(mod, "bounds", A, (d - TF(15)).astype(TF), (d + TF(15)).astype(TF))]
    return n, h, m, c, dict(maxit=300, **opt)


def setup(mod, TF, n, h, c, opt_kw, banded=None):
    """-> (m-independent) g, options, P_sub, TD_OP, set_Prop, AtA.  banded: {set index: value} written into set_Prop.banded."""
    g = mod.compgrid(h, n)
    opt = mod.PARSDMM_options(FL=TF, **opt_kw)
    P, A, prop = mod.setup_constraints(c, g, TF)
    for i, v in (banded or {}).items():
        prop.banded[i] = v
    A, AtA, l, y = mod.PARSDMM_precompute_distribute(A, prop, g, opt)
    return g, opt, P, A, prop, AtA


@functools.lru_cache(maxsize=None)
def oracle_solve(name, tf):
    """x, log of the oracle for a named problem, once per session (the results are not to be modified)."""
    TF = np.dtype(tf).type
    if name == "ragged":
        n, h, m, c, kw = ragged_problem(O, TF)
    elif name == "ragged3d":
        n, h, m, c, kw = ragged_problem(O, TF, n=(16, 12, 8), h=(1.0, 1.0, 1.0))
    elif name == "blur":
        n, h, m, c, kw = blur_problem(O, TF)
    elif name == "blur_feas":
        n, h, m, c, kw = blur_problem(O, TF, feasibility_only=True)
    else:
        raise KeyError(name)
    g, opt, P, A, prop, AtA = setup(O, TF, n, h, c, kw)
    x, log, _, _ = O.PARSDMM(m.copy(), AtA, A, prop, P, g, opt)
    x.setflags(write=False)
    return x, log
