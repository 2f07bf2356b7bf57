"""How far an output of the rank projector is from an optimal rank-r truncation (float64 numpy, no GPU).

The truncated matrix T_r(X) is discontinuous in X wherever sigma_r = sigma_{r+1}; its DISTANCE to X is not.  For an input
slice X (values of the working precision widened to float64), an output slice Y and a rank r:

    excess(X, Y, r)   = (||X - Y||_F - sqrt(sum_{i>r} sigma_i(X)^2)) / ||X||_F    how much farther Y is than the best rank-r matrix
    rankdefect(Y, r)  = sqrt(sum_{i>r} sigma_i(Y)^2) / ||X||_F                    how far Y is from having rank r

Every optimal truncation -- whichever way a tie is broken -- has both at rounding level; a wrong subspace, a missed large
direction, a stale start that was accepted or a slice written to another slice's place raises at least one far above it.
A zero slice must come back as exact zeros (both measures are infinite otherwise).

The bound an engine output is held to, per slice (`tau`):  4 * max(d_oracle, u), where d_oracle is the larger of the two
measures of oracle.project_rank on the same input (the reference's arithmetic) and u the unit roundoff of the working
precision (2^-24 / 2^-53: what rounding the output, and the projector's input inside update_y_l, costs relative to ||X||_F).
The factor 4: two correct decompositions of the Float32 class differ by a small multiple of each other.  At the strict
acceptance level (SIPX_RANK_STRICT=1: pairs accepted at 1e-12 on the Gram matrix) the oracle term is dropped."""
import numpy as np

FACTOR = 4.0


def unit_roundoff(TF):
    return 2.0 ** -24 if np.dtype(TF) == np.float32 else 2.0 ** -53


def slices_of(x, n, mode):
    """The float64 slices of the vector x on the grid n (column-major), in the reference's order: the matrix itself, or
    X[i,:,:] / X[:,i,:] / X[:,:,i] for ("slice", "x" / "y" / "z")."""
    X = np.asarray(x, np.float64).reshape(tuple(n), order="F")
    if X.ndim == 2:
        return [X]
    if mode[0] != "slice":
        raise ValueError("rank projections of a tensor act on its slices")
    ax = {"x": 0, "y": 1, "z": 2}[mode[1]]
    return [np.take(X, i, axis=ax) for i in range(X.shape[ax])]


def truncate(X, r):
    """An optimal rank-r approximation of X (float64 LAPACK SVD)."""
    U, s, Vt = np.linalg.svd(np.asarray(X, np.float64), full_matrices=False)
    return (U[:, :r] * s[:r]) @ Vt[:r, :]


def _sv(M):
    return np.linalg.svd(np.asarray(M, np.float64), compute_uv=False)


def _tail(s, r):
    return float(np.sqrt(np.sum(s[r:] ** 2)))


def excess(X, Y, r, sX=None):
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    nx = float(np.linalg.norm(X))
    if nx == 0.0:
        return 0.0 if not Y.any() else float("inf")
    return (float(np.linalg.norm(X - Y)) - _tail(_sv(X) if sX is None else sX, r)) / nx


def rankdefect(X, Y, r):
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    nx = float(np.linalg.norm(X))
    if nx == 0.0:
        return 0.0 if not Y.any() else float("inf")
    return _tail(_sv(Y), r) / nx


def defect(X, Y, r, sX=None):
    """The larger of the two measures (excess may be negative by rounding only: Y cannot be closer than the optimum by
    more than its own distance from rank r)."""
    return max(excess(X, Y, r, sX), rankdefect(X, Y, r))


def gap(X, r, sX=None):
    """(sigma_r - sigma_{r+1}) / sigma_1; 0 for the zero matrix, and for r >= min(shape) the whole of sigma_r / sigma_1."""
    s = _sv(X) if sX is None else sX
    if s[0] == 0.0 or r < 1:
        return 0.0
    if r >= len(s):
        return float(s[-1] / s[0])
    return float((s[r - 1] - s[r]) / s[0])


def tau(X, Y_oracle, r, TF, strict=False, sX=None):
    u = unit_roundoff(TF)
    if strict:
        return FACTOR * u
    return FACTOR * max(defect(X, Y_oracle, r, sX), u)


def check_rank_output(x, y, y_oracle, r, n, mode, TF, strict=False, label="", gap_tol=None, x_oracle=None, collect=None):
    """Holds every slice of the output y (input x, oracle output y_oracle: vectors on the grid n) to `tau`; where the spectrum
    has a clear gap, (sigma_r - sigma_{r+1}) / sigma_1 >= 0.1, also to ||Y - oracle|| <= gap_tol ||oracle||.  x_oracle: the
    input the oracle was given, where that is x rounded to TF (its own defect is measured against what it saw).
    Returns one record per slice (excess, rankdefect, tau, gap, ...).  collect = None: asserts; a list: failures are appended
    to it as (label, slice, text) and nothing is raised."""
    if gap_tol is None:
        gap_tol = 2e-5 if np.dtype(TF) == np.float32 else 1e-11
    out = []
    bad = []
    Xo = slices_of(x if x_oracle is None else x_oracle, n, mode)
    for i, (X, Y, Yo) in enumerate(zip(slices_of(x, n, mode), slices_of(y, n, mode), slices_of(y_oracle, n, mode))):
        nx = float(np.linalg.norm(X))
        if nx == 0.0:
            out.append(dict(slice=i, excess=0.0, rankdefect=0.0, tau=0.0, gap=0.0, norm=0.0, oracle_defect=0.0))
            if Y.any():
                bad.append((label, i, "a zero slice came back non-zero"))
            continue
        sX = _sv(X)
        rec = dict(slice=i, excess=excess(X, Y, r, sX), rankdefect=rankdefect(X, Y, r), gap=gap(X, r, sX), norm=nx,
                   oracle_defect=defect(Xo[i], Yo, r, sX if x_oracle is None else None))
        rec["tau"] = FACTOR * unit_roundoff(TF) if strict else FACTOR * max(rec["oracle_defect"], unit_roundoff(TF))
        if not (rec["excess"] <= rec["tau"] and rec["rankdefect"] <= rec["tau"]):
            bad.append((label, i, "excess %.3e rankdefect %.3e tau %.3e (oracle %.3e)" % (rec["excess"], rec["rankdefect"],
                                                                                        rec["tau"], rec["oracle_defect"])))
        if rec["gap"] >= 0.1:
            d = float(np.linalg.norm(Y - Yo))
            rec["to_oracle"] = d / float(np.linalg.norm(Yo))
            if not d <= gap_tol * float(np.linalg.norm(Yo)):
                bad.append((label, i, "gap %.2f: ||Y - oracle|| / ||oracle|| = %.3e > %.1e" % (rec["gap"], rec["to_oracle"], gap_tol)))
        out.append(rec)
    if collect is None:
        assert not bad, bad
    else:
        collect.extend(bad)
    return out


# ---- input families (one slice each; the callers stack them) ----------------------------------------------------------------
def gapped(shape, rank, rng, noise=1e-3, scale=1.0):
    """Orthonormal factors, singular values falling from 1 to 0.5 over `rank` directions, plus white noise of `noise` times its
    Frobenius norm: (sigma_rank - sigma_{rank+1}) / sigma_1 is about 0.5."""
    m, n = shape
    U = np.linalg.qr(rng.standard_normal((m, rank)))[0]
    V = np.linalg.qr(rng.standard_normal((n, rank)))[0]
    s = np.linspace(1.0, 0.5, rank)
    S = (U * s) @ V.T
    E = rng.standard_normal(shape)
    return scale * (S + noise * np.linalg.norm(S) / np.linalg.norm(E) * E)


def flat(shape, rng, level=2500.0, sd=1.0):
    """White noise on a constant: sigma_1 about 1e4 times the rest, and no gap anywhere behind it."""
    return level + sd * rng.standard_normal(shape)


def exact_rank2(shape, rng):
    """u1 v1' + u2 v2' from integer vectors with entries in -3 .. 3: exact in Float32, rank exactly 2."""
    m, n = shape
    X = np.zeros(shape)
    for _ in range(2):
        X += np.outer(rng.integers(-3, 4, m), rng.integers(-3, 4, n)).astype(np.float64)
    return X


def hadamard(k):
    H = np.ones((1, 1))
    while H.shape[0] < k:
        H = np.block([[H, H], [H, -H]])
    return H


def tied(shape, rng, r):
    """sum_i s_i h_i g_i' with columns h_i, g_i of a 64 x 64 Hadamard matrix (exactly orthogonal, entries +-1) and integer
    weights s with s_r = s_{r+1}: integer entries, exact in Float32, singular values 64 s_i -- the tie survives rounding.
    Embedded in the top-left corner of a zero matrix of `shape`."""
    H = hadamard(64)
    s = np.zeros(64)
    s[:r + 1] = np.arange(2 * (r + 1), 0, -2) + 2.0          # ... 8, 6, 4
    s[r] = s[r - 1]                                          # the tie at sigma_r
    s[r + 1:r + 3] = (2.0, 1.0)
    s[r + 3:16] = 1.0                                        # (and a flat tail)
    hp, gp = rng.permutation(64), rng.permutation(64)
    X = np.zeros(shape)
    X[:64, :64] = (H[:, hp] * s) @ H[:, gp].T
    return X


def single_entry(shape, rng, value=3.0):
    X = np.zeros(shape)
    X[rng.integers(0, shape[0]), rng.integers(0, shape[1])] = value
    return X


def stack(slabs, d="z"):
    """Slices (all of one shape) to the vector of the tensor that has them along direction d, column-major."""
    ax = {"x": 0, "y": 1, "z": 2}[d]
    return np.stack(slabs, axis=ax).reshape(-1, order="F")
