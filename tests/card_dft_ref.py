"""Cardinality behind the DFT (sipx.h, SIPX_PROJ_CARD_DFT) restated in numpy, float64: what the device projector is held to.

    Z = F x (unitary DFT, column-major order); keep the first k entries of the stable order by descending |Z|, ties to the
    lower column-major index (sortperm(by=abs, rev=true), project_cardinality!.jl:18-19); x <- Re(F' Z).

For a real x the members of a conjugate pair (e, e*), e* = every coordinate negated modulo n, have the same magnitude; the
contract takes them as EXACTLY equal -- the magnitudes are symmetrised, max(|Z[e]|, |Z[e*]|) -- so that the tie rule, not the
rounding noise of an FFT, decides which member stays when the cut separates a pair."""
import numpy as np


def partner(n):
    """e* for every column-major index e of a grid n: the index with every coordinate negated modulo n."""
    n = tuple(int(v) for v in n)
    coords = np.unravel_index(np.arange(int(np.prod(n))), n, order="F")
    return np.ravel_multi_index(tuple((-c) % d for c, d in zip(coords, n)), n, order="F")


def spectrum(x, n):
    """(Z, symmetrised |Z|, stable descending order) of a real x, all in column-major order."""
    Z = np.fft.fftn(np.asarray(x, np.float64).reshape(n, order="F"), norm="ortho").reshape(-1, order="F")
    mag = np.abs(Z)
    mag = np.maximum(mag, mag[partner(n)])
    return Z, mag, np.lexsort((np.arange(len(mag)), -mag))


def keep_mask(x, n, k):
    Z, mag, order = spectrum(x, n)
    keep = np.zeros(len(mag), bool)
    keep[order[:max(int(k), 0)]] = True
    return Z, keep


def margin_of(mag, order, k):
    """The smaller relative gap, over |Z|max, between the magnitude classes on either side of the cut: between the last kept and
    the first dropped class, or, when the cut runs through a class (a conjugate pair), between that class and its neighbours
    above and below.  A perturbation of the magnitudes below this changes nothing about the kept set."""
    s = mag[order]
    N = len(s)
    if k <= 0 or k >= N or s[0] == 0:
        return np.inf
    a, b = s[k - 1], s[k]
    if a != b:
        return (a - b) / s[0]
    gaps = []
    if (s > a).any():
        gaps.append(s[s > a].min() - a)
    if (s < a).any():
        gaps.append(a - s[s < a].max())
    return min(gaps) / s[0] if gaps else np.inf


def project(x, n, k):
    """(P x as float64, margin of this call) -- the contract, literally."""
    n = tuple(int(v) for v in n)
    Z, mag, order = spectrum(x, n)
    keep = np.zeros(len(mag), bool)
    keep[order[:max(int(k), 0)]] = True
    out = np.real(np.fft.ifftn((Z * keep).reshape(n, order="F"), norm="ortho")).reshape(-1, order="F")
    return out, margin_of(mag, order, int(k))


def pair_cutting_k(x, n, start=None):
    """The smallest k >= start (default N // 4) at which the cut separates the two members of a class."""
    _, mag, order = spectrum(x, n)
    s = mag[order]
    k = max(1, len(s) // 4 if start is None else int(start))
    while k < len(s) and s[k - 1] != s[k]:
        k += 1
    if k >= len(s):
        raise ValueError("no k cuts a pair")
    return k


def designed(n, seed, TF):
    """A real model whose spectrum has well separated magnitude classes: 1 + j/C, j a random permutation of 0 .. C-1 over the
    C conjugate classes (at least 1/(2C) apart relative to the maximum), random phases, 0 or pi on the self-conjugate bins;
    the real inverse transform of that Hermitian spectrum, rounded to TF.  Column-major vector."""
    n = tuple(int(v) for v in n)
    N = int(np.prod(n))
    rng = np.random.default_rng(seed)
    p = partner(n)
    e = np.arange(N)
    rep = np.minimum(e, p)                       # the lower index names the class
    reps = np.unique(rep)
    C = len(reps)
    cls = np.searchsorted(reps, rep)
    mags = (1.0 + rng.permutation(C) / C)[cls]
    ph = rng.uniform(0.0, 2 * np.pi, C)[cls]
    ph = np.where(e == p, np.pi * rng.integers(0, 2, C)[cls], np.where(e < p, ph, -ph))
    Z = mags * np.exp(1j * ph)
    X = np.fft.ifftn(Z.reshape(n, order="F"), norm="ortho")
    assert np.abs(X.imag).max() <= 1e-12 * np.abs(X.real).max()
    return np.real(X).reshape(-1, order="F").astype(TF)
