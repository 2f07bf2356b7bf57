"""Cardinality behind the DFT on the device (sipx.h SIPX_PROJ_CARD_DFT, csrc/ext_transform.hip EXT_CARD_DFT) against the numpy
restatement of its contract (tests/card_dft_ref.py): the projector alone on inputs whose kept set is unambiguous, its properties
on generic inputs, the learned count DFT_card_095 fed back into it, and whole solves against the oracle with the restatement
substituted into P_sub (the oracle's own ("cardinality", "DFT") falls through to plain cardinality)."""
import numpy as np
import pytest
import torch      # (before libsipx.so is loaded: one HIP runtime in the process, see host._check_one_hip_runtime)

from oracle import parsdmm_oracle as O      # checker only
from tests import card_dft_ref as R
from tests.test_gpu_device_io import _equal_results
from tests.test_gpu_learn import H as H_LEARN, images

pytestmark = pytest.mark.gpu

GRIDS = [(16, 12, 8), (15, 12, 9), (30, 21), (6, 5), (3, 8)]
TOL = {np.float32: 2e-5, np.float64: 1e-10}          # the bounds test_library_backed_projectors holds the l1-DFT projector to


def _projector(sipx, n, k, TF):
    g = sipx.compgrid(tuple(1.0 for _ in n), n)
    return sipx.Projector(sipx.set_definitions("cardinality", "DFT", 0, int(k), ("matrix" if len(n) == 2 else "tensor", "")), g, TF)


def _ks(x, n):
    N = int(np.prod(n))
    kc = R.pair_cutting_k(x, n, start=2)
    return [1, kc, kc + 1, max(N // 10, 1), N - 1]


def _rel(a, b):
    return np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b)


@pytest.mark.parametrize("TF", [np.float32, np.float64])
@pytest.mark.parametrize("n", GRIDS)
def test_projector_matches_the_contract(sipx, monkeypatch, TF, n):
    """Inputs built from a Hermitian spectrum with magnitude classes at least 1/(2C) apart (card_dft_ref.designed): the kept set
    is the same in both precisions and through both transforms, so the device result is the restatement's up to the rounding of
    the transforms.  Through the real transform (R2C / C2R, half-weights on the stored bins) and through the complex one."""
    x = R.designed(n, 7, TF)
    for k in _ks(x, n):
        want, margin = R.project(x, n, k)
        assert margin >= 1e-4, (n, k, margin)                      # a condition on the input, met by construction
        for real in (("1", "0") if n[0] >= 4 else ("1",)):
            monkeypatch.setenv("SIPX_DFT_REAL", real)
            got = _projector(sipx, n, k, TF)(x.copy())
            err = _rel(got, want)
            print(f"card_dft n={n} {np.dtype(TF).name} k={k} real={real}: rel. l2 error {err:.3e} (margin {margin:.2e})")
            assert got.dtype == TF and err <= TOL[TF], (n, k, real, err)


@pytest.mark.parametrize("TF", [np.float32, np.float64])
@pytest.mark.parametrize("n", GRIDS)
def test_projector_properties(sipx, TF, n):
    """A generic random model.  At most k bins of the result's spectrum stand above the noise of the transforms -- k + 1 when the
    cut separates a conjugate pair, whose two members come back with half their weight.  Projecting the result again leaves it
    where it is; where a pair was halved the second projection halves it again (the set is not convex and Re(F' .) of one member
    of a pair is not a fixed point -- in the contract as in the reference), and what is checked there is the contract applied to
    the first result.  k = N returns the input bit for bit, k = 0 zeros."""
    N = int(np.prod(n))
    x = np.random.default_rng(100 + N).standard_normal(N).astype(TF)
    _, mag, order = R.spectrum(x, n)
    s = mag[order]
    thr = (1e-5 if TF == np.float32 else 1e-11) * s[0]
    for k in _ks(x, n):
        cuts = s[k - 1] == s[k]
        P = _projector(sipx, n, k, TF)
        y = P(x.copy())
        above = int((np.abs(np.fft.fftn(y.astype(np.float64).reshape(n, order="F"), norm="ortho")) > thr).sum())
        assert above <= k + (1 if cuts else 0), (n, k, above)
        assert above >= min(k, int((s > 2 * thr).sum())), (n, k, above)          # ... and nothing more was dropped
        again = P(y.copy())
        ref = y.astype(np.float64) if not cuts else R.project(y, n, k)[0]
        assert _rel(again, ref) <= TOL[TF], (n, k, cuts)
    assert np.array_equal(_projector(sipx, n, N, TF)(x.copy()), x)
    assert np.array_equal(_projector(sipx, n, N + 5, TF)(x.copy()), x)
    assert not _projector(sipx, n, 0, TF)(x.copy()).any()


def test_learned_count_fed_back(sipx):
    """k = DFT_card_095[i], the number of Fourier coefficients that carry 95 % of image i (constraint_learning_by_observation.jl:
    134-136: N - findfirst(cumsum(sort(|F x|)) / total > 0.05)): dropping all but k leaves more than 5 % of ||F x||_1 behind,
    dropping all but k + 1 at most 5 % -- in the float64 unitary spectrum, with 1e-4 for the Float32 transforms."""
    TF, n = np.float32, (64, 64)
    m = images(3, n, TF)
    g = sipx.compgrid(H_LEARN, n)
    got = sipx.constraint_learning_by_obseration(g, m)
    F = lambda v: np.fft.fft2(np.asarray(v, np.float64).reshape(n, order="F"), norm="ortho")
    for i in range(len(m)):
        k = int(got["DFT_card_095"][i])
        assert 0 < k < n[0] * n[1]
        x = m[i].reshape(-1, order="F").copy()
        total = np.abs(F(x)).sum()
        P_k = sipx.Projector(sipx.set_definitions("cardinality", "DFT", 0, k, ("matrix", "")), g, TF)
        P_k1 = sipx.Projector(sipx.set_definitions("cardinality", "DFT", 0, k + 1, ("matrix", "")), g, TF)
        left_k = np.abs(F(x.astype(np.float64) - P_k(x.copy()))).sum()
        left_k1 = np.abs(F(x.astype(np.float64) - P_k1(x.copy()))).sum()
        print(f"image {i}: k = {k}, left behind by P_k {left_k / total:.6f}, by P_k+1 {left_k1 / total:.6f}")
        assert left_k1 <= (0.05 + 1e-4) * total and left_k >= (0.05 - 1e-4) * total, (i, k, left_k / total, left_k1 / total)


# (grid, spacing, seed of the designed model, k): chosen on the CPU so that every projector call of the ORACLE's solve -- 14 in 12
# iterations -- has a margin of 4.7e-4 or more in both precisions; k = 77 separates a conjugate pair, k = 386 does not
SOLVES = [((32, 24), (25.0, 6.0), 2, 77), ((16, 12, 8), (25.0, 25.0, 25.0), 1, 386)]


def _solve_problem(mod, n, h, TF, m, k, margins=None):
    b = float(2.0 * np.std(m.astype(np.float64)))
    g = mod.compgrid(h, n)
    opt = mod.PARSDMM_options(FL=TF, maxit=12)
    c = [mod.set_definitions("bounds", "identity", -b, b, ("matrix", "")),
         mod.set_definitions("cardinality", "DFT", 0, k, ("matrix", ""))]
    P, A, prop = mod.setup_constraints(c, g, TF)
    if margins is not None:                                    # the oracle: the restatement as the set's P_sub, margins recorded
        def closure(x):
            out, mg = R.project(x, n, k)
            margins.append(mg)
            x[:] = out.astype(TF)
            return x
        P[1] = closure
    A, AtA, _, _ = mod.PARSDMM_precompute_distribute(A, prop, g, opt)
    return AtA, A, prop, P, g, opt


@pytest.mark.parametrize("TF", [np.float32, np.float64])
@pytest.mark.parametrize("n,h,seed,k", SOLVES)
def test_solve_with_cardinality_behind_the_dft(sipx, monkeypatch, TF, n, h, seed, k):
    """{bounds on the model, at most k Fourier atoms} + the distance term, 12 iterations: through the real and the complex
    transform, against the oracle -- the bounds of test_l1_behind_the_dft_through_the_real_transform."""
    m = R.designed(n, seed, TF)
    out = []
    for real in ("1", "0"):
        monkeypatch.setenv("SIPX_DFT_REAL", real)
        args = _solve_problem(sipx, n, h, TF, m, k)
        assert args[3][1].kind == "card_dft" and args[2].ncvx[1]
        out.append(sipx.PARSDMM(m.copy(), *args))
    monkeypatch.delenv("SIPX_DFT_REAL")
    margins = []
    xo, lo, _, _ = O.PARSDMM(m.copy(), *_solve_problem(O, n, h, TF, m, k, margins))
    assert len(margins) >= 12 and min(margins) >= 1e-4, (len(margins), min(margins))
    (xr, lr, _, _), (xc, lc, _, _) = out
    nrm = np.linalg.norm(xo)
    e_rc = np.linalg.norm(xr.astype(np.float64) - xc.astype(np.float64)) / nrm
    e_ro = np.linalg.norm(xr.astype(np.float64) - xo) / nrm
    print(f"solve n={n} {np.dtype(TF).name} k={k}: R2C vs C2C {e_rc:.3e}, vs oracle {e_ro:.3e}, smallest margin {min(margins):.2e}, "
          f"iterations {len(lr.obj)} / {len(lc.obj)} / {len(lo.obj)}")
    assert e_rc < (2e-5 if TF == np.float32 else 1e-9)
    assert e_ro < (5e-4 if TF == np.float32 else 1e-6)
    assert len(lr.obj) == len(lc.obj) == len(lo.obj)


def test_device_form_gives_the_bits_of_the_host_form(sipx):
    n, h, seed, k = SOLVES[1]
    TF = np.float32
    m = R.designed(n, seed, TF)
    args = _solve_problem(sipx, n, h, TF, m, k)
    sipx.clear_context_cache()
    try:
        host = sipx.PARSDMM(m.copy(), *args)
        sipx.clear_context_cache()
        dev = sipx.PARSDMM_device(torch.from_numpy(m.copy()).cuda(), *args)
        assert not dev[1].context_reused and len(host[1].obj) > 1
        _equal_results(dev, host)
    finally:
        sipx.clear_context_cache()
