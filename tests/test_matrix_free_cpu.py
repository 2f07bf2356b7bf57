"""Host side of the matrix-free route (no GPU): which custom operators PARSDMM_precompute_distribute hands to the engine
without A'A, the band limit it compares with, and the vectorised CDS conversion of the ones that keep their bands."""
import os
import re

import numpy as np
import pytest

from tests import matrix_free_ops as MF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _setup(sipx, TF, n, h, A, banded=None):
    c = [sipx.set_definitions("bounds", "identity", 0.0, 1.0, ("matrix", "")), MF.custom_set(sipx, "bounds", A, -1.0, 1.0)]
    return MF.setup(sipx, TF, n, h, c, {}, banded=banded)


def test_band_limit_is_the_engines(sipx):
    src = open(os.path.join(ROOT, "setintersectionprojection.jl_amd", "csrc", "sipx_common.h")).read()
    assert sipx.MAX_Q_BANDS == 32 == int(re.search(r"constexpr int MAXD = (\d+);", src).group(1))


@pytest.mark.parametrize("TF", [np.float32, np.float64])
def test_which_operators_go_without_their_ata(sipx, TF):
    n, h = (30, 22), (25.0, 6.0)
    D = MF.dxz(n, h, TF)
    g, opt, P, A, prop, AtA = _setup(sipx, TF, n, h, D)
    assert prop.banded == [True, True, True] and A[1].kind == "custom"
    assert AtA[1].shape == (660, 9) and AtA[1].dtype == TF and len(prop.AtA_offsets[1]) == 9      # banded: the CDS pair, as before
    assert AtA[0] is None and AtA[2] is None
    g, opt, P, A, prop, AtA = _setup(sipx, TF, n, h, D, banded={1: False})                        # the caller says: not banded
    assert AtA[1] is None and prop.AtA_offsets[1].shape == (0,) and prop.AtA_offsets[1].dtype == np.int64
    assert list(prop.AtA_offsets[0]) == [0] and list(prop.AtA_offsets[2]) == [0]
    B = MF.blur()                                                                                  # more diagonals than Q keeps bands
    assert MF.diagonals(B) == 51 > sipx.MAX_Q_BANDS and B.shape == (1560, 2560)
    assert int((np.diff(B.tocsr().indptr) == 0).sum()) == 312
    g, opt, P, A, prop, AtA = _setup(sipx, TF, (64, 40), (1.0, 1.0), B)
    assert prop.banded[1] and AtA[1] is None and len(prop.AtA_offsets[1]) == 0
    assert A[1].ata_diagonals() == 51
    y = [np.zeros(a.shape[0], TF) for a in A]
    assert [len(v) for v in y] == [2560, 1560, 2560]


def test_the_ragged_operator_is_what_the_gpu_tests_say():
    R = MF.ragged((23, 17))
    rows = np.diff(R.tocsr().indptr)
    assert R.shape == (300, 391) and list(rows[:11]) == MF.RAGGED_HEAD and rows[11:].max() <= 11
    assert int((np.diff(R.indptr) == 0).sum()) == 1 and MF.diagonals(R) == 777
    assert MF.tall((23, 17)).shape == (691, 391)


def _ata_cds_loop(op):
    """CustomOperator.ata_cds as it was: one assignment per stored entry of A'A."""
    G = (op.A.T @ op.A).tocsc().astype(op.TF)
    G.sort_indices()
    N = G.shape[0]
    coo = G.tocoo()
    offs = np.unique(coo.col.astype(np.int64) - coo.row.astype(np.int64))
    R = np.zeros((N, len(offs)), op.TF, order="F")
    col = {int(o): b for b, o in enumerate(offs)}
    for r, c, v in zip(coo.row, coo.col, coo.data):
        R[r, col[int(c) - int(r)]] = v
    return R, offs.astype(np.int64)


@pytest.mark.parametrize("TF", [np.float32, np.float64])
def test_vectorised_ata_cds_equals_the_loop(sipx, TF):
    n, h = (30, 22), (25.0, 6.0)
    op = sipx.host.CustomOperator(MF.dxz(n, h, TF), sipx.compgrid(h, n), TF)
    R, off = op.ata_cds()
    R0, off0 = _ata_cds_loop(op)
    assert R.dtype == R0.dtype and R.flags.f_contiguous and off.dtype == off0.dtype
    assert np.array_equal(off, off0) and R.tobytes(order="F") == R0.tobytes(order="F")
    op = sipx.host.CustomOperator(MF.ragged((9, 7, 5)), sipx.compgrid((1.0, 1.0, 1.0), (9, 7, 5)), TF)      # many diagonals, ragged
    R, off = op.ata_cds()
    R0, off0 = _ata_cds_loop(op)
    assert np.array_equal(off, off0) and R.tobytes(order="F") == R0.tobytes(order="F")
