"""The geometries and inputs tests/test_card_groups_cpu.py and tests/test_gpu_card_groups.py share (no GPU needed to import)."""
import numpy as np

from tests import card_groups_ref as R

# the CASES of tests/test_gpu_l21_groups.py, restated (importing that module would import torch and the oracle): the geometry list of
# tests/test_gpu_seg_norms.py on the identity, difference operators along and across the segments, L = 1, (32,12,8) for the 16-byte
# stores, (8200,3) for the fourth path of seg_norm_plan -- and (30,12,8): n1 % 4 != 0, so k_cardg_zero stores scalars there
IDENTITY_CASES = [((33, 6, 5), ("fiber", "x")), ((300, 4, 3), ("fiber", "x")), ((5, 7, 33), ("fiber", "y")), ((5, 7, 33), ("fiber", "z")),
                  ((70, 3, 300), ("fiber", "z")), ((96, 96, 10), ("slice", "z")), ((10, 96, 96), ("slice", "x")),
                  ((96, 10, 96), ("slice", "y")), ((40, 28), ("fiber", "x")), ((40, 28), ("fiber", "z")), ((4, 5, 2), ("fiber", "z"))]
L21G_CASES = [("identity", n, mode) for n, mode in IDENTITY_CASES] + [
    ("D_z", (5, 7, 33), ("fiber", "z")), ("D_x", (5, 7, 33), ("fiber", "z")), ("D_z", (96, 96, 10), ("slice", "z")),
    ("D_x", (40, 28), ("fiber", "x")), ("D_z", (4, 5, 2), ("fiber", "z")),
    ("identity", (32, 12, 8), ("fiber", "z")), ("identity", (32, 12, 8), ("slice", "z")), ("identity", (8200, 3), ("fiber", "x"))]
# ... and the two sides of the threshold between the selection routes: (32,32,3) fiber z has CARDG_SMALL_MAX = 1024 segments, the last
# size of the small route, (41,25,3) fiber z 1025, the first that takes the engine's search by default
CASES = L21G_CASES + [("identity", (30, 12, 8), ("fiber", "z")), ("identity", (30, 12, 8), ("slice", "z")),
                      ("identity", (32, 32, 3), ("fiber", "z")), ("identity", (41, 25, 3), ("fiber", "z"))]
BIG_TIE = ("identity", (96, 96, 4), ("fiber", "z"))      # 9216 identical fibers: a tie group above CARD_CAP = 8192, k = 100
SMALL_MAX = 1024                                          # CARDG_SMALL_MAX (tests/test_card_groups_cpu.py holds it to the header)
CARD_CAP = 8192

_cache = {}


def segs(op, n, mode):
    key = ("s", op, n, mode)
    if key not in _cache:
        _cache[key] = R.segments(n, op, mode)
    return _cache[key]


def ks(ns):
    """k in {1, nseg // 3, nseg - 1}, those that are >= 1 and < nseg."""
    return sorted({k for k in (1, ns // 3, ns - 1) if 1 <= k < ns})


def mixed_input(op, n, mode, TF, zeros=True):
    """Segment s is heavy (s % 4 == 0), light (1) or plain (2, 3); with `zeros` every eighth one (s % 8 == 2) is all zero with -0.0 entries.
    Computed once, handed out as a copy.  Without zeros every segment is non-zero, so k = nseg - 1 drops exactly one."""
    key = ("v", op, n, mode, np.dtype(TF).name, zeros)
    if key not in _cache:
        rng = np.random.default_rng(20261021 + sum(n) + len(op))
        v = np.zeros(R.rows(n, op), TF)
        for s, idx in enumerate(segs(op, n, mode)):
            x = rng.standard_normal(len(idx))
            if zeros and s % 8 == 2:
                v[idx[::2]] = -0.0
            elif s % 4 == 0:
                v[idx] = 30.0 * x * np.exp(rng.standard_normal(len(idx)))
            elif s % 4 == 1:
                v[idx] = 1e-3 * x
            else:
                v[idx] = x
        _cache[key] = v
    return _cache[key].copy()


def tie_input(op, n, mode, TF, k):
    """Entries in {0, +-1, +-2}: sums of squares are exact integers in any order, so equal segments have equal norm bits whatever the
    tile.  Every third segment is `heavy` (one entry 2, one entry -2 where the segment has two), the others share ONE norm (a single entry
    +-1 at a position that moves with s): with k between the heavy count and nseg the k-th place falls inside that tie group."""
    sg = segs(op, n, mode)
    v = np.zeros(R.rows(n, op), TF)
    for s, idx in enumerate(sg):
        if s % 3 == 0:
            v[idx[s % len(idx)]] = 2.0
            if len(idx) > 1:
                v[idx[(s + 1) % len(idx)]] = -2.0
        else:
            v[idx[(5 * s) % len(idx)]] = -1.0 if s % 2 else 1.0
    heavy = len(range(0, len(sg), 3))
    assert heavy < k < len(sg) - 1, "k does not straddle the tie group"
    return v
