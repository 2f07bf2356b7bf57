"""What tests/test_l20_cpu.py and tests/test_gpu_l20.py share: the cases of the l2,0 sets on TV / TV_xy (csrc/l20.h), their budgets and
their inputs.  A case is (op, n, form), form one of tests/l20_ref.FORMS.  The shapes are the smallest at which each path can go wrong:

  2-D  (5, 7)        scalar stores                          (8, 6)       16-byte stores, the far face along x inside a vector
  3-D  (4, 5, 3)     wide in Float32 only, 60 groups        (8, 4, 6)    wide       (30, 12, 8)   scalar, 2880 groups: the search route
  the selection routes: (32, 32) has CARDG_SMALL_MAX = 1024 groups, (41, 25) has 1025
  joint: the chunked grids of tests/test_gpu_l21_joint.py, (8, 4, 67) with 8 ragged chunks and (4, 3, 16) with two, and (33, 20, 3)
  frames: one frame size on each side of the LDS cap of 32 KiB per precision -- (64, 64, 3) fits in both (exactly in Float64), (96, 96, 3)
          streams in both, (72, 64, 3) fits in Float32 and streams in Float64 -- and (5, 4, 2), (8, 6, 3) for the two store widths"""
import numpy as np

from tests import l20_ref as R

SMALL_MAX = 1024          # csrc/card_groups.h: CARDG_SMALL_MAX
CARD_CAP = 8192           # tests/card_exact.py, the engine's gather capacity: a tie group above it goes through the search's tie cut
LDS_BYTES = 32 * 1024     # csrc/seg_norm.h: SEGN_LDS_BYTES

WHOLE = [("TV", (5, 7), "whole"), ("TV", (8, 6), "whole"), ("TV", (4, 5, 3), "whole"), ("TV", (8, 4, 6), "whole"), ("TV", (30, 12, 8), "whole"),
         ("TV", (32, 32), "whole"), ("TV", (41, 25), "whole"), ("TV_xy", (8, 4, 6), "whole"), ("TV_xy", (5, 4, 3), "whole")]
JOINT = [("TV_xy", (8, 4, 67), "joint"), ("TV_xy", (4, 3, 16), "joint"), ("TV_xy", (33, 20, 3), "joint")]
FRAMES = [("TV_xy", (5, 4, 2), "frames"), ("TV_xy", (8, 6, 3), "frames"), ("TV_xy", (64, 64, 3), "frames"), ("TV_xy", (72, 64, 3), "frames"),
          ("TV_xy", (96, 96, 3), "frames")]
CASES = WHOLE + JOINT + FRAMES
BIG_TIE = ("TV", (96, 96), "whole")          # 96 x 96 identical groups: one tie group above CARD_CAP

_cache = {}


def ks(ng):
    """The budgets of the selection test: 1, a third, all but one."""
    return sorted({1, max(ng // 3, 1), ng - 1} - {0})


def mixed_input(op, n, form, TF, zeros=True):
    """An M-vector of the range (any v is allowed, not only gradients): heavy-tailed entries, some groups all zero (with -0.0 members), some
    pairs of groups with equal members.  Cached, read-only."""
    key = (op, tuple(n), form, np.dtype(TF).name, zeros)
    if key not in _cache:
        rng = np.random.default_rng(1000 + sum(n) + len(n))
        M = R.rows(n, op)
        v = (rng.standard_normal(M) * np.exp(1.5 * rng.standard_normal(M))).astype(TF)
        G = R.members(n, op)
        N = G.shape[0]
        if zeros:
            for p in range(0, N, 5):                       # every fifth group: all zero, the odd ones with -0.0
                idx = G[p][G[p] >= 0]
                v[idx] = TF(-0.0) if p % 2 else TF(0.0)
        if N >= 12:
            for a, b in ((1, 7), (2, 11)):                 # ties: copy the members of group a onto group b where both have them
                both = (G[a] >= 0) & (G[b] >= 0)
                if form != "joint":
                    v[G[b][both]] = v[G[a][both]]
        v.setflags(write=False)
        _cache[key] = v
    return _cache[key]


def group_rows(n, op, form):
    """list over the groups that compete (whole: N points; frames: N points too, frame by frame; joint: pixels) of their member indices."""
    G = R.members(n, op)
    if form != "joint":
        return [G[p][G[p] >= 0] for p in range(G.shape[0])]
    L, n3 = int(n[0]) * int(n[1]), int(n[2])
    return [np.concatenate([G[p + f * L][G[p + f * L] >= 0] for f in range(n3)]) for p in range(L)]
