"""Joint (vectorial) total variation of a three-channel image: frames that share their edges, with different contrasts.

examples/per_frame_isotropic_tv.py gives every frame its own isotropic TV budget, ("l21", "TV_xy", ("slice", "z")): the frames do not
know of each other, and after a projection an edge pixel may keep its gradient in the frame where the contrast is high and lose it in
the frame where it is low.  The joint set ("l21_joint", "TV_xy", ("tensor", "")) puts one budget on the sum over the pixels of the l2
norm of ALL in-plane differences at that pixel in ALL frames: a pixel is an edge in every frame or in none.

Here both projectors act on the in-plane gradient field of a noisy (x, y, 3) stack at comparable budgets -- the norms of the clean
scene as the projectors themselves sum them -- and the pixels that keep a gradient in some but not all frames are counted.

    python examples/joint_tv_frames.py            (needs the built library and a GPU)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

sipx = load_package()
TF = np.float32
n = (64, 48, 3)                                      # x, y, channel
L = n[0] * n[1]

# one geometry, three contrasts, plus noise
rng = np.random.default_rng(0)
shape = np.zeros(n[:2], TF)
shape[12:40, 10:30] = 1.0
shape[30:56, 24:42] += 0.5
clean = np.stack([c * shape for c in (1.0, 0.35, 0.1)], axis=2).astype(TF)
m = (clean + 0.05 * rng.standard_normal(n)).astype(TF).reshape(-1, order="F")
c0 = clean.reshape(-1, order="F")

comp_grid = sipx.compgrid((TF(1.0), TF(1.0), TF(1.0)), n)
A = sipx.TDOperator("TV_xy", comp_grid, TF)
v = A @ m                                            # rows of D_y over (n1, n2 - 1, n3), then rows of D_x over (n1 - 1, n2, n3)

# comparable budgets: what the clean scene needs, per frame and jointly
tau_frames = sipx.l21_norm(c0, comp_grid, "TV_xy", ("slice", "z"))
tau_joint = sipx.l21_joint_norm(c0, comp_grid)
P_frames = sipx.Projector(sipx.set_definitions("l21", "TV_xy", 0.0, tau_frames, ("slice", "z")), comp_grid, TF)
P_joint = sipx.Projector(sipx.set_definitions("l21_joint", "TV_xy", 0.0, float(tau_joint), ("tensor", "")), comp_grid, TF)


def has_gradient(w):
    """(n1 n2, n3) bool: does pixel p keep a non-zero in-plane difference in frame k?"""
    ny = n[0] * (n[1] - 1) * n[2]
    dy = np.zeros(n, bool)
    dx = np.zeros(n, bool)
    dy[:, :-1, :] = w[:ny].reshape((n[0], n[1] - 1, n[2]), order="F") != 0
    dx[:-1, :, :] = w[ny:].reshape((n[0] - 1, n[1], n[2]), order="F") != 0
    return (dy | dx).reshape(L, n[2], order="F")


print("budgets: per frame %s, joint %.2f" % (np.array2string(tau_frames, precision=2), tau_joint))
print("set          pixels with a gradient in: all frames   some but not all   none")
mixed = {}
for name, P in (("input", None), ("per frame", P_frames), ("joint", P_joint)):
    w = v.copy() if P is None else P(v.copy())
    cnt = has_gradient(w).sum(axis=1)
    mixed[name] = int(((cnt > 0) & (cnt < n[2])).sum())
    print("%-12s %37d %18d %6d" % (name, (cnt == n[2]).sum(), mixed[name], (cnt == 0).sum()))
assert mixed["joint"] == 0, "the joint set keeps or drops a pixel's gradient in every frame at once"
