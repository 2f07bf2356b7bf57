"""Per-frame isotropic TV of a small video-like tensor: bounds plus, for every time frame, an l2,1 ball on the in-plane gradient.

examples/per_frame_tv.py gives every frame an anisotropic budget (an l1 ball on D_x and one on D_y), examples/isotropic_tv.py the
whole array one isotropic budget on the 3-D TV operator, whose groups couple neighbouring frames.  Here every frame k has its own
2-D isotropic TV budget: sum over the frame's points of ||(D_y x, D_x x)_p||_2 <= tau_k, the set ("l21", "TV_xy", ("slice", "z")).
The radii are observed per frame on the clean scene with l21_norm(..., ("slice", "z")): the numbers the projector itself compares.

    python examples/per_frame_isotropic_tv.py            (needs the built library and a GPU)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

sipx = load_package()
TF = np.float32
n = (48, 40, 12)                                     # x, y, time

# a blocky scene whose box moves one pixel per frame and grows, plus noise
rng = np.random.default_rng(0)
clean = np.zeros(n, TF)
for t in range(n[2]):
    clean[8 + t:24 + t + t // 2, 10:26, t] = 1.0
m = (clean + 0.15 * rng.standard_normal(n)).astype(TF).reshape(-1, order="F")
c0 = clean.reshape(-1, order="F")

comp_grid = sipx.compgrid((TF(1.0), TF(1.0), TF(1.0)), n)
options = sipx.PARSDMM_options(FL=TF, maxit=300)

# radii: the isotropic TV of every frame of the clean scene
tau = sipx.l21_norm(c0, comp_grid, "TV_xy", ("slice", "z"))
constraint = [
    sipx.set_definitions("bounds", "identity", 0.0, 1.0, ("tensor", "")),
    sipx.set_definitions("l21", "TV_xy", 0.0, tau, ("slice", "z")),
]
P_sub, TD_OP, set_Prop = sipx.setup_constraints(constraint, comp_grid, TF)
TD_OP, AtA, l, y = sipx.PARSDMM_precompute_distribute(TD_OP, set_Prop, comp_grid, options)
x, log, _, _ = sipx.PARSDMM(m, AtA, TD_OP, set_Prop, P_sub, comp_grid, options)

before = sipx.l21_norm(m, comp_grid, "TV_xy", ("slice", "z"))
after = sipx.l21_norm(x, comp_grid, "TV_xy", ("slice", "z"))
print("%d iterations, set feasibility %s" % (len(log.obj), np.array2string(log.set_feasibility[-1], precision=2)))
print("frame   radius    noisy  projected  projected / radius")
for k in range(n[2]):
    print("%5d %8.2f %8.2f %10.2f %19.4f" % (k, tau[k], before[k], after[k], after[k] / tau[k]))
print("rel. error against the clean scene: noisy %.3f, projected %.3f" % (
    np.linalg.norm(m - c0) / np.linalg.norm(c0), np.linalg.norm(x - c0) / np.linalg.norm(c0)))
