"""Per-frame anisotropic TV of a small video-like tensor: bounds plus an l1 ball on D_x and on D_y of every time frame.

The reference's examples/GeneralizedMinkowski/Minkowski_video_decomposition.jl constrains every frame (("slice", "z")) with
cardinality sets, because its l1 ball exists for the whole array only.  The convex per-frame form is an l1 ball per z-slice,
which `setup_constraints(..., segment_norms=True)` takes: every frame is projected on its own, all frames share the radius.

    python examples/per_frame_tv.py            (needs the built library and a GPU)
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

# a blocky scene whose box moves one pixel per frame, plus noise
rng = np.random.default_rng(0)
clean = np.zeros(n, TF)
for t in range(n[2]):
    clean[8 + t:24 + t, 10:26, t] = 1.0
m = (clean + 0.15 * rng.standard_normal(n)).astype(TF).reshape(-1, order="F")

comp_grid = sipx.compgrid((TF(1.0), TF(1.0), TF(1.0)), n)
options = sipx.PARSDMM_options(FL=TF, maxit=300)
Dx = sipx.get_TD_operator(comp_grid, "D_x", TF)[0]
Dy = sipx.get_TD_operator(comp_grid, "D_y", TF)[0]
c0 = clean.reshape(-1, order="F")


def per_frame_l1(A, shape, x):
    return np.abs(A @ x).reshape(shape, order="F").sum(axis=(0, 1))


# radius: the largest per-frame TV of the clean scene
bx = float(per_frame_l1(Dx, (n[0] - 1, n[1], n[2]), c0).max())
by = float(per_frame_l1(Dy, (n[0], n[1] - 1, n[2]), c0).max())
constraint = [
    sipx.set_definitions("bounds", "identity", 0.0, 1.0, ("tensor", "")),
    sipx.set_definitions("l1", "D_x", 0.0, bx, ("slice", "z")),
    sipx.set_definitions("l1", "D_y", 0.0, by, ("slice", "z")),
]
P_sub, TD_OP, set_Prop = sipx.setup_constraints(constraint, comp_grid, TF, segment_norms=True)
TD_OP, AtA, l, y = sipx.PARSDMM_precompute_distribute(TD_OP, set_Prop, comp_grid, options)
x, log, _, _ = sipx.PARSDMM(m, AtA, TD_OP, set_Prop, P_sub, comp_grid, options)

print("%d iterations, set feasibility %s" % (len(log.obj), np.array2string(log.set_feasibility[-1], precision=2)))
print("per-frame ||D_x x||_1 / radius: noisy %.2f .. %.2f, projected %.3f .. %.3f" % (
    per_frame_l1(Dx, (n[0] - 1, n[1], n[2]), m).min() / bx, per_frame_l1(Dx, (n[0] - 1, n[1], n[2]), m).max() / bx,
    per_frame_l1(Dx, (n[0] - 1, n[1], n[2]), x).min() / bx, per_frame_l1(Dx, (n[0] - 1, n[1], n[2]), x).max() / bx))
print("rel. error against the clean scene: noisy %.3f, projected %.3f" % (
    np.linalg.norm(m - c0) / np.linalg.norm(c0), np.linalg.norm(x - c0) / np.linalg.norm(c0)))
