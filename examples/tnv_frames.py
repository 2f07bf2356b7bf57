"""Total nuclear variation of a three-frame stack: frames that share their edges with opposite contrast.

examples/joint_tv_frames.py couples the frames through WHERE the edges are: ("l21_joint", "TV_xy", ("tensor", "")) shrinks every frame's
gradient at a pixel by one factor, whatever the directions of those gradients.  ("tnv", "TV_xy", ("tensor", "")) -- total nuclear variation
-- puts its budget on the sum over the pixels of the nuclear norm of the 2 x n3 matrix of that pixel's gradients: the part of the
gradients that is parallel across the frames (the first singular value) is kept longer than the part that is not (the second), which is
noise when the frames show one geometry.  A frame with the opposite contrast has the opposite gradient: parallel all the same.

Here the clean stack is one shape with contrasts (1, -0.6, 0.3), so every clean Jacobian has rank 1 and both sets measure the same norm on
it.  Both projectors act on the in-plane gradient field of the noisy stack, each at the radius it observes on the clean stack, and the
distance of the result to the clean gradient field is printed.

    python examples/tnv_frames.py            (needs the built library and a GPU)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

sipx = load_package()
TF = np.float32
n = (64, 48, 3)                                      # x, y, frame

# one geometry, three contrasts of either sign, plus noise
rng = np.random.default_rng(0)
shape = np.zeros(n[:2], TF)
shape[12:40, 10:30] = 1.0
shape[30:56, 24:42] += 0.5
clean = np.stack([c * shape for c in (1.0, -0.6, 0.3)], axis=2).astype(TF)
m = (clean + 0.05 * rng.standard_normal(n)).astype(TF).reshape(-1, order="F")
c0 = clean.reshape(-1, order="F")

comp_grid = sipx.compgrid((TF(1.0), TF(1.0), TF(1.0)), n)
A = sipx.TDOperator("TV_xy", comp_grid, TF)
v, v0 = A @ m, A @ c0                                # rows of D_y over (n1, n2 - 1, n3), then rows of D_x over (n1 - 1, n2, n3)

# the radius each set observes on the clean stack: equal up to rounding, the clean Jacobians have rank 1
tau = {"l21_joint": float(sipx.l21_joint_norm(c0, comp_grid)), "tnv": float(sipx.tnv_norm(c0, comp_grid))}
print("radii observed on the clean stack: joint %.4f, nuclear %.4f" % (tau["l21_joint"], tau["tnv"]))
print("norms of the noisy stack:          joint %.4f, nuclear %.4f" % (sipx.l21_joint_norm(m, comp_grid), sipx.tnv_norm(m, comp_grid)))

res = {}
print("set          |P(TV_xy m) - TV_xy clean| / |TV_xy clean|")
print("%-12s %.4f" % ("input", np.linalg.norm(v - v0) / np.linalg.norm(v0)))
for st in ("l21_joint", "tnv"):
    P = sipx.Projector(sipx.set_definitions(st, "TV_xy", 0.0, tau[st], ("tensor", "")), comp_grid, TF)
    res[st] = float(np.linalg.norm(P(v.copy()) - v0) / np.linalg.norm(v0))
    print("%-12s %.4f" % (st, res[st]))
assert res["tnv"] < res["l21_joint"], "the nuclear norm removes the gradient noise that is not parallel across the frames first"
