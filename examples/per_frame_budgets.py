"""Per-frame anisotropic TV with one budget per frame: bounds plus an l1 ball on D_x and on D_y of every time frame, each frame with
the radius observed on that frame of a clean scene.

examples/per_frame_tv.py gives every frame the largest per-frame TV of the clean scene: a frame with little structure is
constrained by the budget of the busiest one.  Here `sipx.segment_norms` observes ||D_x c||_1 and ||D_y c||_1 of every frame of the
clean scene c on the device, and `setup_constraints(..., segment_norms=True)` takes the two vectors as the radii of the per-slice
sets.  The scene holds a box that grows from frame to frame, so the budgets differ.  Printed: per frame, the TV of the projected
scene over the frame's own budget, with per-frame budgets and with the shared maximum.

    python examples/per_frame_budgets.py       (needs the built library and a GPU)
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

# a box that moves one pixel per frame and grows with it, plus noise
rng = np.random.default_rng(0)
clean = np.zeros(n, TF)
for t in range(n[2]):
    clean[8 + t:14 + 2 * t + t, 10:16 + 2 * t, t] = 1.0
c0 = clean.reshape(-1, order="F")
m = (clean + 0.15 * rng.standard_normal(n)).astype(TF).reshape(-1, order="F")

comp_grid = sipx.compgrid((TF(1.0), TF(1.0), TF(1.0)), n)
options = sipx.PARSDMM_options(FL=TF, maxit=300)
frames = ("slice", "z")

# the budgets: one per frame, observed on the clean scene (several training scenes: np.maximum over the results)
bx = sipx.segment_norms(c0, comp_grid, "D_x", frames, "l1")
by = sipx.segment_norms(c0, comp_grid, "D_y", frames, "l1")


def solve(rx, ry):
    constraint = [
        sipx.set_definitions("bounds", "identity", 0.0, 1.0, ("tensor", "")),
        sipx.set_definitions("l1", "D_x", 0.0, rx, frames),
        sipx.set_definitions("l1", "D_y", 0.0, ry, frames),
    ]
    P_sub, TD_OP, set_Prop = sipx.setup_constraints(constraint, comp_grid, TF, segment_norms=True)
    TD_OP, AtA, l, y = sipx.PARSDMM_precompute_distribute(TD_OP, set_Prop, comp_grid, options)
    x, log, _, _ = sipx.PARSDMM(m.copy(), AtA, TD_OP, set_Prop, P_sub, comp_grid, options)
    return x, log


x_own, log_own = solve(bx, by)
x_max, log_max = solve(float(bx.max()), float(by.max()))

print("budgets ||D_x c||_1 per frame:", np.array2string(bx, precision=0))
print("frame   TV_x / own budget:  noisy   per-frame budgets   shared maximum")
tx = {k: sipx.segment_norms(v, comp_grid, "D_x", frames, "l1") / bx for k, v in (("noisy", m), ("own", x_own), ("max", x_max))}
for t in range(n[2]):
    print("%5d %27.2f %19.3f %16.3f" % (t, tx["noisy"][t], tx["own"][t], tx["max"][t]))
for name, x, log in (("per-frame budgets", x_own, log_own), ("shared maximum", x_max, log_max)):
    print("%s: %d iterations, rel. error against the clean scene %.3f (noisy %.3f)" % (
        name, len(log.obj), np.linalg.norm(x - c0) / np.linalg.norm(c0), np.linalg.norm(m - c0) / np.linalg.norm(c0)))
