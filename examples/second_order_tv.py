"""First- against second-order isotropic total variation on a ramp with a step.

`("l21", "TV")` bounds sum_p ||grad x(p)||_2: its cheapest models are piecewise constant, so it turns a ramp into a staircase.
`("l21", "Hessian")` bounds sum_p ||H x(p)||_F, the l2,1 norm of the Hessian field (TV^2, the bounded-Hessian regulariser): its null
space is the affine functions, so a ramp costs nothing and a kink or a step costs its height.  A noisy ramp with a step is projected
onto {bounds, ball} with either set, both radii observed on the clean image, and the number of plateaus each result has on the ramp is
printed: a plateau is a run of at least four pixels along the ramp whose successive differences are below a tenth of its slope.

    python examples/second_order_tv.py            (needs the built library and a GPU)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

sipx = load_package()
TF = np.float32
n = (128, 96)
slope = 1.0 / n[0]

# a ramp along the first axis, a step of height 0.5 across the second
i, j = np.meshgrid(np.arange(n[0]), np.arange(n[1]), indexing="ij")
clean = (slope * i + 0.5 * (j >= 60)).astype(TF)
rng = np.random.default_rng(0)
c0 = clean.reshape(-1, order="F")
m = (clean + 0.05 * rng.standard_normal(n)).astype(TF).reshape(-1, order="F")

comp_grid = sipx.compgrid((TF(1.0), TF(1.0)), n)
options = sipx.PARSDMM_options(FL=TF, maxit=500)
radius = {"TV": float(sipx.l21_norm(c0, comp_grid)), "Hessian": float(sipx.l21_stacked_norm(c0, comp_grid, "Hessian"))}


def plateaus(x):
    """Runs of at least four pixels along the ramp with successive differences below slope / 10, summed over the columns left of the step."""
    X = x.reshape(n, order="F")[:, :56]
    flat = np.abs(np.diff(X, axis=0)) < 0.1 * slope
    count = 0
    for col in flat.T:
        run = 0
        for f in list(col) + [False]:
            if f:
                run += 1
            else:
                count += run >= 3      # three flat differences: four pixels
                run = 0
    return count


print("noisy image: %d plateaus on the ramp, rel. error %.3f" % (plateaus(m), np.linalg.norm(m - c0) / np.linalg.norm(c0)))
for op in ("TV", "Hessian"):
    constraint = [
        sipx.set_definitions("bounds", "identity", 0.0, 1.5, ("matrix", "")),
        sipx.set_definitions("l21", op, 0.0, radius[op], ("matrix", "")),
    ]
    P_sub, TD_OP, set_Prop = sipx.setup_constraints(constraint, comp_grid, TF)
    TD_OP, AtA, l, y = sipx.PARSDMM_precompute_distribute(TD_OP, set_Prop, comp_grid, options)
    x, log, _, _ = sipx.PARSDMM(m.copy(), AtA, TD_OP, set_Prop, P_sub, comp_grid, options)
    print("l21 on %-7s radius %8.2f: %3d iterations, set feasibility %s" % (
        op + ",", radius[op], len(log.obj), np.array2string(log.set_feasibility[-1], precision=2)))
    print("    ||TV x||_2,1 = %8.2f   ||H x||_2,1 = %8.2f   plateaus on the ramp: %4d   rel. error against the clean image: %.3f" % (
        sipx.l21_norm(x, comp_grid), sipx.l21_stacked_norm(x, comp_grid, "Hessian"), plateaus(x),
        np.linalg.norm(x - c0) / np.linalg.norm(c0)))
