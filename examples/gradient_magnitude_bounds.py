"""A slope bound that does not care which way an edge runs: ("l2inf", "TV") against ("bounds", "TV").

`("bounds", "TV", -c, c)` bounds every difference direction on its own: a box around the gradient vector.  An edge along a grid axis
may be as steep as c, a diagonal one sqrt(2) c, so the two are treated differently.  `("l2inf", "TV", 0, c)` bounds the gradient
magnitude ||grad x(p)||_2 <= c at every grid point (csrc/l2inf.h): the isotropic slope constraint.  The model has two ramps of equal
steepness s, one along the first axis and one along the diagonal; both are projected onto {amplitude bounds, slope set} with c = s / 2
and the steepest gradient magnitude left on either ramp is printed.  Then the vector form: "nowhere steeper than 1.1 times the gradient
of a smooth prior model", c = 1.1 * tv_group_norms(prior).

    python examples/gradient_magnitude_bounds.py            (needs the built library and a GPU)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

sipx = load_package()
TF = np.float32
n = (96, 96)
s = 0.05                                   # the steepness of both ramps: the gradient magnitude on them

i, j = np.meshgrid(np.arange(n[0]), np.arange(n[1]), indexing="ij")
ramp = lambda t: np.clip(t, 0.0, 14.0)     # fourteen pixels of slope 1 in its argument
axis_edge = s * ramp(i - 20.0)                                  # a ramp along the first axis, gradient (s, 0)
diag_edge = s * ramp((i + j - 150.0) / np.sqrt(2.0))            # a ramp along the diagonal, gradient (s, s) / sqrt(2); the two do not meet
model = (axis_edge + diag_edge).astype(TF)
m = model.reshape(-1, order="F")
comp_grid = sipx.compgrid((TF(1.0), TF(1.0)), n)
options = sipx.PARSDMM_options(FL=TF, maxit=300)
on_axis = ((i > 10) & (i < 45) & (i + j < 130)).reshape(-1, order="F")
on_diag = ((i + j > 135) & (i > 50) & (i < 95) & (j < 95)).reshape(-1, order="F")


def steepest(x):
    g = sipx.tv_group_norms(x, comp_grid)
    return float(g[on_axis].max()), float(g[on_diag].max())


def project(slope_set):
    constraint = [sipx.set_definitions("bounds", "identity", -1.0, 2.0, ("matrix", "")), slope_set]
    P_sub, TD_OP, set_Prop = sipx.setup_constraints(constraint, comp_grid, TF)
    TD_OP, AtA, l, y = sipx.PARSDMM_precompute_distribute(TD_OP, set_Prop, comp_grid, options)
    x, log, _, _ = sipx.PARSDMM(m.copy(), AtA, TD_OP, set_Prop, P_sub, comp_grid, options)
    return x, log


c = s / 2
print("model: steepest gradient magnitude on the axis-aligned ramp %.4f, on the diagonal ramp %.4f (c = %.4f)" % (*steepest(m), c))
for name, sd in (("bounds on TV (box)", sipx.set_definitions("bounds", "TV", -c, c, ("matrix", ""))),
                 ("l2inf on TV (ball)", sipx.set_definitions("l2inf", "TV", 0, c, ("matrix", "")))):
    x, log = project(sd)
    a, d = steepest(x)
    print("%s: %3d iterations; steepest on the axis-aligned ramp %.4f = %.2f c, on the diagonal ramp %.4f = %.2f c" % (
        name, len(log.obj), a, a / c, d, d / c))

# the vector form: a smooth prior model, and "nowhere steeper than 1.1 times the prior"
prior = (0.5 * (1 + np.tanh((i - 48.0) / 12.0)) * (1 + 0.3 * np.cos(j / 15.0))).astype(TF).reshape(-1, order="F")
cvec = (TF(1.1) * sipx.tv_group_norms(prior, comp_grid)).astype(TF)
noisy = (prior + 0.05 * np.random.default_rng(0).standard_normal(prior.size)).astype(TF)
m = noisy
x, log = project(sipx.set_definitions("l2inf", "TV", 0, cvec, ("matrix", "")))
g = sipx.tv_group_norms(x, comp_grid)
has = cvec > 0.05 * cvec.max()             # (where the prior is flat c is tiny and the ratio says little)
print("vector form, c = 1.1 tv_group_norms(prior): %3d iterations, set feasibility %s; max g / c where the prior has a slope %.3f "
      "(noisy model: %.1f); rel. error against the prior %.3f (noisy model: %.3f)" % (
          len(log.obj), np.array2string(log.set_feasibility[-1], precision=2), float((g[has] / cvec[has]).max()),
          float((sipx.tv_group_norms(noisy, comp_grid)[has] / cvec[has]).max()),
          np.linalg.norm(x - prior) / np.linalg.norm(prior), np.linalg.norm(noisy - prior) / np.linalg.norm(prior)))
