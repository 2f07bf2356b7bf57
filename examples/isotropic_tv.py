"""Anisotropic against isotropic total variation on an image with oblique edges.

`("l1", "TV")` bounds sum |D_x x| + |D_z x|: it favours edges along the axes and turns an oblique edge into a staircase.
`("l21", "TV")` bounds sum sqrt((D_x x)^2 + (D_z x)^2), the l2,1 norm of the gradient field -- what the literature calls TV --
and has no preferred direction.  A noisy disc on a ramp is projected onto {bounds, TV ball} with either set, the radius the same
fraction of the respective norm of the clean image, and the two results are compared with the clean image.

    python examples/isotropic_tv.py            (needs the built library and a GPU)
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

# a disc and an oblique half-plane: edges of every orientation
i, j = np.meshgrid(np.arange(n[0]), np.arange(n[1]), indexing="ij")
clean = ((i - 48) ** 2 + (j - 40) ** 2 < 24 ** 2).astype(TF) + 0.5 * (0.6 * i + j > 120).astype(TF)
rng = np.random.default_rng(0)
c0 = clean.reshape(-1, order="F")
m = (clean + 0.2 * rng.standard_normal(n)).astype(TF).reshape(-1, order="F")

comp_grid = sipx.compgrid((TF(1.0), TF(1.0)), n)
options = sipx.PARSDMM_options(FL=TF, maxit=300)
TV = sipx.get_TD_operator(comp_grid, "TV", TF)[0]
fraction = 1.0                                                # of the clean image's norm
radius = {"l1": fraction * float(np.abs(TV @ c0).sum()), "l21": fraction * float(sipx.l21_norm(c0, comp_grid))}

for st in ("l1", "l21"):
    constraint = [
        sipx.set_definitions("bounds", "identity", 0.0, 1.5, ("matrix", "")),
        sipx.set_definitions(st, "TV", 0.0, radius[st], ("matrix", "")),
    ]
    P_sub, TD_OP, set_Prop = sipx.setup_constraints(constraint, comp_grid, TF)
    TD_OP, AtA, l, y = sipx.PARSDMM_precompute_distribute(TD_OP, set_Prop, comp_grid, options)
    x, log, _, _ = sipx.PARSDMM(m.copy(), AtA, TD_OP, set_Prop, P_sub, comp_grid, options)
    print("%-3s on TV, radius %8.1f: %3d iterations, set feasibility %s" % (
        st, radius[st], len(log.obj), np.array2string(log.set_feasibility[-1], precision=2)))
    print("    ||TV x||_1 = %8.1f   ||TV x||_2,1 = %8.1f   rel. error against the clean image: noisy %.3f, projected %.3f" % (
        np.abs(TV @ x).sum(), sipx.l21_norm(x, comp_grid), np.linalg.norm(m - c0) / np.linalg.norm(c0),
        np.linalg.norm(x - c0) / np.linalg.norm(c0)))
