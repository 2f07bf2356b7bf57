"""Three noisy material-fraction maps projected onto {probability simplex per pixel, smooth in the plane}.

A fraction map stack (x, y, material) holds, at every pixel, numbers that are nonnegative and sum to one along the material axis.
`("simplex", "identity", 1.0, 1.0, ("fiber", "z"))` is that set: every fiber z of the array is projected onto the probability simplex
(csrc/seg_simplex.h, one GPU lane a pixel for so short a fiber).  Together with the anisotropic total variation of every map in its own
plane, `("l1", "TV_xy")`, the solve denoises the stack without leaving the set of fraction maps.

It prints the per-pixel sums (sipx.segment_sums, the projector's own first pass) and the most negative entry before and after, and the
relative error against the clean maps.

    python examples/fraction_maps.py            (needs the built library and a GPU)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

sipx = load_package()
TF = np.float32
n = (96, 80, 3)
mode = ("fiber", "z")

i, j = np.meshgrid(np.arange(n[0]), np.arange(n[1]), indexing="ij")
a = ((i - 30) ** 2 + (j - 30) ** 2 < 18 ** 2).astype(np.float64)           # a disc of material 1
b = ((i >= 50) & (j >= 35)).astype(np.float64) * (1.0 - a)                  # a block of material 2, the rest is material 3
clean = np.stack([0.8 * a + 0.1, 0.8 * b + 0.1, 1.0 - (0.8 * a + 0.1) - (0.8 * b + 0.1)], axis=2)
rng = np.random.default_rng(0)
m = (clean + 0.15 * rng.standard_normal(n)).astype(TF).reshape(-1, order="F")
clean = clean.astype(TF).reshape(-1, order="F")

comp_grid = sipx.compgrid((TF(1.0), TF(1.0), TF(1.0)), n)
options = sipx.PARSDMM_options(FL=TF, maxit=200)
TVxy = sipx.get_TD_operator(comp_grid, "TV_xy", TF)[0]
constraint = [sipx.set_definitions("simplex", "identity", 1.0, 1.0, mode),
              sipx.set_definitions("l1", "TV_xy", 0.0, float(np.abs(TVxy @ clean).sum()), ("tensor", ""))]
P_sub, TD_OP, set_Prop = sipx.setup_constraints(constraint, comp_grid, TF)
TD_OP, AtA, _, _ = sipx.PARSDMM_precompute_distribute(TD_OP, set_Prop, comp_grid, options)
x, log, _, _ = sipx.PARSDMM(m.copy(), AtA, TD_OP, set_Prop, P_sub, comp_grid, options)


def report(name, v):
    s = sipx.segment_sums(v, comp_grid, "identity", mode)      # sums of the positive parts, one per pixel
    print("%-8s per-pixel sums in [%.4f, %.4f], most negative entry %+.4f, rel. error %.4f"
          % (name, s.min(), s.max(), v.min(), np.linalg.norm(v - clean) / np.linalg.norm(clean)))


report("noisy", m)
report("solved", x)
y = P_sub[0](x.copy())                                         # the last step onto the simplex itself
report("on set", y)
s = sipx.segment_sums(y, comp_grid, "identity", mode)
assert y.min() >= 0 and np.all(np.abs(s - 1) <= 4 * np.finfo(TF).eps), "the projection left the simplex"
assert np.linalg.norm(y - clean) < np.linalg.norm(m - clean), "the solve did not bring the maps closer to the clean ones"
print("%d iterations" % len(log.obj))
