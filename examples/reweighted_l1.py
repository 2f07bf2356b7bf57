"""Iteratively reweighted anisotropic total variation (Candes, Wakin, Boyd: reweighted l1) through one Solver.

`("l1_weighted", "TV", weights=w)` bounds sum_i w_i |(TV x)_i| with one weight per ROW of the TV operator, so the x- and the
z-difference at one grid point carry weights of their own -- what an l2,1 group cannot express.  A noisy piecewise-constant image (a
rectangle, an L-shaped block and a step: axis-aligned edges, the case anisotropic TV is made for) is projected onto {bounds, the ball}

  1. with all weights equal (the plain ("l1", "TV") ball), and
  2. with three rounds of reweighting: w_i = 1 / (|TV x|_i + delta) from the previous result, handed over with Solver.set_data (the
     context, its operators and its device memory stay).  The radius stays the one the Solver was built with -- the l1 norm of TV of the
     clean image -- so every round's weights are scaled to give the clean image exactly that weighted norm
     (sipx.l1_weighted_norm(clean, ..., w)).

It prints the relative error of every round and asserts that the best reweighted round beats the flat one.

    python examples/reweighted_l1.py            (needs the built library and a GPU)
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
N = n[0] * n[1]

i, j = np.meshgrid(np.arange(n[0]), np.arange(n[1]), indexing="ij")
rect = ((i >= 24) & (i < 72) & (j >= 16) & (j < 48)).astype(TF)
ell = (((i >= 60) & (i < 110) & (j >= 56) & (j < 84)) & ~((i >= 80) & (j < 70))).astype(TF)
step = (j >= 64).astype(TF)
clean = (rect + 0.7 * ell + 0.4 * step).reshape(-1, order="F").astype(TF)
rng = np.random.default_rng(0)
m = (clean + 0.2 * rng.standard_normal(N)).astype(TF)

comp_grid = sipx.compgrid((TF(1.0), TF(1.0)), n)
options = sipx.PARSDMM_options(FL=TF, maxit=300)
TV = sipx.get_TD_operator(comp_grid, "TV", TF)[0]
M = TV.shape[0]


def rel_err(x):
    return float(np.linalg.norm(x - clean) / np.linalg.norm(clean))


flat = np.ones(M, TF)
radius = float(sipx.l1_weighted_norm(clean, comp_grid, "TV", flat))
constraint = [sipx.set_definitions("bounds", "identity", 0.0, 2.2, ("matrix", "")),
              sipx.set_definitions("l1_weighted", "TV", 0.0, radius, ("matrix", ""), weights=flat)]
P_sub, TD_OP, set_Prop = sipx.setup_constraints(constraint, comp_grid, TF)
TD_OP, AtA, _, _ = sipx.PARSDMM_precompute_distribute(TD_OP, set_Prop, comp_grid, options)

delta = 0.05
errs = []
print("noisy image: rel. error %.4f" % rel_err(m))
with sipx.Solver(AtA, TD_OP, set_Prop, P_sub, comp_grid, options, TF) as S:
    x, log, _, _ = S(m.copy())
    errs.append(rel_err(x))
    print("%-24s %3d iterations, rel. error against the clean image %.4f" % ("flat weights (plain l1)", len(log.obj), errs[-1]))
    for k in range(3):
        w = (1.0 / (np.abs(np.asarray(TV @ x, np.float64)) + delta)).astype(TF)
        w = (w * TF(radius / float(sipx.l1_weighted_norm(clean, comp_grid, "TV", w)))).astype(TF)
        S.set_data(1, lb=w)
        x, log, _, _ = S(m.copy())
        errs.append(rel_err(x))
        print("%-24s %3d iterations, rel. error against the clean image %.4f" % ("reweighted, round %d" % (k + 1), len(log.obj), errs[-1]))

assert min(errs[1:]) < errs[0], "no reweighted round beat the flat weights: %r" % (errs,)
print("best reweighted round: %.4f against %.4f with flat weights" % (min(errs[1:]), errs[0]))
