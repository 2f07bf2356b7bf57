"""Structure-guided and iteratively reweighted isotropic total variation.

`("l21", "TV", weights=w)` bounds sum_p w_p ||(grad x)_p||_2: a small weight makes a gradient at p cheap, weight 0 takes p out of the
constraint.  A noisy image of a disc on an oblique half-plane is projected onto {bounds, the TV ball}

  1. with all weights equal (plain isotropic TV),
  2. with weights from a guide image that has the same edges at other amplitudes, w_p = 1 / (1 + |grad guide|_p / eta), and
  3. with three rounds of reweighting through ONE Solver: w_p = 1 / (g_p + delta) from the gradient norms g of the previous result,
     handed over with Solver.set_data (the context, its operators and its device memory stay).

Every radius is the weighted norm of the clean image under the weights in use (sipx.l21_norm(..., weights=w)).

    python examples/weighted_tv.py            (needs the built library and a GPU)
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
shape = ((i - 48) ** 2 + (j - 40) ** 2 < 24 ** 2).astype(TF), (0.6 * i + j > 120).astype(TF)
clean = (shape[0] + 0.5 * shape[1]).reshape(-1, order="F")
guide = (0.3 * shape[0] - 1.0 * shape[1]).reshape(-1, order="F")          # another modality: same edges, other amplitudes
rng = np.random.default_rng(0)
m = (clean + 0.2 * rng.standard_normal(N)).astype(TF)

comp_grid = sipx.compgrid((TF(1.0), TF(1.0)), n)
options = sipx.PARSDMM_options(FL=TF, maxit=300)
TV = sipx.get_TD_operator(comp_grid, "TV", TF)[0]


def gradient_norms(x):
    """g_p = ||(grad x)_p||_2 per grid point, column-major: the M-vector of TV x is vcat(D_z x, D_x x) in the rows of each block."""
    v = np.asarray(TV @ x, np.float64)
    nz = n[0] * (n[1] - 1)
    dz = np.zeros(n)
    dz[:, :-1] = v[:nz].reshape((n[0], n[1] - 1), order="F")
    dx = np.zeros(n)
    dx[:-1, :] = v[nz:].reshape((n[0] - 1, n[1]), order="F")
    return np.sqrt(dz ** 2 + dx ** 2).reshape(-1, order="F")


def problem(w):
    radius = float(sipx.l21_norm(clean, comp_grid, "TV", weights=w))
    constraint = [sipx.set_definitions("bounds", "identity", 0.0, 1.5, ("matrix", "")),
                  sipx.set_definitions("l21", "TV", 0.0, radius, ("matrix", ""), weights=w)]
    P_sub, TD_OP, set_Prop = sipx.setup_constraints(constraint, comp_grid, TF)
    TD_OP, AtA, _, _ = sipx.PARSDMM_precompute_distribute(TD_OP, set_Prop, comp_grid, options)
    return AtA, TD_OP, set_Prop, P_sub, comp_grid, options


def report(name, x, log):
    print("%-28s %3d iterations, rel. error against the clean image %.4f (noisy: %.4f)" % (
        name, len(log.obj), np.linalg.norm(x - clean) / np.linalg.norm(clean), np.linalg.norm(m - clean) / np.linalg.norm(clean)))


flat = np.ones(N, TF)
x, log, _, _ = sipx.PARSDMM(m.copy(), *problem(flat))
report("flat weights (plain TV)", x, log)

eta = 0.05
w_guide = (1.0 / (1.0 + gradient_norms(guide) / eta)).astype(TF)
x, log, _, _ = sipx.PARSDMM(m.copy(), *problem(w_guide))
report("weights from the guide", x, log)

# reweighting: the radius stays the one the Solver was built with, so every round's weights are scaled to give the clean image
# that weighted norm
delta = 0.05
args = problem(flat)
radius = args[3][1].pmax
with sipx.Solver(*args, TF) as S:
    x, log, _, _ = S(m.copy())
    for k in range(3):
        w = 1.0 / (gradient_norms(x) + delta)
        w = (w * (radius / float(np.sum(w * gradient_norms(clean))))).astype(TF)
        S.set_data(1, lb=w)
        x, log, _, _ = S(m.copy())
        report("reweighted, round %d" % (k + 1), x, log)
