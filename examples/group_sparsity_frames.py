"""Group sparsity on a stack of frames: where, and when, does a time lapse change?

`("l21_groups", "D_z", ("fiber", "z"))` bounds the sum over the pixels of the l2 norm of a pixel's change over time: the changes are
confined to a few places.  `("l21_groups", "D_z", ("slice", "z"))` bounds the sum over the time steps of the l2 norm of the whole frame
difference: there are few change times (the group fused lasso).  Both are ONE ball whose segments compete for the budget;
`("l2", "D_z", same mode)` would give every segment a ball of its own.

A synthetic (x, y, frame) stack -- a static background, a patch that brightens at frame 6 and another that fades at frame 11 -- is
observed with noise and projected onto {bounds, the group ball}

  1. per fiber z (few places),
  2. per slice z (few times), and
  3. per fiber z once more with weights w = 1 / (segment_norms + c) from the first result, handed over with Solver.set_data.

Every radius is the group norm of the clean stack (sipx.l21_groups_norm).

    python examples/group_sparsity_frames.py            (needs the built library and a GPU)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

sipx = load_package()
TF = np.float32
n = (48, 40, 16)
N = int(np.prod(n))

clean = np.full(n, 0.5, TF)
clean[10:22, 8:20, 6:] += 0.4            # brightens at frame 6
clean[30:40, 22:34, :11] += 0.3          # fades at frame 11
clean = clean.reshape(-1, order="F")
rng = np.random.default_rng(0)
m = (clean + 0.1 * rng.standard_normal(N)).astype(TF)

comp_grid = sipx.compgrid((TF(1.0), TF(1.0), TF(1.0)), n)
options = sipx.PARSDMM_options(FL=TF, maxit=300)


def problem(mode, weights=None, radius=None):
    if radius is None:
        radius = float(sipx.l21_groups_norm(clean, comp_grid, "D_z", mode, weights=weights))
    constraint = [sipx.set_definitions("bounds", "identity", 0.0, 1.5, ("tensor", "")),
                  sipx.set_definitions("l21_groups", "D_z", 0.0, radius, mode, weights=weights)]
    P_sub, TD_OP, set_Prop = sipx.setup_constraints(constraint, comp_grid, TF)
    TD_OP, AtA, _, _ = sipx.PARSDMM_precompute_distribute(TD_OP, set_Prop, comp_grid, options)
    return AtA, TD_OP, set_Prop, P_sub, comp_grid, options


def report(name, x, log, mode):
    g = sipx.segment_norms(x, comp_grid, "D_z", mode, "l2")
    print("%-34s %3d iterations, rel. error %.4f (noisy: %.4f), segments with a change: %d of %d" % (
        name, len(log.obj), np.linalg.norm(x - clean) / np.linalg.norm(clean), np.linalg.norm(m - clean) / np.linalg.norm(clean),
        int(np.sum(g > 1e-3 * g.max())), len(g)))


fiber, slab = ("fiber", "z"), ("slice", "z")
x, log, _, _ = sipx.PARSDMM(m.copy(), *problem(slab))
report("few change times (slice z)", x, log, slab)

# few places, then one reweighting step through the same Solver: the weights of a set built with weights are replaceable
ones = np.ones(n[0] * n[1], TF)
args = problem(fiber, ones)
radius = args[3][1].pmax
with sipx.Solver(*args, TF) as S:
    x, log, _, _ = S(m.copy())
    report("few places (fiber z)", x, log, fiber)
    c = 0.05
    w = 1.0 / (sipx.segment_norms(x, comp_grid, "D_z", fiber, "l2").astype(np.float64) + c)
    # the radius stays the one the Solver was built with: the weights are scaled to give the clean stack that weighted norm
    w = (w * (radius / float(sipx.l21_groups_norm(clean, comp_grid, "D_z", fiber, weights=w.astype(TF))))).astype(TF)
    S.set_data(1, lb=w)
    x, log, _, _ = S(m.copy())
    report("few places, reweighted once", x, log, fiber)
