"""L0 gradient smoothing: at most k edge pixels, at full contrast.

`("l20", "TV", 0, k, ("matrix", ""))` says that at most k grid points of an image carry a gradient at all -- a piecewise-constant model
whose edges are not shrunk -- where the convex set `("l21", "TV")`, isotropic total variation, asks for a radius tau that nobody knows in
advance and pays for every edge it keeps with its contrast.  `("cardinality", "TV")` is another set: it counts differences, so a
diagonal edge costs two and it prefers staircases.

A noisy piecewise-constant image -- a disc and a rectangle on a flat ground -- is projected onto

  1. {bounds, l20 on TV with the k of the clean image}, and
  2. {bounds, l21 on TV with the radius of the clean image} (sipx.l21_norm),

and both are compared with the clean image: the error, the number of edge pixels (sipx.tv_group_norms, the array the projector selects
on) and how much of the contrast across the edges survives.  Then three frames that share one edge set, with another contrast each, are
projected onto {bounds, l20_joint on TV_xy}: at most k pixels carry an edge in any frame.

    python examples/l0_gradient.py            (needs the built library and a GPU)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

sipx = load_package()
TF = np.float32
n = (64, 48)
options = sipx.PARSDMM_options(FL=TF, maxit=300)
rng = np.random.default_rng(0)


def shapes(n2d):
    i, j = np.meshgrid(np.arange(n2d[0]), np.arange(n2d[1]), indexing="ij")
    return (i - 20) ** 2 + (j - 18) ** 2 < 100, (i > 38) & (i < 56) & (j > 24) & (j < 40)


def solve(m, constraint, comp_grid):
    P_sub, TD_OP, set_Prop = sipx.setup_constraints(constraint, comp_grid, TF)
    TD_OP, AtA, _, _ = sipx.PARSDMM_precompute_distribute(TD_OP, set_Prop, comp_grid, options)
    return sipx.PARSDMM(m.copy(), AtA, TD_OP, set_Prop, P_sub, comp_grid, options)


def report(name, x, log, clean, m, g_of):
    g, truth = g_of(x).astype(np.float64), g_of(clean).astype(np.float64)
    edges = truth > 0
    print("%-28s %3d iterations, rel. error %.4f (noisy: %.4f), edge pixels: %4d (clean: %d), contrast kept across the true edges: %.0f %%"
          % (name, len(log.obj), np.linalg.norm(x - clean) / np.linalg.norm(clean), np.linalg.norm(m - clean) / np.linalg.norm(clean),
             int(np.count_nonzero(g > 1e-3 * g.max())), int(edges.sum()), 100.0 * g[edges].sum() / truth[edges].sum()))


# ---- one image ---------------------------------------------------------------------------------------------------------------------------------
disc, rect = shapes(n)
clean = np.full(n, 0.4, TF)
clean[disc], clean[rect] = 0.9, 0.0
clean = clean.reshape(-1, order="F")
m = (clean + 0.02 * rng.standard_normal(clean.size)).astype(TF)
comp_grid = sipx.compgrid((TF(1.0), TF(1.0)), n)
bounds = sipx.set_definitions("bounds", "identity", 0.0, 1.0, ("matrix", ""))
g_of = lambda x: sipx.tv_group_norms(x, comp_grid, "TV")
k = int(np.count_nonzero(g_of(clean)))
g_noisy = np.sort(g_of(m))[::-1]
print("sorted gradient norms of the noisy image around the k-th place (k = %d): ... %s | %s ..." % (
    k, " ".join("%.3f" % v for v in g_noisy[k - 3:k]), " ".join("%.3f" % v for v in g_noisy[k:k + 3])))
x, log, _, _ = solve(m, [bounds, sipx.set_definitions("l20", "TV", 0, k, ("matrix", ""))], comp_grid)
report("l20 on TV, k = %d" % k, x, log, clean, m, g_of)
tau = float(sipx.l21_norm(clean, comp_grid, "TV"))
x, log, _, _ = solve(m, [bounds, sipx.set_definitions("l21", "TV", 0.0, tau, ("matrix", ""))], comp_grid)
report("l21 on TV, tau of the truth", x, log, clean, m, g_of)

# ---- three frames, one edge set ------------------------------------------------------------------------------------------------------------------
n3 = n + (3,)
stack = np.full(n3, 0.4, TF)
for f, (a, b) in enumerate([(0.9, 0.0), (0.7, 0.15), (0.6, 0.1)]):
    stack[disc, f], stack[rect, f] = a, b
stack = stack.reshape(-1, order="F")
m3 = (stack + 0.02 * rng.standard_normal(stack.size)).astype(TF)
grid3 = sipx.compgrid((TF(1.0), TF(1.0), TF(1.0)), n3)
g_joint = lambda x: sipx.tv_group_norms(x, grid3, "TV_xy", joint=True)
kj = int(np.count_nonzero(g_joint(stack)))
x, log, _, _ = solve(m3, [sipx.set_definitions("bounds", "identity", 0.0, 1.0, ("tensor", "")),
                          sipx.set_definitions("l20_joint", "TV_xy", 0, kj, ("tensor", ""))], grid3)
report("l20_joint on TV_xy, k = %d" % kj, x, log, stack, m3, g_joint)
