"""At most k traces change: group cardinality on a time lapse.

`("card_groups", "D_z", 0, k, ("fiber", "z"))` says that at most k pixels of an (x, y, frame) stack change over time at all -- k is what
one knows ("twelve wells", "these few injection points"), where the convex set `("l21_groups", "D_z", ("fiber", "z"))` asks for a
radius tau that nobody knows in advance and shrinks every trace it lets through.

A synthetic stack -- a static background in which k = 12 scattered pixels step by a different amount at a different frame each -- is
observed with noise and projected onto

  1. {bounds, card_groups with the true k}, and
  2. {bounds, l21_groups with the radius of the truth} (sipx.l21_groups_norm of the clean stack),

and both are compared with the clean stack: the error, the traces found to change (sipx.group_norms, the array the projector selects
on) and how much of the true steps survives.

    python examples/sparse_changes_frames.py            (needs the built library and a GPU)
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
k = 12

rng = np.random.default_rng(0)
clean = np.full(n, 0.5, TF)
pixels = rng.choice(n[0] * n[1], k, replace=False)
for p in pixels:
    clean[p % n[0], p // n[0], int(rng.integers(3, n[2] - 3)):] += TF(rng.uniform(0.25, 0.5))
clean = clean.reshape(-1, order="F")
m = (clean + 0.02 * rng.standard_normal(N)).astype(TF)

comp_grid = sipx.compgrid((TF(1.0), TF(1.0), TF(1.0)), n)
options = sipx.PARSDMM_options(FL=TF, maxit=300)
mode = ("fiber", "z")


def solve(c):
    constraint = [sipx.set_definitions("bounds", "identity", 0.0, 1.5, ("tensor", "")), c]
    P_sub, TD_OP, set_Prop = sipx.setup_constraints(constraint, comp_grid, TF)
    TD_OP, AtA, _, _ = sipx.PARSDMM_precompute_distribute(TD_OP, set_Prop, comp_grid, options)
    return sipx.PARSDMM(m.copy(), AtA, TD_OP, set_Prop, P_sub, comp_grid, options)


def report(name, x, log):
    g = sipx.group_norms(x, comp_grid, "D_z", mode).astype(np.float64)
    truth = sipx.group_norms(clean, comp_grid, "D_z", mode).astype(np.float64)
    found = set(np.flatnonzero(g > 1e-3 * g.max()).tolist())
    print("%-28s %3d iterations, rel. error %.4f (noisy: %.4f), changing traces: %3d (true ones among them: %2d of %d), "
          "step height kept: %.0f %%" % (name, len(log.obj), np.linalg.norm(x - clean) / np.linalg.norm(clean),
                                        np.linalg.norm(m - clean) / np.linalg.norm(clean), len(found), len(found & set(pixels.tolist())), k,
                                        100.0 * g[pixels].sum() / truth[pixels].sum()))


g_noisy = np.sort(sipx.group_norms(m, comp_grid, "D_z", mode))[::-1]
print("sorted trace norms of the noisy stack around the k-th place: ... %s | %s ..." % (
    " ".join("%.3f" % v for v in g_noisy[k - 3:k]), " ".join("%.3f" % v for v in g_noisy[k:k + 3])))
x, log, _, _ = solve(sipx.set_definitions("card_groups", "D_z", 0, k, mode))
report("card_groups, k = %d" % k, x, log)
tau = float(sipx.l21_groups_norm(clean, comp_grid, "D_z", mode))
x, log, _, _ = solve(sipx.set_definitions("l21_groups", "D_z", 0.0, tau, mode))
report("l21_groups, tau of the truth", x, log)
