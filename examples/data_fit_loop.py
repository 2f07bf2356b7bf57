"""The loop of the reference's application examples on the MI355X engine, on synthetic images: learn constraint values from
training images, build ONE list of sets, then project image after image through it -- between images only the data-fit box
LBD <= x <= UBD around the current observation changes (examples/Indonesia_desaturation/
image_desaturation_by_constraint_learning.jl:204-270: P_sub[end] = x -> project_bounds!(x, LBD, UBD), warm start x_ini and y).
Here the list lives in one context (sipx.Solver) and Solver.set_data replaces the two bound vectors in place.

    python examples/data_fit_loop.py [n=128] [images=6]          (needs the built library and a GPU)
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

H = (1.0, 1.0)
CLIP_QUANTILE = 0.85      # the observations are saturated above this quantile of their grey values


def synthetic_images(count, n, TF, seed=0):
    """count images (count, n1, n2) with grey values in [0, 255]: a few smooth blobs on a ramp, a little texture."""
    rng = np.random.default_rng(1000 + seed)
    a, b = np.meshgrid(np.linspace(0, 1, n[0]), np.linspace(0, 1, n[1]), indexing="ij")
    out = np.empty((count,) + tuple(n), TF)
    for i in range(count):
        img = 60.0 + 80.0 * (a * rng.uniform(0.2, 1.0) + b * rng.uniform(0.2, 1.0))
        for _ in range(5):
            ca, cb, w = rng.uniform(0, 1), rng.uniform(0, 1), rng.uniform(0.05, 0.25)
            img += rng.uniform(20, 70) * np.exp(-((a - ca) ** 2 + (b - cb) ** 2) / (2 * w * w))
        img += 3.0 * rng.standard_normal(n)
        out[i] = np.clip(img, 0.0, 255.0)
    return out


def learned_constraints(mod, o, TF):
    """The desaturation example's list from the learned statistics (:150-200): bounds, relaxed histogram, and the median of
    the nuclear norm, TV, the l2 norm of the gradient and the l1 norm of the DFT over the training images."""
    q = lambda k: float(np.quantile(o[k].astype(np.float64), 0.5))
    return [mod.set_definitions("bounds", "identity", 0.0, 255.0, ("matrix", "")),
            mod.set_definitions("histogram", "identity", o["hist_min"].astype(TF), o["hist_max"].astype(TF), ("matrix", "")),
            mod.set_definitions("nuclear", "identity", 0.0, q("nuclear_norm"), ("matrix", "")),
            mod.set_definitions("l1", "TV", 0.0, q("TV"), ("matrix", "")),
            mod.set_definitions("l2", "TV", 0.0, q("D_l2"), ("matrix", "")),
            mod.set_definitions("l1", "DFT", 0.0, q("DFT_l1"), ("matrix", ""))]


def observe(img, TF):
    """A saturated observation of an image and what the example makes of it (:218-236): the data-fit box LBD <= x <= UBD
    (two grey values around the data, open to 255 where the sensor clipped) and the start x_ini."""
    data = img.reshape(-1, order="F").astype(TF)
    clip = TF(np.quantile(data, CLIP_QUANTILE))
    sat = data >= clip
    data = np.minimum(data, clip)
    lbd, ubd = (data - TF(2.0)).astype(TF), (data + TF(2.0)).astype(TF)
    ubd[sat] = TF(255.0)
    x_ini = data.copy()
    x_ini[sat] = TF(225.0)
    return data, lbd, ubd, x_ini, sat


def build_problem(sipx, n, TF, n_train=16, maxit=60, seed=0):
    """-> (AtA, TD_OP, set_Prop, P_sub, comp_grid, options), index of the data-fit set: learned list + a placeholder box."""
    g = sipx.compgrid(H, n)
    o = sipx.constraint_learning_by_obseration(g, synthetic_images(n_train, n, TF, seed),
                                               keys=("hist_min", "hist_max", "nuclear_norm", "TV", "D_l2", "DFT_l1"))
    N = n[0] * n[1]
    c = learned_constraints(sipx, o, TF)
    c.append(sipx.set_definitions("bounds", "identity", np.zeros(N, TF), np.full(N, 255.0, TF), ("matrix", "")))
    opt = sipx.PARSDMM_options(FL=TF, maxit=maxit, zero_ini_guess=False)
    P, A, prop = sipx.setup_constraints(c, g, TF)
    A, AtA, _, _ = sipx.PARSDMM_precompute_distribute(A, prop, g, opt)
    return (AtA, A, prop, P, g, opt), len(c) - 1


def main(n=128, count=6):
    sipx = load_package()
    TF = np.float32
    n = (n, n)
    problem, i_data = build_problem(sipx, n, TF)
    TD_OP = problem[1]
    truth = synthetic_images(count, n, TF, seed=1)
    y = None
    print(f"{count} saturated {n[0]} x {n[1]} images through one context; the data-fit box is set {i_data} of {i_data + 1}")
    with sipx.Solver(*problem, TF) as S:
        for k in range(count):
            data, lbd, ubd, x_ini, sat = observe(truth[k], TF)
            if y is None:
                y = [A @ x_ini for A in TD_OP]          # the example's first start (:247)
            t0 = time.perf_counter()
            S.set_data(i_data, lbd, ubd)
            x, log, _, y = S(x_ini.copy(), x_ini.copy(), None, y)      # p2proj = deepcopy(x_ini) (:250)
            dt = time.perf_counter() - t0
            print(f"  image {k}: {dt * 1e3:7.1f} ms ({'reset' if log.context_reused else 'build'} {log.timing['initialization'] * 1e3:6.1f} ms), "
                  f"{len(log.obj):3d} iterations, {int(sat.sum())} saturated pixels, largest set infeasibility at the end "
                  f"{float(np.max(log.set_feasibility[-1])):.2e}, x in [{float(x.min()):.1f}, {float(x.max()):.1f}]")
    return 0


if __name__ == "__main__":
    kv = dict(a.split("=", 1) for a in sys.argv[1:])
    sys.exit(main(int(kv.get("n", 128)), int(kv.get("images", 6))))
