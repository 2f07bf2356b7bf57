"""Time of one projection onto the weighted l2,1 ball on the TV operator (csrc/l21_weighted.h, csrc/ext_group.hip) next to the
unweighted ("l21", "TV") set, same build, same run.

    python tools/l21_weighted_bench.py [--size 256,256,256] [--steps 10] [--rounds 3] [--out FILE]

Float32.  Five contexts, {bounds, the set}: the unweighted ball, and the weighted one with four weight families -- all ones,
1 / (1 + |heavy-tailed|), 30 % zeros with the rest in [0.5, 2], exp(3 randn) -- each inside a PARSDMM solve so that the projector sees
the vectors a user's solve hands it; tau = half the (weighted) norm of TV m.  After a warm-up window the contexts are measured in
alternating windows of `steps` iterations with the engine's device events around every launch (sipx_kernel_stats mode 2); per figure
the median over the windows with the spread.  Figures per set:
    ms_per_projection   the row "ext_proj (library-backed)" per launch (norms, the passes with the host's reads of the flag between
                        the batches, the scale) plus "k_pass<M_STORE>", the pass that materialises v in front of it
    passes              Michelot passes of the last projection of the window, the first included (kernel_stats: l21_weighted)
    norms_ms            k_l21_norms per launch: what a pass is compared with -- a pass reads 2 n words, the norms launch reads 3 n and
                        writes n
    pass_ms             the row k_l21w_part per projection divided by the passes (launches that return at once because the iteration
                        is done are in the row too: a few microseconds each)
Needs a GPU."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROW, STORE, NORMS, PASS = "ext_proj (library-backed)", "k_pass<M_STORE>", "k_l21_norms", "k_l21w_part"
FAMILIES = ("ones", "edge", "masked", "lognormal")


def weights(family, rng, n, TF):
    if family == "ones":
        return np.ones(n, TF)
    if family == "edge":
        return (1.0 / (1.0 + np.abs(rng.standard_normal(n) * np.exp(rng.standard_normal(n))))).astype(TF)
    if family == "masked":
        w = rng.uniform(0.5, 2.0, n)
        w[rng.random(n) < 0.3] = 0.0
        return w.astype(TF)
    return np.exp(3.0 * rng.standard_normal(n)).astype(TF)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="256,256,256")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from __graft_entry__ import load_package
    sipx = load_package()
    TF = np.float32
    n = tuple(int(v) for v in a.size.split(","))
    N = int(np.prod(n))
    mode = ("matrix", "") if len(n) == 2 else ("tensor", "")
    rng = np.random.default_rng(0)
    z = np.linspace(0, 1, n[-1]).reshape((1,) * (len(n) - 1) + (-1,))
    m = (1500 + 2500 * z + 150 * rng.standard_normal(n)).astype(TF).reshape(-1, order="F")
    g = sipx.compgrid((25.0,) * len(n), n)
    opt = sipx.PARSDMM_options(FL=TF, maxit=a.steps * (a.rounds + 1), evol_rel_tol=0.0, feas_tol=0.0, obj_tol=0.0)
    sets = {"unweighted": sipx.set_definitions("l21", "TV", 0.0, 0.5 * float(sipx.l21_norm(m, g)), mode)}
    for fam in FAMILIES:
        w = weights(fam, rng, N, TF)
        sets[fam] = sipx.set_definitions("l21", "TV", 0.0, 0.5 * float(sipx.l21_norm(m, g, "TV", weights=w)), mode, weights=w)
    ctxs, fig = {}, {name: {"ms": [], "passes": [], "norms_ms": [], "pass_ms": []} for name in sets}
    try:
        for name, c in sets.items():
            P, A, prop = sipx.setup_constraints([sipx.set_definitions("bounds", "identity", 1600.0, 3900.0, mode), c], g, TF)
            A, AtA, _, _ = sipx.PARSDMM_precompute_distribute(A, prop, g, opt)
            ctx = ctxs[name] = sipx.host.build_context(m, AtA, A, prop, P, g, opt)
            ctx.parsdmm_begin(opt)
            ctx.parsdmm_steps(a.steps)                      # warm-up
        for _ in range(a.rounds):
            for name, ctx in ctxs.items():
                ctx.kernel_stats(2)
                ctx.parsdmm_steps(a.steps)
                st = ctx.kernel_stats_all(0)
                ks = {k["name"]: k for k in st["kernels"]}
                ext, store, nrm = ks.get(ROW), ks.get(STORE), ks.get(NORMS)
                if not ext or not ext["launches"] or not store or not store["launches"] or not nrm or not nrm["launches"]:
                    raise RuntimeError("no projector call was recorded")
                f = fig[name]
                f["ms"].append(ext["total_ms"] / ext["launches"] + store["total_ms"] / store["launches"])
                f["norms_ms"].append(nrm["total_ms"] / nrm["launches"])
                if name != "unweighted":
                    passes = st["l21_weighted"]["passes"]
                    f["passes"].append(passes)
                    f["pass_ms"].append(ks[PASS]["total_ms"] / nrm["launches"] / passes)
    finally:
        for ctx in ctxs.values():
            ctx.close()

    def stat(v, nd=4):
        return {"median": round(float(np.median(v)), nd), "min": round(float(min(v)), nd), "max": round(float(max(v)), nd)}
    res = {"n": list(n), "dtype": "float32", "steps_per_window": a.steps, "windows": a.rounds, "sets": {}}
    for name, f in fig.items():
        r = {"ms_per_projection": stat(f["ms"]), "norms_ms": stat(f["norms_ms"])}
        if f["passes"]:
            r["passes"] = stat(f["passes"], 0)
            r["pass_ms"] = stat(f["pass_ms"])
            r["pass_over_norms"] = round(float(np.median(f["pass_ms"])) / float(np.median(f["norms_ms"])), 3)
        res["sets"][name] = r
    txt = json.dumps(res)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
