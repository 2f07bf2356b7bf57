"""Time of one projection onto the weighted l1 ball on the TV operator (csrc/l1_weighted.h, csrc/ext_group.hip: L1WProj) next to the
weighted ("l21", "TV") set and the plain ("l1", "TV") set, same build, same run.

    python tools/l1_weighted_bench.py [--size 256,256,256] [--steps 10] [--rounds 3] [--out FILE]

Float32.  Six contexts, {bounds, the set}: the weighted l1 ball with four weight families over the rows of TV (just under 3 N) -- all ones,
1 / (1 + |heavy-tailed|), 30 % zeros with the rest in [0.5, 2], exp(3 randn) --, the weighted l2,1 ball with the edge family over the N
grid points, and the plain l1 ball; each inside a PARSDMM solve so that the projector sees the vectors a user's solve hands it; tau =
half the (weighted) norm of TV m.  After a warm-up window the contexts are measured in alternating windows of `steps` iterations with
the engine's device events around every launch (sipx_kernel_stats mode 2); per figure the median over the windows with the spread.
Figures per weighted l1 set:
    ms_per_projection   the row "ext_proj (library-backed)" per launch (the passes with the host's reads of the flag between the
                        batches, the apply) plus "k_pass<M_STORE>", the pass that materialises v in front of it
    passes              Michelot passes of the last projection of the window, the first included (kernel_stats: l1_weighted)
    pass_ms             the row k_l1w_part per projection divided by the passes (launches that return at once because the iteration is
                        done are in the row too: a few microseconds each); a pass reads 2 * 3 N words
    apply_ms            k_l1w_apply per launch: reads 2 * 3 N words, writes 3 N
    pass_bytes, apply_bytes   the bytes booked per launch of the two rows
The weighted l2,1 set reports ms_per_projection and passes alike (kernel_stats: l21_weighted); the plain l1 set, whose search and
apply run inside the engine's own update, reports ms_per_iteration of the whole solve step instead (wall clock around the window) --
as do all sets, so that the three can be compared on one figure.
Needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROW, STORE, PASS, APPLY = "ext_proj (library-backed)", "k_pass<M_STORE>", "k_l1w_part", "k_l1w_apply"
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
    M = sipx.TDOperator("TV", g, TF).shape[0]
    opt = sipx.PARSDMM_options(FL=TF, maxit=a.steps * (a.rounds + 1), evol_rel_tol=0.0, feas_tol=0.0, obj_tol=0.0)
    sets = {}
    for fam in FAMILIES:
        w = weights(fam, rng, M, TF)
        sets["l1_weighted/" + fam] = sipx.set_definitions("l1_weighted", "TV", 0.0, 0.5 * float(sipx.l1_weighted_norm(m, g, "TV", w)), mode,
                                                          weights=w)
    w = weights("edge", rng, N, TF)
    sets["l21_weighted/edge"] = sipx.set_definitions("l21", "TV", 0.0, 0.5 * float(sipx.l21_norm(m, g, "TV", weights=w)), mode, weights=w)
    sets["l1"] = sipx.set_definitions("l1", "TV", 0.0, 0.5 * float(sipx.l1_weighted_norm(m, g, "TV", np.ones(M, TF))), mode)
    del w
    keys = ("ms", "iter_ms", "passes", "pass_ms", "apply_ms", "pass_bytes", "apply_bytes")
    ctxs, fig = {}, {name: {k: [] for k in keys} for name in sets}
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
                t0 = time.perf_counter()
                ctx.parsdmm_steps(a.steps)
                wall = time.perf_counter() - t0
                st = ctx.kernel_stats_all(0)
                ks = {k["name"]: k for k in st["kernels"]}
                f = fig[name]
                f["iter_ms"].append(1e3 * wall / a.steps)      # (mode 2 times one kernel at a time: comparable between the sets only)
                if name == "l1":
                    continue
                ext, store = ks.get(ROW), ks.get(STORE)
                if not ext or not ext["launches"] or not store or not store["launches"]:
                    raise RuntimeError("no projector call was recorded")
                f["ms"].append(ext["total_ms"] / ext["launches"] + store["total_ms"] / store["launches"])
                if name.startswith("l21"):
                    f["passes"].append(st["l21_weighted"]["passes"])
                    continue
                passes = st["l1_weighted"]["passes"]
                f["passes"].append(passes)
                f["pass_ms"].append(ks[PASS]["total_ms"] / ext["launches"] / passes)
                f["apply_ms"].append(ks[APPLY]["total_ms"] / ks[APPLY]["launches"])
                f["pass_bytes"].append(ks[PASS]["bytes_moved"] / ks[PASS]["launches"])
                f["apply_bytes"].append(ks[APPLY]["bytes_moved"] / ks[APPLY]["launches"])
    finally:
        for ctx in ctxs.values():
            ctx.close()

    def stat(v, nd=4):
        return {"median": round(float(np.median(v)), nd), "min": round(float(min(v)), nd), "max": round(float(max(v)), nd)}
    res = {"n": list(n), "rows": M, "dtype": "float32", "steps_per_window": a.steps, "windows": a.rounds, "sets": {}}
    for name, f in fig.items():
        r = {"ms_per_iteration": stat(f["iter_ms"])}
        if f["ms"]:
            r["ms_per_projection"] = stat(f["ms"])
            r["passes"] = stat(f["passes"], 0)
        if f["pass_ms"]:
            r["pass_ms"] = stat(f["pass_ms"])
            r["apply_ms"] = stat(f["apply_ms"])
            r["pass_bytes"] = int(np.median(f["pass_bytes"]))
            r["apply_bytes"] = int(np.median(f["apply_bytes"]))
            r["pass_GBps"] = round(r["pass_bytes"] / (r["pass_ms"]["median"] * 1e-3) / 1e9, 1)
            r["apply_GBps"] = round(r["apply_bytes"] / (r["apply_ms"]["median"] * 1e-3) / 1e9, 1)
        res["sets"][name] = r
    txt = json.dumps(res)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
