"""Time of one projection onto the total-nuclear-variation ball (csrc/tnv.h, csrc/ext_group.hip: TnvProj) next to the joint l2,1 ball on the
same operator (csrc/l21_joint.h, BallProj), same build, same run.

    python tools/tnv_bench.py [--size 256,256,64] [--steps 10] [--rounds 3] [--out FILE]

Float32.  Two contexts, each inside a PARSDMM solve of {bounds, the set} so that the projector sees the vectors a user's solve hands it;
radius: half of the array's own norm of A m.
    tnv      ("tnv", "TV_xy", ("tensor", "")): a 2 x 2 Gram matrix per pixel, the threshold search on 2 n1 n2 singular values
    joint    ("l21_joint", "TV_xy", ("tensor", "")): a sum of squares per pixel, the threshold search on n1 n2 norms
After a warm-up window the contexts are measured in alternating windows of `steps` iterations with the engine's device events around
every launch (sipx_kernel_stats mode 2); per figure the median over the windows with the spread.

The row "ext_proj (library-backed)" is a whole materialised projector in the y/l update and "k_pass<M_STORE>" the pass that
materialises v in front of it; ms_per_projection is their sum per launch.  The rows k_tnv_gram / k_tnv_finish / k_tnv_apply (tnv) and
k_l21j_norms / k_l21j_finish / k_l21j_scale (joint) are the kernels on their own, recorded inside the ext_proj row (and by the feasibility
estimate, which runs the same projector): ms per launch, and GB/s over the traffic of DESIGN.md section 7i -- the Gram march reads 2 N
words and writes 4 L, the apply kernel reads 2 N + 4 L and writes 2 N; the joint kernels as their launcher books them.  tnv moves
l21_joint's bytes plus a few L words, so tnv_over_joint is the figure to read: the joint set in the same run is the yardstick.  Needs a
GPU."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROW, STORE = "ext_proj (library-backed)", "k_pass<M_STORE>"
KERNELS = {"tnv": ("k_tnv_gram", "k_tnv_finish", "k_tnv_apply"), "joint": ("k_l21j_norms", "k_l21j_finish", "k_l21j_scale")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="256,256,64")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from __graft_entry__ import load_package
    sipx = load_package()
    TF = np.float32
    n = tuple(int(v) for v in a.size.split(","))
    rng = np.random.default_rng(0)
    z = np.linspace(0, 1, n[-1]).reshape((1, 1, -1))
    m = (1500 + 2500 * z + 150 * rng.standard_normal(n)).astype(TF).reshape(-1, order="F")
    g = sipx.compgrid((25.0,) * 3, n)
    opt = sipx.PARSDMM_options(FL=TF, maxit=a.steps * (a.rounds + 1), evol_rel_tol=0.0, feas_tol=0.0, obj_tol=0.0)
    bounds = sipx.set_definitions("bounds", "identity", 1600.0, 3900.0, ("tensor", ""))
    sets = {
        "tnv": sipx.set_definitions("tnv", "TV_xy", 0.0, 0.5 * float(sipx.tnv_norm(m, g)), ("tensor", "")),
        "joint": sipx.set_definitions("l21_joint", "TV_xy", 0.0, 0.5 * float(sipx.l21_joint_norm(m, g)), ("tensor", "")),
    }
    ctxs = {}
    fig = {name: {"ms": [], **{k: [] for k in KERNELS[name]}} for name in sets}
    gbs = {name: {k: [] for k in KERNELS[name]} for name in sets}
    try:
        for name, c in sets.items():
            P, A, prop = sipx.setup_constraints([bounds, c], g, TF)
            A, AtA, _, _ = sipx.PARSDMM_precompute_distribute(A, prop, g, opt)
            ctx = ctxs[name] = sipx.host.build_context(m, AtA, A, prop, P, g, opt)
            ctx.parsdmm_begin(opt)
            ctx.parsdmm_steps(a.steps)                      # warm-up
        for _ in range(a.rounds):
            for name, ctx in ctxs.items():
                ctx.kernel_stats(2)
                ctx.parsdmm_steps(a.steps)
                ks = {k["name"]: k for k in ctx.kernel_stats_all(0)["kernels"]}
                ext, store = ks.get(ROW), ks.get(STORE)
                if not ext or not ext["launches"] or not store or not store["launches"]:
                    raise RuntimeError("no projector call was recorded")
                fig[name]["ms"].append(ext["total_ms"] / ext["launches"] + store["total_ms"] / store["launches"])
                for k in KERNELS[name]:
                    if k in ks and ks[k]["launches"]:
                        per = ks[k]["total_ms"] / ks[k]["launches"]
                        fig[name][k].append(per)
                        gbs[name][k].append(ks[k]["bytes_survey"] / ks[k]["launches"] / (per * 1e-3) / 1e9)
    finally:
        for ctx in ctxs.values():
            ctx.close()

    def stat(v, nd=4):
        return {"median": round(float(np.median(v)), nd), "min": round(float(min(v)), nd), "max": round(float(max(v)), nd)} if v else None
    res = {"n": list(n), "dtype": "float32", "steps_per_window": a.steps, "windows": a.rounds,
           "library": os.path.basename(sipx.LIB_PATH)}
    for name in sets:
        res[name + "_ms_per_projection"] = stat(fig[name]["ms"])
        for k in KERNELS[name]:
            if fig[name][k]:
                res[f"{name}_{k}_ms"] = stat(fig[name][k])
                res[f"{name}_{k}_GB_per_s"] = stat(gbs[name][k], 1)
    t, j = res["tnv_ms_per_projection"], res["joint_ms_per_projection"]
    res["tnv_over_joint"] = round(t["median"] / j["median"], 3)
    N, L = int(np.prod(n)), n[0] * n[1]
    res["tnv_bytes_per_projection"] = (2 * N + 4 * L + 4 * N + 4 * L) * 4      # Gram: 2 N read, 4 L written; apply: 2 N + 4 L read, 2 N written
    kern = sum(res[f"tnv_{k}_ms"]["median"] for k in KERNELS["tnv"] if f"tnv_{k}_ms" in res)
    res["tnv_kernels_GB_per_s"] = round(res["tnv_bytes_per_projection"] / (kern * 1e-3) / 1e9, 1)
    kj = sum(res[f"joint_{k}_ms"]["median"] for k in KERNELS["joint"] if f"joint_{k}_ms" in res)
    res["tnv_kernels_over_joint_kernels"] = round(kern / kj, 3)
    txt = json.dumps(res)
    print(txt)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
