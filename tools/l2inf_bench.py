"""Time of one projection onto the l2,inf ball (csrc/l2inf.h) next to the l2,1 ball on the same operator, same build: the one-sweep
clip kernel against the norms and scale kernels it replaces, and the whole materialised projector with and without a threshold search.

    python tools/l2inf_bench.py [--size 2048,2048] [--steps 10] [--rounds 3] [--out FILE]

Float32.  Four contexts -- {bounds, l2inf on TV}, {bounds, l21 on TV}, {bounds, l2inf on Hessian}, {bounds, l21 on Hessian} -- each
inside a PARSDMM solve so that the projector sees the vectors a user's solve hands it; the l2inf bound is half the observed maximum
(sipx.l2inf_norm), the l21 radius half the observed norm.  After a warm-up window the contexts are measured in alternating windows of
`steps` iterations with the engine's device events around every launch (sipx_kernel_stats mode 2); per figure the median over the
windows with the spread.  Figures (w = 4 bytes, G = N groups, b = nblk blocks of TV or B of the Hessian):
    <op>_clip_ms                  k_l2inf_clip (tv) / k_l2infs_clip (hessian) per launch; _TB_per_s: 2 b G w over it, the traffic of a
                                  call that clips everywhere (a scalar bound reads no vector; where nothing is clipped nothing is stored)
    <op>_norms_ms, <op>_scale_ms  k_l21_norms / k_l21_scale (k_l21s_norms / k_l21s_scale) per launch, the yardstick: (b + 1) G w and
                                  (2 b + 1) G w; <op>_l21_kernels_ms their sum
    <op>_clip_over_l21_kernels    the ratio of the two; by traffic at most 2 b / (3 b + 2)
    <op>_l2inf_ext_ms, <op>_l21_ext_ms   the whole materialised projector in the y/l update (the row "ext_proj (library-backed)")
                                  per call: what the absent search saves
Needs a GPU."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLIP = {"tv": "k_l2inf_clip", "hessian": "k_l2infs_clip"}
L21 = {"tv": ("k_l21_norms", "k_l21_scale"), "hessian": ("k_l21s_norms", "k_l21s_scale")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="2048,2048")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--ops", default="tv,hessian")
    a = ap.parse_args()
    from __graft_entry__ import load_package
    sipx = load_package()
    TF = np.float32
    n = tuple(int(v) for v in a.size.split(","))
    N, nblk = int(np.prod(n)), len(n)
    B = nblk * (nblk + 1) // 2
    mode = ("matrix", "") if nblk == 2 else ("tensor", "")
    rng = np.random.default_rng(0)
    z = np.linspace(0, 1, n[-1]).reshape((1,) * (len(n) - 1) + (-1,))
    m = (1500 + 2500 * z + 150 * rng.standard_normal(n)).astype(TF).reshape(-1, order="F")
    g = sipx.compgrid((25.0,) * len(n), n)
    opt = sipx.PARSDMM_options(FL=TF, maxit=a.steps * (a.rounds + 1), evol_rel_tol=0.0, feas_tol=0.0, obj_tol=0.0)
    ops = [o for o in a.ops.split(",") if o]
    sets = {}
    if "tv" in ops:
        sets["tv_l2inf"] = sipx.set_definitions("l2inf", "TV", 0, 0.5 * float(sipx.l2inf_norm(m, g, "TV")), mode)
        sets["tv_l21"] = sipx.set_definitions("l21", "TV", 0.0, 0.5 * float(sipx.l21_norm(m, g)), mode)
    if "hessian" in ops:
        sets["hessian_l2inf"] = sipx.set_definitions("l2inf", "Hessian", 0, 0.5 * float(sipx.l2inf_norm(m, g, "Hessian")), mode)
        sets["hessian_l21"] = sipx.set_definitions("l21", "Hessian", 0.0, 0.5 * float(sipx.l21_stacked_norm(m, g, "Hessian")), mode)
    ctxs, fig = {}, {}
    try:
        for name, c in sets.items():
            P, A, prop = sipx.setup_constraints([sipx.set_definitions("bounds", "identity", 1600.0, 3900.0, mode), c], g, TF)
            A, AtA, _, _ = sipx.PARSDMM_precompute_distribute(A, prop, g, opt)
            ctx = ctxs[name] = sipx.host.build_context(m, AtA, A, prop, P, g, opt)
            ctx.parsdmm_begin(opt)
            ctx.parsdmm_steps(a.steps)                      # warm-up
        for _ in range(a.rounds):
            for name, ctx in ctxs.items():
                op, kind = name.split("_")
                ctx.kernel_stats(2)
                ctx.parsdmm_steps(a.steps)
                ks = {k["name"]: k for k in ctx.kernel_stats_all(0)["kernels"]}
                rows = {"clip": CLIP[op]} if kind == "l2inf" else dict(zip(("norms", "scale"), L21[op]))
                for what, row in rows.items():
                    k = ks.get(row)
                    if not k or not k["launches"]:
                        raise RuntimeError(f"no launch of {row} was recorded")
                    fig.setdefault(f"{op}_{what}_ms", []).append(k["total_ms"] / k["launches"])
                ext = ks["ext_proj (library-backed)"]
                fig.setdefault(f"{name}_ext_ms", []).append(ext["total_ms"] / ext["launches"])
    finally:
        for ctx in ctxs.values():
            ctx.close()

    def stat(v, nd=4):
        return {"median": round(float(np.median(v)), nd), "min": round(float(min(v)), nd), "max": round(float(max(v)), nd)}

    def tbs(words, ms):
        return round(words * 4 / (ms * 1e-3) / 1e12, 3)
    res = {"n": list(n), "dtype": "float32", "steps_per_window": a.steps, "windows": a.rounds, "groups": N}
    for op, b in (("tv", nblk), ("hessian", B)):
        if op not in ops:
            continue
        tc, tn, ts = (float(np.median(fig[f"{op}_{w}_ms"])) for w in ("clip", "norms", "scale"))
        res[f"{op}_blocks"] = b
        for w in ("clip", "norms", "scale"):
            res[f"{op}_{w}_ms"] = stat(fig[f"{op}_{w}_ms"])
        res[f"{op}_clip_TB_per_s"] = tbs(2 * b * N, tc)
        res[f"{op}_norms_TB_per_s"], res[f"{op}_scale_TB_per_s"] = tbs((b + 1) * N, tn), tbs((2 * b + 1) * N, ts)
        res[f"{op}_l21_kernels_ms"] = round(tn + ts, 4)
        res[f"{op}_clip_over_l21_kernels"] = round(tc / (tn + ts), 4)
        res[f"{op}_traffic_ratio"] = round(2 * b / (3 * b + 2), 4)
        res[f"{op}_l2inf_ext_ms"], res[f"{op}_l21_ext_ms"] = stat(fig[f"{op}_l2inf_ext_ms"]), stat(fig[f"{op}_l21_ext_ms"])
    txt = json.dumps(res)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
