"""Time of one projection onto the l2,1 ball on the Hessian (second-order isotropic TV, csrc/l21_stacked.h) next to the l2,1 ball on the
TV operator, same build, and the time the Hessian's operator products take beside it.

    python tools/l21_stacked_bench.py [--size 2048,2048] [--steps 10] [--rounds 3] [--out FILE]

Float32.  Two contexts, {bounds, l21 on Hessian} and {bounds, l21 on TV}, each inside a PARSDMM solve so that the projector sees the
vectors a user's solve hands it; both radii are half the observed norm.  After a warm-up window the contexts are measured in
alternating windows of `steps` iterations with the engine's device events around every launch (sipx_kernel_stats mode 2); per figure
the median over the windows with the spread.  Figures (w = 4 bytes, G = N groups, B = 3 or 6 blocks, nblk = 2 or 3):
    hessian_norms_ms, hessian_scale_ms    k_l21s_norms / k_l21s_scale per launch; _TB_per_s: (B + 1) G w and (2 B + 1) G w over them
    hessian_kernels_ms                    their sum = the two new kernels per projection; hessian_kernels_TB_per_s: (2 B + 1) G w over it
    tv_norms_ms, tv_scale_ms, tv_kernels_ms, ..._TB_per_s: the same for k_l21_norms / k_l21_scale with nblk in place of B -- the
                                          yardstick: the same launches on the same grid, the traffic ratio is (2 B + 1) / (2 nblk + 1)
    hessian_ext_ms                        the whole materialised projector in the y/l update (the row "ext_proj (library-backed)": norms,
                                          search, scale) per call
    hessian_mf_fwd_ms_per_iteration, hessian_mf_adj_ms_per_iteration
                                          all launches of k_mf_fwd / k_mf_adj of an iteration: s = H x of the set's update and of the
                                          feasibility estimate, H'(rho y + l) of the right-hand side, the adjoint norm, and the
                                          matrix-free term of Q in every CG product (the Hessian's A'A has more bands than a set
                                          hands over); with the launches per iteration
Needs a GPU."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = {"hessian": ("k_l21s_norms", "k_l21s_scale"), "tv": ("k_l21_norms", "k_l21_scale")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="2048,2048")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
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
    maxit = a.steps * (a.rounds + 1)
    opt = sipx.PARSDMM_options(FL=TF, maxit=maxit, evol_rel_tol=0.0, feas_tol=0.0, obj_tol=0.0)
    sets = {        # radii: half the respective observed norm
        "hessian": sipx.set_definitions("l21", "Hessian", 0.0, 0.5 * float(sipx.l21_stacked_norm(m, g, "Hessian")), mode),
        "tv": sipx.set_definitions("l21", "TV", 0.0, 0.5 * float(sipx.l21_norm(m, g)), mode),
    }
    ctxs = {}
    fig = {k: [] for k in ("hessian_norms_ms", "hessian_scale_ms", "tv_norms_ms", "tv_scale_ms", "hessian_ext_ms", "tv_ext_ms",
                           "hessian_mf_fwd_ms_per_iteration", "hessian_mf_adj_ms_per_iteration", "hessian_mf_fwd_launches_per_iteration",
                           "hessian_mf_adj_launches_per_iteration", "hessian_iteration_ms", "tv_iteration_ms")}
    try:
        for name, c in sets.items():
            P, A, prop = sipx.setup_constraints([sipx.set_definitions("bounds", "identity", 1600.0, 3900.0, mode), c], g, TF)
            A, AtA, _, _ = sipx.PARSDMM_precompute_distribute(A, prop, g, opt)
            if name == "hessian" and AtA[1] is not None:
                raise RuntimeError("the Hessian was expected to enter Q matrix-free")
            ctx = ctxs[name] = sipx.host.build_context(m, AtA, A, prop, P, g, opt)
            ctx.parsdmm_begin(opt)
            ctx.parsdmm_steps(a.steps)                      # warm-up
        for _ in range(a.rounds):
            for name, ctx in ctxs.items():
                ctx.kernel_stats(2)
                ctx.parsdmm_steps(a.steps)
                ks = {k["name"]: k for k in ctx.kernel_stats_all(0)["kernels"]}
                for what, row in zip(("norms", "scale"), ROWS[name]):
                    k = ks.get(row)
                    if not k or not k["launches"]:
                        raise RuntimeError(f"no launch of {row} was recorded")
                    fig[f"{name}_{what}_ms"].append(k["total_ms"] / k["launches"])
                ext = ks["ext_proj (library-backed)"]
                fig[f"{name}_ext_ms"].append(ext["total_ms"] / ext["launches"])
                fig[f"{name}_iteration_ms"].append(sum(k["total_ms"] for nm, k in ks.items() if nm != "ext_proj (library-backed)") / a.steps)
                if name == "hessian":
                    for what, row in (("fwd", "k_mf_fwd"), ("adj", "k_mf_adj")):
                        fig[f"hessian_mf_{what}_ms_per_iteration"].append(ks[row]["total_ms"] / a.steps)
                        fig[f"hessian_mf_{what}_launches_per_iteration"].append(ks[row]["launches"] / a.steps)
    finally:
        for ctx in ctxs.values():
            ctx.close()

    def stat(v, nd=4):
        return {"median": round(float(np.median(v)), nd), "min": round(float(min(v)), nd), "max": round(float(max(v)), nd)}

    def tbs(words, ms):
        return round(words * 4 / (ms * 1e-3) / 1e12, 3)
    res = {"n": list(n), "dtype": "float32", "steps_per_window": a.steps, "windows": a.rounds, "blocks": B, "groups": N}
    for name, b in (("hessian", B), ("tv", nblk)):
        tn, ts = float(np.median(fig[f"{name}_norms_ms"])), float(np.median(fig[f"{name}_scale_ms"]))
        res[f"{name}_norms_ms"], res[f"{name}_scale_ms"] = stat(fig[f"{name}_norms_ms"]), stat(fig[f"{name}_scale_ms"])
        res[f"{name}_norms_TB_per_s"], res[f"{name}_scale_TB_per_s"] = tbs((b + 1) * N, tn), tbs((2 * b + 1) * N, ts)
        res[f"{name}_kernels_ms"] = round(tn + ts, 4)
        res[f"{name}_kernels_TB_per_s"] = tbs((2 * b + 1) * N, tn + ts)
        res[f"{name}_ext_ms"] = stat(fig[f"{name}_ext_ms"])
        res[f"{name}_iteration_ms"] = stat(fig[f"{name}_iteration_ms"])
    res["traffic_ratio"] = round((2 * B + 1) / (2 * nblk + 1), 4)
    res["tv_kernels_ms_scaled_by_traffic"] = round(res["tv_kernels_ms"] * (2 * B + 1) / (2 * nblk + 1), 4)
    for k in ("hessian_mf_fwd_ms_per_iteration", "hessian_mf_adj_ms_per_iteration", "hessian_mf_fwd_launches_per_iteration",
              "hessian_mf_adj_launches_per_iteration"):
        res[k] = stat(fig[k])
    txt = json.dumps(res)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
