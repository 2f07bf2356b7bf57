"""Time of one projection onto an l2,0 set on total variation (csrc/l20.h, csrc/ext_group.hip: L20Proj, L20FrameProj) against the l2,1
ball on the same operator, in the same run.

    python tools/l20_bench.py --case tv2d|tv3d|frames|joint [--size n1,n2[,n3]] [--steps 10] [--rounds 3] [--out FILE]

Float32, inside a PARSDMM solve of {bounds, the set} so that the projector sees the vectors a user's solve hands it, the engine's device
events around every launch (sipx_kernel_stats mode 2), a warm-up window, then `rounds` alternating windows of `steps` iterations; every
figure is the median over the windows with its spread [min, max].  The l2,0 set has k = a tenth of its groups, the l2,1 ball half the
observed norm of A m; same arrays.  The cases and their default sizes:
    tv2d    ("l20", "TV") on 2048 x 2048            against ("l21", "TV")
    tv3d    ("l20", "TV") on 256^3                  against ("l21", "TV")
    frames  ("l20", "TV_xy", ("slice", "z")) on 256 x 256 x 64    against ("l21", "TV_xy", ("slice", "z"))
    joint   ("l20_joint", "TV_xy") on 1024 x 1024 x 8             against ("l21_joint", "TV_xy")
Figures per set:
    ms_per_projection   the row "ext_proj (library-backed)" per launch: norms, selection, apply
    norms_ms, apply_ms  the rows k_l21_norms (joint: k_l21j_norms + k_l21j_finish), and k_l20_zero or k_l21_scale (k_l21j_scale), per launch
    frames_kernel_ms    the per-frame selection kernel, k_l20_frames or k_l21_frames, per launch
    select_ms           ms_per_projection - norms_ms - apply_ms: the selection with the gaps between its launches
Needs a GPU."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROW = "ext_proj (library-backed)"
NORMS = ("k_l21_norms", "k_l21j_norms", "k_l21j_finish")
APPLY = ("k_l20_zero", "k_l21_scale", "k_l21j_scale")
FRAMES = ("k_l20_frames", "k_l21_frames")
CASES = {"tv2d": ((2048, 2048), "TV", "whole"), "tv3d": ((256, 256, 256), "TV", "whole"), "frames": ((256, 256, 64), "TV_xy", "frames"),
         "joint": ((1024, 1024, 8), "TV_xy", "joint")}


def stat(v, nd=4):
    return {"median": round(float(np.median(v)), nd), "min": round(float(min(v)), nd), "max": round(float(max(v)), nd)}


def model(n, TF):
    rng = np.random.default_rng(0)
    z = np.linspace(0, 1, n[-1]).reshape((1,) * (len(n) - 1) + (-1,))
    return (1500 + 2500 * z + 150 * rng.standard_normal(n)).astype(TF).reshape(-1, order="F")


def measure(sipx, g, m, TF, sets, steps, rounds, whole):
    """sets: name -> set_definitions.  Returns name -> lists per window."""
    opt = sipx.PARSDMM_options(FL=TF, maxit=steps * (rounds + 1), evol_rel_tol=0.0, feas_tol=0.0, obj_tol=0.0)
    ctxs, fig = {}, {name: {"ms": [], "norms_ms": [], "apply_ms": [], "frames_ms": [], "stats": None} for name in sets}
    try:
        for name, c in sets.items():
            P, A, prop = sipx.setup_constraints([sipx.set_definitions("bounds", "identity", 1600.0, 3900.0, whole), c], g, TF)
            A, AtA, _, _ = sipx.PARSDMM_precompute_distribute(A, prop, g, opt)
            ctx = ctxs[name] = sipx.host.build_context(m, AtA, A, prop, P, g, opt)
            ctx.parsdmm_begin(opt)
            ctx.parsdmm_steps(steps)                      # warm-up
        for _ in range(rounds):
            for name, ctx in ctxs.items():
                ctx.kernel_stats(2)
                ctx.parsdmm_steps(steps)
                st = ctx.kernel_stats_all(0)
                ks = {k["name"]: k for k in st["kernels"]}
                ext = ks.get(ROW)
                if not ext or not ext["launches"]:
                    raise RuntimeError("no projector call was recorded")
                # per launch of the row itself: the feasibility estimate projects outside the "ext_proj" row, so a kernel row has more
                # launches than that row; every kernel named here runs once a projection
                per = lambda rows: sum((ks[r]["total_ms"] / ks[r]["launches"]) for r in rows if r in ks and ks[r]["launches"])
                f = fig[name]
                f["ms"].append(ext["total_ms"] / ext["launches"])
                f["norms_ms"].append(per(NORMS))
                f["apply_ms"].append(per(APPLY))
                f["frames_ms"].append(per(FRAMES))
                f["stats"] = {k: st[k] for k in ("l20", "l21_frames") if k in st}
    finally:
        for ctx in ctxs.values():
            ctx.close()
    return fig


def report(f):
    sel = [a - b - c for a, b, c in zip(f["ms"], f["norms_ms"], f["apply_ms"])]
    return {"ms_per_projection": stat(f["ms"]), "norms_ms": stat(f["norms_ms"]), "apply_ms": stat(f["apply_ms"]), "select_ms": stat(sel),
            "frames_kernel_ms": stat(f["frames_ms"]), "stats": f["stats"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="tv2d", choices=sorted(CASES))
    ap.add_argument("--size", default="")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from __graft_entry__ import load_package
    sipx = load_package()
    TF = np.float32
    n, op, form = CASES[a.case]
    if a.size:
        n = tuple(int(v) for v in a.size.split(","))
    whole = ("matrix", "") if len(n) == 2 else ("tensor", "")
    mode = ("slice", "z") if form == "frames" else whole
    g, m = sipx.compgrid((25.0,) * len(n), n), model(n, TF)
    ng = int(np.prod(n)) if form == "whole" else int(n[0]) * int(n[1])
    k = max(1, ng // 10)
    if form == "joint":
        radius = 0.5 * float(sipx.l21_joint_norm(m, g))
    elif form == "frames":
        radius = (0.5 * np.asarray(sipx.l21_norm(m, g, "TV_xy", mode), np.float64)).astype(TF)
    else:
        radius = 0.5 * float(sipx.l21_norm(m, g, op))
    l20, l21 = ("l20_joint", "l21_joint") if form == "joint" else ("l20", "l21")
    sets = {"l20": sipx.set_definitions(l20, op, 0, k, mode), "l21": sipx.set_definitions(l21, op, 0.0, radius, mode)}
    fig = measure(sipx, g, m, TF, sets, a.steps, a.rounds, whole)
    res = {"dtype": "float32", "steps_per_window": a.steps, "windows": a.rounds, "case": a.case, "n": list(n), "op": op, "form": form,
           "groups": ng, "k": k, "l20": report(fig["l20"]), "l21": report(fig["l21"])}
    res["l20_over_l21"] = round(float(np.median(fig["l20"]["ms"])) / float(np.median(fig["l21"]["ms"])), 3)
    res["apply_not_slower_beyond_the_spread"] = bool(res["l20"]["apply_ms"]["min"] <= res["l21"]["apply_ms"]["max"])
    if form == "frames":
        res["frames_kernel_share_of_l20"] = round(res["l20"]["frames_kernel_ms"]["median"] / res["l20"]["ms_per_projection"]["median"], 3)
    txt = json.dumps(res)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
