"""Time of one projection onto a group-cardinality set (csrc/card_groups.h, csrc/ext_group.hip: CardGroupsProj), in two modes.

    python tools/card_groups_bench.py --size 256,256,64 --mode fiber [--steps 10] [--rounds 3] [--out FILE]
    python tools/card_groups_bench.py --routes [--steps 10] [--rounds 3] [--out FILE]

Float32, inside a PARSDMM solve of {bounds, the set} so that the projector sees the vectors a user's solve hands it, the engine's device
events around every launch (sipx_kernel_stats mode 2), a warm-up window, then `rounds` alternating windows of `steps` iterations; every
figure is the median over the windows with its spread [min, max].

--size / --mode: ("card_groups", D_z, (mode, z)) with k = a quarter of the segments against ("l21_groups", D_z, same mode) at half the
    group norm of A m, same arrays, same run.  The norms launch of the two is the same code.  Figures per set:
    ms_per_projection   the row "ext_proj (library-backed)" per launch: norms, selection (or Michelot passes with the reads of their
                        flag), apply
    norms_ms, apply_ms  the rows k_l21g_norms (+ k_l21g_finish for slices), and k_cardg_zero or k_l21g_scale, per projection
    select_ms           ms_per_projection - norms_ms - apply_ms: the selection with the gaps between its launches
--routes: the small route (k_cardg_rank, one launch) against the engine's search on the same g, nseg in {8, 64, 1024, 4096}: two
    contexts that differ in the forced route alone (sipx_card_groups_route).  CARDG_SMALL_MAX follows from these numbers: the small
    route stays where it beats the search by more than the spread between the windows.  Above the cap as built only the search is
    measured (profiles/card_groups_routes_cap4096_f32.json holds the run of the first form of the kernel, four segments a thread at 4096,
    which lowered the cap).
Needs a GPU."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROW, NORMS, FINISH, ZERO, SCALE, RANK = ("ext_proj (library-backed)", "k_l21g_norms", "k_l21g_finish", "k_cardg_zero", "k_l21g_scale",
                                         "k_cardg_rank")
ROUTE_GEOMETRIES = [((256, 256, 8), ("slice", "z")), ((256, 256, 64), ("slice", "z")), ((32, 32, 64), ("fiber", "z")),
                    ((64, 64, 64), ("fiber", "z"))]      # nseg = 8, 64, 1024, 4096 on the identity
SMALL_MAX = 1024                                         # CARDG_SMALL_MAX of csrc/card_groups.h


def stat(v, nd=4):
    return {"median": round(float(np.median(v)), nd), "min": round(float(min(v)), nd), "max": round(float(max(v)), nd)}


def model(n, TF):
    rng = np.random.default_rng(0)
    z = np.linspace(0, 1, n[-1]).reshape((1, 1, -1))
    return (1500 + 2500 * z + 150 * rng.standard_normal(n)).astype(TF).reshape(-1, order="F")


def measure(sipx, g, m, TF, sets, steps, rounds, routes=None):
    """sets: name -> set_definitions; routes: name -> forced route while that context is built.  Returns name -> lists per window."""
    opt = sipx.PARSDMM_options(FL=TF, maxit=steps * (rounds + 1), evol_rel_tol=0.0, feas_tol=0.0, obj_tol=0.0)
    ctxs, fig = {}, {name: {"ms": [], "norms_ms": [], "apply_ms": [], "rank_ms": [], "stats": None} for name in sets}
    try:
        for name, c in sets.items():
            if sipx.lib().sipx_card_groups_route((routes or {}).get(name, 0)) != 0:
                raise RuntimeError(sipx.lib().sipx_last_error().decode())
            P, A, prop = sipx.setup_constraints([sipx.set_definitions("bounds", "identity", 1600.0, 3900.0, ("tensor", "")), c], g, TF)
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
                per = lambda row: (ks[row]["total_ms"] / ks[row]["launches"]) if row in ks and ks[row]["launches"] else 0.0
                f = fig[name]
                f["ms"].append(ext["total_ms"] / ext["launches"])
                f["norms_ms"].append(per(NORMS) + per(FINISH))
                f["apply_ms"].append(per(ZERO) + per(SCALE))
                f["rank_ms"].append(per(RANK))
                f["stats"] = {k: st[k] for k in ("card_groups", "l21_groups") if k in st}
    finally:
        sipx.lib().sipx_card_groups_route(0)
        for ctx in ctxs.values():
            ctx.close()
    return fig


def report(f):
    sel = [a - b - c for a, b, c in zip(f["ms"], f["norms_ms"], f["apply_ms"])]
    return {"ms_per_projection": stat(f["ms"]), "norms_ms": stat(f["norms_ms"]), "apply_ms": stat(f["apply_ms"]), "select_ms": stat(sel),
            "rank_kernel_ms": stat(f["rank_ms"]), "stats": f["stats"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="256,256,64")
    ap.add_argument("--mode", default="fiber", choices=("fiber", "slice"))
    ap.add_argument("--routes", action="store_true")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from __graft_entry__ import load_package
    sipx = load_package()
    TF = np.float32
    res = {"dtype": "float32", "steps_per_window": a.steps, "windows": a.rounds}
    if a.routes:
        res["cases"] = {}
        for n, mode in ROUTE_GEOMETRIES:
            g, m = sipx.compgrid((25.0,) * 3, n), model(n, TF)
            nseg = len(sipx.group_norms(m, g, "identity", mode))
            k = max(1, nseg // 4)
            c = sipx.set_definitions("card_groups", "identity", 0, k, mode)
            names = ("small", "search") if nseg <= SMALL_MAX else ("search",)      # (above the cap the library refuses the small route)
            fig = measure(sipx, g, m, TF, {q: c for q in names}, a.steps, a.rounds, {"small": 1, "search": 2})
            case = {"n": list(n), "mode": list(mode), "nseg": nseg, "k": k}
            case.update({q: report(fig[q]) for q in names})
            if "small" in case:
                lo, hi = case["small"]["select_ms"], case["search"]["select_ms"]
                case["small_beats_search_beyond_the_spread"] = bool(lo["max"] < hi["min"])
            res["cases"][str(nseg)] = case
    else:
        n = tuple(int(v) for v in a.size.split(","))
        mode = (a.mode, "z")
        g, m = sipx.compgrid((25.0,) * 3, n), model(n, TF)
        nseg = len(sipx.group_norms(m, g, "D_z", mode))
        k = max(1, nseg // 4)
        sets = {"card_groups": sipx.set_definitions("card_groups", "D_z", 0, k, mode),
                "l21_groups": sipx.set_definitions("l21_groups", "D_z", 0.0, 0.5 * float(sipx.l21_groups_norm(m, g, "D_z", mode)), mode)}
        fig = measure(sipx, g, m, TF, sets, a.steps, a.rounds)
        res.update({"n": list(n), "op": "D_z", "mode": list(mode), "nseg": nseg, "k": k, "rows": int(np.prod(n)) - int(n[0] * n[1]),
                    "card_groups": report(fig["card_groups"]), "l21_groups": report(fig["l21_groups"])})
        res["card_groups_over_l21_groups"] = round(float(np.median(fig["card_groups"]["ms"])) / float(np.median(fig["l21_groups"]["ms"])), 3)
    txt = json.dumps(res)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
