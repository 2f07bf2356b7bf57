"""Time of one projection onto the simplex of every fiber z (csrc/seg_simplex.h, csrc/ext_segments.hip: SimplexSegProj) next to the l1
ball of every fiber z (csrc/seg_norm.h, the tile mapping), same build, same run.

    python tools/simplex_bench.py [--size 512,512,8] [--steps 10] [--rounds 3] [--out FILE]

Float32.  Two contexts, {bounds, the set} on the identity with mode ("fiber", "z"): the simplex with min / max = 0.5 / 0.8 times the
median fiber sum of the model, and the ("l1", identity, ("fiber", "z")) set of setup_constraints(..., segment_norms=True) with 0.8 times
the median fiber l1 norm as its radius -- it moves the same bytes through the tile mapping, eight lanes a fiber.  Each runs inside a
PARSDMM solve so that the projector sees the vectors a user's solve hands it.  After a warm-up window the contexts are measured in
alternating windows of `steps` iterations with the engine's device events around every launch (sipx_kernel_stats mode 2); per figure
the median over the windows with the spread.  Figures per set:
    ms_per_projection   the row "ext_proj (library-backed)" per launch: the one kernel of the projector
    bytes               one read and one write of the array, 2 * 4 N: what a projection that moves every segment has to move (the engine
                        books no bytes for this row inside a solve)
    GBps, of_peak       bytes / ms_per_projection, and that against the 8 TB/s of the MI355X's HBM
    ms_per_iteration    wall clock of the window per solve step
and for the simplex the route its projector took (kernel_stats: simplex).  A fiber longer than SIMPLEX_REG_MAX = 32 goes through the
tile route: --size 256,256,40 measures that.
Needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROW = "ext_proj (library-backed)"
PEAK_GBPS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="512,512,8")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from __graft_entry__ import load_package
    sipx = load_package()
    TF = np.float32
    n = tuple(int(v) for v in a.size.split(","))
    if len(n) != 3:
        raise SystemExit("simplex_bench: --size needs three extents")
    mode, whole = ("fiber", "z"), ("tensor", "")
    rng = np.random.default_rng(0)
    z = np.linspace(0, 1, n[-1]).reshape((1, 1, -1))
    m = (1500 + 2500 * z + 150 * rng.standard_normal(n)).astype(TF).reshape(-1, order="F")
    g = sipx.compgrid((25.0,) * 3, n)
    med = float(np.median(sipx.segment_sums(m, g, "identity", mode)))
    med1 = float(np.median(sipx.segment_norms(m, g, "identity", mode, "l1")))
    opt = sipx.PARSDMM_options(FL=TF, maxit=a.steps * (a.rounds + 1), evol_rel_tol=0.0, feas_tol=0.0, obj_tol=0.0)
    sets = {"simplex": sipx.set_definitions("simplex", "identity", 0.5 * med, 0.8 * med, mode),
            "l1": sipx.set_definitions("l1", "identity", 0.0, 0.8 * med1, mode)}
    ctxs, fig = {}, {name: {"ms": [], "iter_ms": [], "bytes": []} for name in sets}
    route = {}
    try:
        for name, c in sets.items():
            P, A, prop = sipx.setup_constraints([sipx.set_definitions("bounds", "identity", 1600.0, 3900.0, whole), c], g, TF, segment_norms=True)
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
                ext = {k["name"]: k for k in st["kernels"]}.get(ROW)
                if not ext or not ext["launches"]:
                    raise RuntimeError("no projector call was recorded")
                fig[name]["iter_ms"].append(1e3 * wall / a.steps)      # (mode 2 times one kernel at a time: comparable between the sets only)
                fig[name]["ms"].append(ext["total_ms"] / ext["launches"])
                fig[name]["bytes"].append(2.0 * m.size * m.itemsize)
                if name == "simplex":
                    route = st["simplex"]
    finally:
        for ctx in ctxs.values():
            ctx.close()

    def stat(v, nd=4):
        return {"median": round(float(np.median(v)), nd), "min": round(float(min(v)), nd), "max": round(float(max(v)), nd)}
    res = {"n": list(n), "dtype": "float32", "steps_per_window": a.steps, "windows": a.rounds, "sets": {}}
    for name, f in fig.items():
        r = {"ms_per_projection": stat(f["ms"]), "ms_per_iteration": stat(f["iter_ms"]), "bytes": int(np.median(f["bytes"]))}
        r["GBps"] = round(r["bytes"] / (r["ms_per_projection"]["median"] * 1e-3) / 1e9, 1)
        r["of_peak"] = round(r["GBps"] / PEAK_GBPS, 3)
        res["sets"][name] = r
    res["sets"]["simplex"]["route"] = "lane" if route.get("lane") else "tile"
    txt = json.dumps(res)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
