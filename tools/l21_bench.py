"""Time of one projection onto the l2,1 ball on the TV operator (isotropic TV, csrc/ext_group.hip) next to the anisotropic l1 ball on
TV, same build.

    python tools/l21_bench.py [--size 256,256,256] [--steps 10] [--rounds 3] [--out FILE]

Float32.  Two contexts, {bounds, l21 on TV} and {bounds, l1 on TV}, each inside a PARSDMM solve so that the projector sees the
vectors a user's solve hands it.  After a warm-up window the contexts are measured in alternating windows of `steps` iterations
with the engine's device events around every launch (sipx_kernel_stats mode 2); per figure the median over the windows with the
spread.

l21: the row "ext_proj (library-backed)" is the whole materialised projector in the y/l update -- k_l21_norms, the threshold search
on the N group norms, k_l21_scale -- and "k_pass<M_STORE>" the pass that materialises v in front of it; their sum is the time per
projection.  The feasibility estimate runs the same projector outside the ext_proj row, but its store pass and its search are in
their rows: the search's rows are divided by the launches of the store pass (one per search), and the bytes the engine booked on
them likewise.  Figures:
    ms_per_projection            ext_proj + store pass
    TB_per_s                     ((2 nblk + 2) N w + search bytes) / ms_per_projection, nblk = the grid's dimension count, w = 4
    kernels_ms, kernels_TB_per_s the two new kernels alone: ext_proj minus the search's rows per search, (2 nblk + 2) N w over that
                                 (the ext_proj row also holds the event records around the search's launches, a few microseconds
                                 each: the kernels' share is overstated by that)
l1 on TV has no such row -- its projection is part of k_yl -- so its figure is the sum of the rows of its threshold search per
iteration, as tools/seg_norms_bench.py reports the whole-array set.  Needs a GPU."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROW, STORE = "ext_proj (library-backed)", "k_pass<M_STORE>"
SEARCH_ROWS = ("k_pass<M_FIRST>", "k_pass<M_LEAN>", "k_pass<M_PROBE>", "k_pass<M_COMPACT>", "k_pass_multi", "k_slot_sums", "k_decide",
               "k_sample", "k_l1_solve")


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
    N, nblk = int(np.prod(n)), len(n)
    mode = ("matrix", "") if nblk == 2 else ("tensor", "")
    rng = np.random.default_rng(0)
    z = np.linspace(0, 1, n[-1]).reshape((1,) * (len(n) - 1) + (-1,))
    m = (1500 + 2500 * z + 150 * rng.standard_normal(n)).astype(TF).reshape(-1, order="F")
    g = sipx.compgrid((25.0,) * len(n), n)
    maxit = a.steps * (a.rounds + 1)
    opt = sipx.PARSDMM_options(FL=TF, maxit=maxit, evol_rel_tol=0.0, feas_tol=0.0, obj_tol=0.0)
    s = np.asarray(sipx.get_TD_operator(g, "TV", TF)[0] @ m, np.float64)
    sets = {        # radii: half the respective norm of TV m
        "l21_TV": sipx.set_definitions("l21", "TV", 0.0, 0.5 * float(sipx.l21_norm(m, g)), mode),
        "l1_TV": sipx.set_definitions("l1", "TV", 0.0, 0.5 * float(np.abs(s).sum()), mode),
    }
    ctxs, fig = {}, {"l21_ms": [], "l21_kernels_ms": [], "l21_search_bytes": [], "l1_search_ms": []}
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
                ks = {k["name"]: k for k in ctx.kernel_stats_all(0)["kernels"]}
                search_ms = sum(k["total_ms"] for nm, k in ks.items() if nm in SEARCH_ROWS)
                if name == "l1_TV":
                    fig["l1_search_ms"].append(search_ms / a.steps)
                    continue
                ext, store = ks.get(ROW), ks.get(STORE)
                if not ext or not ext["launches"] or not store or not store["launches"]:
                    raise RuntimeError("no projector call was recorded")
                searches = store["launches"]                # y update and feasibility estimate: one store pass in front of each
                per_ext = ext["total_ms"] / ext["launches"]
                fig["l21_ms"].append(per_ext + store["total_ms"] / store["launches"])
                fig["l21_kernels_ms"].append(per_ext - search_ms / searches)
                fig["l21_search_bytes"].append(sum(k["bytes_survey"] for nm, k in ks.items() if nm in SEARCH_ROWS) / searches)
    finally:
        for ctx in ctxs.values():
            ctx.close()

    def stat(v, nd=4):
        return {"median": round(float(np.median(v)), nd), "min": round(float(min(v)), nd), "max": round(float(max(v)), nd)}
    own = (2 * nblk + 2) * N * 4
    ms, kms, sb = float(np.median(fig["l21_ms"])), float(np.median(fig["l21_kernels_ms"])), float(np.median(fig["l21_search_bytes"]))
    res = {"n": list(n), "dtype": "float32", "steps_per_window": a.steps, "windows": a.rounds,
           "l21_TV_ms_per_projection": stat(fig["l21_ms"]), "l21_TV_kernel_bytes": own, "l21_TV_search_bytes_per_projection": round(sb),
           "l21_TV_TB_per_s": round((own + sb) / (ms * 1e-3) / 1e12, 3),
           "l21_TV_kernels_ms": stat(fig["l21_kernels_ms"]), "l21_TV_kernels_TB_per_s": round(own / (kms * 1e-3) / 1e12, 3),
           "l1_TV_search_ms_per_iteration": stat(fig["l1_search_ms"])}
    txt = json.dumps(res)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
