"""Time of one projection onto an l1 / l2 ball per fiber or per slice (csrc/seg_norm.h) next to the whole-array l1 ball, same build.

    python tools/seg_norms_bench.py [--size 256,256,256] [--steps 10] [--rounds 3] [--out FILE]

Float32.  One context per set, {bounds, the set}, each inside a PARSDMM solve so that the projector sees the vectors a user's solve
hands it.  The per-segment sets are timed by the engine's device events around every call of the materialised projector
(sipx_kernel_stats mode 2, row "ext_proj (library-backed)": here the one kernel k_seg_norm).  The whole-array l1 set on the same
operator has no such row -- its projection is part of k_yl -- so its figure is the sum of the rows of its threshold search
(first / probe / compaction passes, sums, decision, solve) per iteration: what the set costs on top of the y/l update.  After a
warm-up window the contexts are measured in alternating windows of `steps` iterations; per context the median
over the windows is reported with the spread, and 2 M w / t (read once, write once) for the per-segment sets.  Needs a GPU."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROW = "ext_proj (library-backed)"
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
    rng = np.random.default_rng(0)
    z = np.linspace(0, 1, n[-1]).reshape((1,) * (len(n) - 1) + (-1,))
    m = (1500 + 2500 * z + 150 * rng.standard_normal(n)).astype(TF).reshape(-1, order="F")
    g = sipx.compgrid((25.0,) * len(n), n)
    maxit = a.steps * (a.rounds + 1)
    opt = sipx.PARSDMM_options(FL=TF, maxit=maxit, evol_rel_tol=0.0, feas_tol=0.0, obj_tol=0.0)

    def rows_of(opn):
        A, _, _, tdn, _ = sipx.get_TD_operator(g, opn, TF)
        return np.asarray(A @ m, np.float64).reshape(tuple(int(q) for q in tdn), order="F")
    sz, sx, si = rows_of("D_z"), rows_of("D_x"), rows_of("identity")
    sets = {        # radii: half the mean per-segment norm
        "l1_fiber_z_Dz": (sipx.set_definitions("l1", "D_z", 0.0, float(0.5 * np.abs(sz).sum(axis=2).mean()), ("fiber", "z")), sz.size),
        "l1_slice_z_Dx": (sipx.set_definitions("l1", "D_x", 0.0, float(0.5 * np.abs(sx).sum(axis=(0, 1)).mean()), ("slice", "z")), sx.size),
        "l2_fiber_x": (sipx.set_definitions("l2", "identity", 0.0, float(0.5 * np.sqrt((si ** 2).sum(axis=0)).mean()), ("fiber", "x")), si.size),
        "l1_whole_Dz": (sipx.set_definitions("l1", "D_z", 0.0, float(0.5 * np.abs(sz).sum()), ("tensor", "")), sz.size),
    }
    ctxs, per_call = {}, {k: [] for k in sets}
    try:
        for name, (c, _) in sets.items():
            P, A, prop = sipx.setup_constraints([sipx.set_definitions("bounds", "identity", 1600.0, 3900.0, ("tensor", "")), c], g, TF,
                                                segment_norms=True)
            A, AtA, _, _ = sipx.PARSDMM_precompute_distribute(A, prop, g, opt)
            ctx = ctxs[name] = sipx.host.build_context(m, AtA, A, prop, P, g, opt)
            ctx.parsdmm_begin(opt)
            ctx.parsdmm_steps(a.steps)                      # warm-up
        for _ in range(a.rounds):
            for name, ctx in ctxs.items():
                ctx.kernel_stats(2)
                ctx.parsdmm_steps(a.steps)
                ks = ctx.kernel_stats_all(0)["kernels"]
                if name == "l1_whole_Dz":                   # the rows of its threshold search, per iteration (the projection itself is part of k_yl)
                    per_call[name].append(sum(k["total_ms"] for k in ks if k["name"] in SEARCH_ROWS) / a.steps)
                    continue
                rows = [k for k in ks if k["name"] == ROW]
                if not rows or not rows[0]["launches"]:
                    raise RuntimeError("no projector call was recorded")
                per_call[name].append(rows[0]["total_ms"] / rows[0]["launches"])
    finally:
        for ctx in ctxs.values():
            ctx.close()
    res = {"n": list(n), "dtype": "float32", "steps_per_window": a.steps, "windows": a.rounds}
    for name, v in per_call.items():
        med = float(np.median(v))
        key = name + ("_search_ms_per_iteration" if name == "l1_whole_Dz" else "_ms_per_projection")
        res[key] = {"median": round(med, 4), "min": round(min(v), 4), "max": round(max(v), 4)}
        if name != "l1_whole_Dz":
            res[name + "_TB_per_s_2Mw"] = round(2.0 * sets[name][1] * 4 / (med * 1e-3) / 1e12, 3)
    txt = json.dumps(res)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
