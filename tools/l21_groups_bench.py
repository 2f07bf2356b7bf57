"""Time of one projection onto the l2,1 ball over fibers or slices (csrc/l21_groups.h, csrc/ext_group.hip: GroupsProj) next to the
("l2", op, same mode) projector -- one independent l2 ball per segment, one workgroup per slice (csrc/seg_norm.h) -- on the same arrays,
same build, same run, in alternating windows.

    python tools/l21_groups_bench.py [--size 256,256,64] [--steps 5] [--rounds 3] [--out FILE]

Float32.  For op in {D_z, identity} and mode in {("fiber", "z"), ("slice", "z")}: two contexts {bounds, the set}, each inside a PARSDMM
solve so that the projector sees the vectors a user's solve hands it; tau = half the group norm of A m, the l2 radius half the median
segment norm (most segments are read and written).  After a warm-up window the contexts are measured in alternating windows of `steps`
iterations with the engine's device events around every launch (sipx_kernel_stats mode 2); per figure the median over the windows with
the spread.  Figures per set:
    ms_per_projection   the row "ext_proj (library-backed)" per launch: for l21_groups the norms, the passes with the host's reads of the
                        flag between the batches, and the scale; for l2 the one launch of k_seg_norm
    norms_ms, scale_ms  l21_groups: the rows k_l21g_norms (+ k_l21g_finish for slices) and k_l21g_scale per launch
    passes              Michelot passes of the last projection of the window (kernel_stats: l21_groups)
    bytes               (N reads for the norms + passes * 2 nseg for the search + 2 N for the scale) * 4, the count of DESIGN.md
    gbps, share         bytes over ms_per_projection, and its share of the 5.98 TB/s measured copy ceiling quoted in VERDICT.md
Needs a GPU."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROW, NORMS, FINISH, SCALE = "ext_proj (library-backed)", "k_l21g_norms", "k_l21g_finish", "k_l21g_scale"
COPY_CEILING_TBPS = 5.98      # the measured device-to-device copy ceiling


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="256,256,64")
    ap.add_argument("--steps", type=int, default=5)
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
    res = {"n": list(n), "dtype": "float32", "steps_per_window": a.steps, "windows": a.rounds, "copy_ceiling_tbps": COPY_CEILING_TBPS, "cases": {}}
    for op in ("D_z", "identity"):
        for mode in (("fiber", "z"), ("slice", "z")):
            seg = sipx.segment_norms(m, g, op, mode, "l2")
            rows = int(np.prod(n)) - (int(n[0] * n[1]) if op == "D_z" else 0)
            sets = {"l21_groups": sipx.set_definitions("l21_groups", op, 0.0, 0.5 * float(sipx.l21_groups_norm(m, g, op, mode)), mode),
                    "l2": sipx.set_definitions("l2", op, 0.0, 0.5 * float(np.median(seg)), mode)}
            ctxs, fig = {}, {name: {"ms": [], "norms_ms": [], "scale_ms": [], "passes": []} for name in sets}
            try:
                for name, c in sets.items():
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
                        st = ctx.kernel_stats_all(0)
                        ks = {k["name"]: k for k in st["kernels"]}
                        ext = ks.get(ROW)
                        if not ext or not ext["launches"]:
                            raise RuntimeError("no projector call was recorded")
                        f = fig[name]
                        f["ms"].append(ext["total_ms"] / ext["launches"])
                        if name == "l21_groups":
                            per = lambda row: (ks[row]["total_ms"] / ext["launches"]) if row in ks and ks[row]["launches"] else 0.0
                            f["norms_ms"].append(per(NORMS) + per(FINISH))
                            f["scale_ms"].append(per(SCALE))
                            f["passes"].append(st["l21_groups"]["passes"])
            finally:
                for ctx in ctxs.values():
                    ctx.close()

            def stat(v, nd=4):
                return {"median": round(float(np.median(v)), nd), "min": round(float(min(v)), nd), "max": round(float(max(v)), nd)}
            f = fig["l21_groups"]
            passes = float(np.median(f["passes"]))
            nbytes = (3.0 * rows + passes * 2.0 * len(seg)) * 4.0
            ms = float(np.median(f["ms"]))
            case = {"nseg": int(len(seg)), "rows": rows,
                    "l21_groups": {"ms_per_projection": stat(f["ms"]), "norms_ms": stat(f["norms_ms"]), "scale_ms": stat(f["scale_ms"]),
                                   "passes": stat(f["passes"], 0), "bytes": nbytes, "gbps": round(nbytes / ms * 1e-6, 1),
                                   "share_of_copy_ceiling": round(nbytes / ms * 1e-9 / COPY_CEILING_TBPS, 4)},
                    "l2_per_segment": {"ms_per_projection": stat(fig["l2"]["ms"])}}
            case["norms_over_l2_projection"] = round(float(np.median(f["norms_ms"])) / float(np.median(fig["l2"]["ms"])), 3)
            res["cases"][f"{op} {mode[0]} {mode[1]}"] = case
    txt = json.dumps(res)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
