"""Time of one projection onto an l1 / l2 ball per fiber or per slice (csrc/seg_norm.h) with a scalar radius and with one radius per
segment, and of the observation kernel behind sipx.segment_norms.

    python tools/seg_radii_bench.py [--size 256,256,256] [--steps 10] [--rounds 3] [--radii scalar|vector|both] [--observe] [--out FILE]

Float32, the three rows of tools/seg_norms_bench.py: l1 per fiber z on D_z, l2 per fiber x on the identity, l1 per slice z on D_x.  One
context per set and form, {bounds, the set}, each inside a PARSDMM solve so that the projector sees the vectors a user's solve hands
it; timed by the engine's device events around every call of the materialised projector (sipx_kernel_stats mode 2, row "ext_proj
(library-backed)": here the one kernel k_seg_norm).  The vector form holds the scalar's value in every entry: the same arithmetic and
the same bits, so the difference is the radius load.  After a warm-up window the contexts are measured in alternating windows of
`steps` iterations; per context the median over the windows with the spread.  --radii scalar runs on a library without vector radii
too (SIPX_LIBRARY names it): the figure of an earlier build, from a process of its own.
--observe: k_seg_observe on the same three A x, timed the same way on a context of its own; M w / t (one read pass).  Needs a GPU."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROW = "ext_proj (library-backed)"
SETS = {"l1_fiber_z_Dz": ("l1", "D_z", ("fiber", "z")), "l2_fiber_x": ("l2", "identity", ("fiber", "x")),
        "l1_slice_z_Dx": ("l1", "D_x", ("slice", "z"))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="256,256,256")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--radii", default="both", choices=("scalar", "vector", "both"))
    ap.add_argument("--observe", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch      # (before the library: one HIP runtime in the process)
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
    bounds = sipx.set_definitions("bounds", "identity", 1600.0, 3900.0, ("tensor", ""))

    def rows_of(opn):
        A, _, _, tdn, _ = sipx.get_TD_operator(g, opn, TF)
        return np.asarray(A @ m, np.float64).reshape(tuple(int(q) for q in tdn), order="F")
    ax = {"x": 0, "y": 1, "z": 2}
    defs, size = {}, {}
    for name, (st, opn, mode) in SETS.items():
        s = rows_of(opn)
        size[name] = s.size
        red = ax[mode[1]] if mode[0] == "fiber" else tuple(q for q in range(3) if q != ax[mode[1]])
        nrm = np.abs(s).sum(axis=red) if st == "l1" else np.sqrt((s ** 2).sum(axis=red))
        r = float(TF(0.5 * nrm.mean()))              # half the mean per-segment norm
        if a.radii in ("scalar", "both"):
            defs[name + "_scalar"] = sipx.set_definitions(st, opn, 0.0, r, mode)
        if a.radii in ("vector", "both"):
            defs[name + "_vector"] = sipx.set_definitions(st, opn, 0.0, np.full(nrm.size, r, TF), mode)
    ctxs, per_call = {}, {k: [] for k in defs}
    res = {"n": list(n), "dtype": "float32", "steps_per_window": a.steps, "windows": a.rounds, "library": os.path.basename(os.path.dirname(sipx.LIB_PATH)) + "/" + os.path.basename(sipx.LIB_PATH)}
    try:
        for name, c in defs.items():
            P, A, prop = sipx.setup_constraints([bounds, c], g, TF, segment_norms=True)
            A, AtA, _, _ = sipx.PARSDMM_precompute_distribute(A, prop, g, opt)
            ctx = ctxs[name] = sipx.host.build_context(m, AtA, A, prop, P, g, opt)
            ctx.parsdmm_begin(opt)
            ctx.parsdmm_steps(a.steps)                      # warm-up
        for _ in range(a.rounds):
            for name, ctx in ctxs.items():
                ctx.kernel_stats(2)
                ctx.parsdmm_steps(a.steps)
                rows = [k for k in ctx.kernel_stats_all(0)["kernels"] if k["name"] == ROW]
                if not rows or not rows[0]["launches"]:
                    raise RuntimeError("no projector call was recorded")
                per_call[name].append(rows[0]["total_ms"] / rows[0]["launches"])
    finally:
        for ctx in ctxs.values():
            ctx.close()
    for name, v in per_call.items():
        med = float(np.median(v))
        res[name + "_ms_per_projection"] = {"median": round(med, 4), "min": round(min(v), 4), "max": round(max(v), 4)}
        res[name + "_TB_per_s_2Mw"] = round(2.0 * size[name.rsplit("_", 1)[0]] * 4 / (med * 1e-3) / 1e12, 3)
    if a.observe:
        # a finalized context of its own (the statistics need one); the calls go straight to the C ABI with tensors that stay put
        P, A, prop = sipx.setup_constraints([bounds], g, TF)
        A, AtA, _, _ = sipx.PARSDMM_precompute_distribute(A, prop, g, opt)
        ctx = sipx.host.build_context(m, AtA, A, prop, P, g, opt)
        try:
            dev = torch.device("cuda", 0)
            x = torch.from_numpy(m).to(dev)
            ctx.set_caller_stream(torch.cuda.current_stream(dev).cuda_stream)
            for name, (st, opn, mode) in SETS.items():
                Pd = sipx.Projector(sipx.set_definitions("l2", opn, 0.0, 1.0, mode), g, TF)
                out = torch.empty(Pd.nseg(sipx.TDOperator(opn, g, TF)), dtype=torch.float32, device=dev)
                cnt = C.c_int64()

                def call():
                    sipx.host._chk(sipx.lib().sipx_segment_norms_dev(ctx.h, sipx.host.OPS[opn], Pd.mode, Pd.dir, 0 if st == "l1" else 1,
                                                                     C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), C.byref(cnt)))
                call()                                      # warm-up
                v = []
                for _ in range(a.rounds):
                    ctx.kernel_stats(2)
                    for _ in range(a.steps):
                        call()
                    rows = [k for k in ctx.kernel_stats_all(0)["kernels"] if k["name"] == ROW]
                    v.append(rows[0]["total_ms"] / rows[0]["launches"])
                med = float(np.median(v))
                res[name + "_observe_ms"] = {"median": round(med, 4), "min": round(min(v), 4), "max": round(max(v), 4)}
                res[name + "_observe_TB_per_s_Mw"] = round(size[name] * 4 / (med * 1e-3) / 1e12, 3)
        finally:
            ctx.close()
    txt = json.dumps(res)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
