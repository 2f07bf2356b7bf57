"""Time of one projection onto "at most k Fourier atoms" (SIPX_PROJ_CARD_DFT) next to the l1 ball behind the DFT, same build.

    python tools/card_dft_bench.py [--size 256,256,256] [--steps 10] [--rounds 3] [--out FILE]

Float32.  Two contexts, {bounds, cardinality behind the DFT at k = N/10} and {bounds, l1 behind the DFT at a quarter of
||F m||_1}, each inside a PARSDMM solve so that the projector sees the vectors a user's solve hands it (warm search state,
both of its per-iteration calls).  The figure is the engine's own: device events around every call of the materialised
projector (sipx_kernel_stats mode 2, row "ext_proj (library-backed)": transforms, magnitude pass, threshold search, weights,
unpack), total milliseconds over calls.  After a warm-up window the two contexts are measured in alternating windows of
`steps` iterations; per context the median over the windows is reported, and the spread.  Needs a GPU."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROW = "ext_proj (library-backed)"


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
    N = int(np.prod(n))
    rng = np.random.default_rng(0)
    z = np.linspace(0, 1, n[-1]).reshape((1,) * (len(n) - 1) + (-1,))
    m = (1500 + 2500 * z + 150 * rng.standard_normal(n)).astype(TF).reshape(-1, order="F")
    l1 = float(0.25 * np.abs(np.fft.fftn(m.reshape(n, order="F").astype(np.float64), norm="ortho")).sum())
    g = sipx.compgrid((25.0,) * len(n), n)
    maxit = a.steps * (a.rounds + 1)
    opt = sipx.PARSDMM_options(FL=TF, maxit=maxit, evol_rel_tol=0.0, feas_tol=0.0, obj_tol=0.0)
    sets = {"cardinality_dft": sipx.set_definitions("cardinality", "DFT", 0, N // 10, ("matrix", "")),
            "l1_dft": sipx.set_definitions("l1", "DFT", 0.0, l1, ("matrix", ""))}
    ctxs, per_call = {}, {k: [] for k in sets}
    try:
        for name, c in sets.items():
            P, A, prop = sipx.setup_constraints([sipx.set_definitions("bounds", "identity", 1600.0, 3900.0, ("matrix", "")), c], g, TF)
            A, AtA, _, _ = sipx.PARSDMM_precompute_distribute(A, prop, g, opt)
            ctx = ctxs[name] = sipx.host.build_context(m, AtA, A, prop, P, g, opt)
            ctx.parsdmm_begin(opt)
            ctx.parsdmm_steps(a.steps)                      # warm-up: first launches, plans, the searches' warm starts
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
    res = {"n": list(n), "dtype": "float32", "k": N // 10, "steps_per_window": a.steps, "windows": a.rounds}
    for name, v in per_call.items():
        res[name + "_ms_per_projection"] = {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    txt = json.dumps(res)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
