"""Timing of constraint learning (sipx.constraint_learning_by_obseration, csrc/learn.hip) at user sizes.

    python tools/learn_bench.py [--reps 3] [--out FILE]
    python tools/learn_bench.py --summarize <rocprofv3 results .db of a run of this tool> [--out FILE]

Cases: 512 images of 256^2 and 64 images of 1024^2 in Float32, 64 images of 256^2 in Float64, every key.  Each case is called
once to warm up (code objects, library plans), then `reps` times; reported is the median wall time per call and per image,
host <-> device copies and allocations included.  As context only, the numpy restatement (tests/learn_ref.py) is timed in the
same run on a few of the images and scaled per image.

--summarize reads a trace of this tool under `rocprofv3 --kernel-trace --stats` and reports the kernel time per phase (diff,
FFT, DWT, sort, histogram fold, cardinality scan, DCT, SVD, other) and the achieved bytes/s of k_learn_diff, from the bytes it
must move computed here from the shapes (read the image, write the TV rows, |TV| and the float64 D_x / D_z matrices when every
key is wanted), against the 6.29 TB/s measured float4 copy rate of the MI355X."""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(512, (256, 256), "float32"), (64, (1024, 1024), "float32"), (64, (256, 256), "float64")]
COPY_TBPS = 6.29
TILE = 4096          # elements per k_learn_diff workgroup (learn.hip)


def diff_bytes(n, w):
    """Bytes one image costs k_learn_diff with every key wanted: read N w, write TV and |TV| (2 M w) and D_x, D_z in float64."""
    n1, n2 = n
    N, Mx, Mz = n1 * n2, (n1 - 1) * n2, n1 * (n2 - 1)
    return N * w + 2 * (Mx + Mz) * w + 8 * (Mx + Mz)


PHASES = [("diff", r"k_learn_diff"), ("repack", r"k_learn_repack"), ("fft", r"k_learn_to_complex|k_learn_dft_abs|fft|FFT"),
          ("dwt", r"k_dwt|k_learn_l1"), ("sort", r"radix|sort|Sort"), ("hist_fold", r"k_learn_fold"), ("card_scan", r"k_learn_card"),
          ("dct", r"k_learn_dct|gemm|Cijk"), ("svd", r"k_learn_sv|k_learn_to_f64|rocsolver|syevd|gesvdj|stedc|sytrd|sterf|lasr|jacobi|"
                                                   r"Jacobi|latrd|larf|steqr")]


def summarize(db_path):
    import sqlite3
    db = sqlite3.connect(db_path)
    cols = [r[1] for r in db.execute("pragma table_info(kernels)")]
    gy = "grid_y" if "grid_y" in cols else ("grid_size_y" if "grid_size_y" in cols else None)
    gx = "grid_x" if "grid_x" in cols else "grid_size_x"
    rows = db.execute(f"select name, {gx}, {gy or 1}, duration from kernels order by start").fetchall()
    phase_ns = {p: 0 for p, _ in PHASES}
    phase_ns["other"] = 0
    diff = {}
    for name, x, y, dur in rows:
        for p, rx in PHASES:
            if re.search(rx, name):
                phase_ns[p] += dur
                break
        else:
            phase_ns["other"] += dur
        if "k_learn_diff" in name:
            w = 8 if "k_learn_diff<double>" in name or "k_learn_diffIdE" in name else 4
            tiles = x // 256
            for nt, n, dt in CASES:
                if -(-n[0] * n[1] // TILE) == tiles and (w == 8) == (dt == "float64"):
                    d = diff.setdefault("x".join(map(str, n)) + " " + dt, {"bytes": 0, "ns": 0, "launches": 0})
                    d["bytes"] += diff_bytes(n, w) * y
                    d["ns"] += dur
                    d["launches"] += 1
    total = sum(phase_ns.values())
    out = {"kernel_ms_per_phase": {p: round(v * 1e-6, 3) for p, v in phase_ns.items()},
           "share_per_phase": {p: round(v / total, 3) for p, v in phase_ns.items()} if total else {},
           "k_learn_diff": {k: {"launches": v["launches"], "ms": round(v["ns"] * 1e-6, 3), "GB": round(v["bytes"] * 1e-9, 3),
                                "TBps": round(v["bytes"] / v["ns"] * 1e-3, 3),
                                "frac_of_copy_rate": round(v["bytes"] / v["ns"] * 1e-3 / COPY_TBPS, 3)} for k, v in diff.items()},
           "copy_rate_TBps": COPY_TBPS}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--summarize", default="")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ref-images", type=int, default=4)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.summarize:
        res = summarize(a.summarize)
    else:
        from __graft_entry__ import load_package
        from tests import learn_ref as R
        sipx = load_package()
        res = []
        H = (25.0, 6.0)
        for nt, n, dt in CASES:
            TF = np.dtype(dt).type
            rng = np.random.default_rng(nt + n[0])
            m = (1500 + 150 * rng.standard_normal((nt,) + n)).astype(TF)
            g = sipx.compgrid(H, n)
            sipx.constraint_learning_by_obseration(g, m)
            t = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                sipx.constraint_learning_by_obseration(g, m)
                t.append(time.perf_counter() - t0)
            k = min(a.ref_images, nt)
            t0 = time.perf_counter()
            R.learn(m[:k], H)
            t_ref = (time.perf_counter() - t0) / k
            med = float(np.median(t))
            e = {"n_train": nt, "n": list(n), "dtype": dt, "reps": a.reps, "call_s": round(med, 4),
                 "ms_per_image": round(1e3 * med / nt, 4), "numpy_restatement_ms_per_image": round(1e3 * t_ref, 2),
                 "k_learn_diff_bytes_per_image": diff_bytes(n, np.dtype(dt).itemsize)}
            print(json.dumps(e), flush=True)
            res.append(e)
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
