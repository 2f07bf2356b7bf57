"""Timing of the db4 wavelet transform (kernels_dwt.hip) and of the l1 ball behind it.

    python tools/dwt_bench.py [--sizes 256,256,256 512,512,512 2048,2048] [--reps 10] [--out FILE]
    python tools/dwt_bench.py --summarize <rocprofv3 results .db of a run of this tool> [--out FILE]

Per grid (Float32): sipx_dwt forward and inverse, a whole sipx_project call of the l1 ball behind the wavelet and, as context,
of the l1 ball behind the DCT.  Each entry is the median wall time of `reps` calls after one warm-up; the calls include the
host <-> device copies of the C entry points (4 N bytes each way per vector) and their allocations, so kernel times come from a
run of this tool under `rocprofv3 --kernel-trace --stats` (k_dwt_pass / k_dwt_small rows).  Also printed: the algorithmic bytes
of one axis pass of the first level, 2 N w, and what 8 TB/s would take for them.  --summarize maps every k_dwt_pass dispatch of such
a trace to its grid, level, axis and direction (by its work-item count) and reports the median duration and the fraction of 8 TB/s
on 2 box w algorithmic bytes per pass, and the one-workgroup k_dwt_small launch per transform."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def lib_sha16():
    import hashlib
    path = os.environ.get("SIPX_LIBRARY") or os.path.join(ROOT, "setintersectionprojection.jl_amd", "libsipx.so")
    return hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]


def pass_table(sizes):
    """(R, work-item count) -> [(grid, level, axis, box entries)] for the axis passes of kernels_dwt.hip (RC = 2, RS = 8,
    boxes above 4096 entries)."""
    t = {}
    for n in sizes:
        nd = len(n)
        b = list(n) + [1] * (3 - nd)
        L, m = 0, min(n)
        while m % 2 == 0:
            m //= 2
            L += 1
        for lev in range(1, L + 1):
            box = b[0] * b[1] * b[2]
            if box <= 4096:
                break
            for ax in range(nd):
                R = 2 if ax == 0 else 8
                items = -(-(b[ax] // 2) // R) * (box // b[ax])
                t.setdefault((R, -(-items // 256) * 256), []).append((tuple(n), lev, ax, box))
            b = [v // 2 for v in b[:nd]] + [1] * (3 - nd)
    return t


def summarize(db_path, sizes):
    """Dispatches in trace order: the grids follow each other as the tool ran them; inside a level the two strided passes of a
    3-D grid have the same work-item count and are told apart by their order (forward: axis 1 then 2, inverse: 2 then 1)."""
    import re
    import sqlite3
    db = sqlite3.connect(db_path)
    rows = db.execute("select name, grid_x, duration from kernels where name like '%k_dwt%' order by start").fetchall()
    tables = [pass_table([n]) for n in sizes]
    acc, small = {}, {}
    gi, prev = 0, None
    for name, gx, dur in rows:
        mp = re.search(r"k_dwt_pass<(float|double), (true|false), (\d+)>", name)
        ms = re.search(r"k_dwt_small<(float|double), (true|false)>", name)
        if ms:
            small.setdefault((ms.group(2) == "true", ms.group(1)), []).append(dur)
            prev = None
            continue
        if not mp:
            continue
        dt, inv, key = mp.group(1), mp.group(2) == "true", (int(mp.group(3)), gx)
        while gi < len(tables) and key not in tables[gi]:
            gi += 1
        if gi == len(tables):
            break
        cands = tables[gi][key]
        if len(cands) > 1:      # two strided axes of one level: the second launch of the pair takes the other one
            second = prev == (key, inv, dt)
            cands = sorted(cands, key=lambda c: c[2], reverse=inv)
            c = cands[1 if second else 0]
            prev = None if second else (key, inv, dt)
        else:
            c = cands[0]
            prev = None
        n, lev, ax, box = c
        acc.setdefault((n, lev, ax, inv, dt, box), []).append(dur)
    out = {"libsipx_sha16": lib_sha16(), "peak_TBps": 8.0, "passes": [], "small_box_kernel": []}
    for (n, lev, ax, inv, dt, box), d in sorted(acc.items()):
        w = 8 if dt == "double" else 4
        med = float(np.median(d)) * 1e-9
        out["passes"].append({"grid": list(n), "level": lev, "axis": ax, "inverse": inv, "dtype": dt, "launches": len(d),
                              "median_us": round(med * 1e6, 2), "bytes": 2 * box * w,
                              "frac_of_8TBps": round(2 * box * w / med / 8e12, 3)})
    for (inv, dt), d in sorted(small.items()):
        out["small_box_kernel"].append({"inverse": inv, "dtype": dt, "launches": len(d), "median_us": round(float(np.median(d)) * 1e-3, 2)})
    out["per_transform_us"] = {}
    for p in out["passes"]:
        k = "x".join(map(str, p["grid"])) + (" inverse" if p["inverse"] else " forward")
        out["per_transform_us"][k] = round(out["per_transform_us"].get(k, 0.0) + p["median_us"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--summarize", default="")
    ap.add_argument("--sizes", nargs="+", default=["256,256,256", "512,512,512", "2048,2048"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.summarize:
        res = summarize(a.summarize, [tuple(int(v) for v in s.split(",")) for s in a.sizes])
        txt = json.dumps(res, indent=1)
        print(txt)
        if a.out:
            with open(a.out, "w") as f:
                f.write(txt + "\n")
        return
    from __graft_entry__ import load_package
    sipx = load_package()
    TF = np.float32
    res = []
    for s in a.sizes:
        n = tuple(int(v) for v in s.split(","))
        N = int(np.prod(n))
        rng = np.random.default_rng(0)
        x = rng.standard_normal(N).astype(TF)
        g = sipx.compgrid((1.0,) * len(n), n)
        c = sipx.dwt(x, n)
        r = float(0.3 * np.abs(c).sum())

        def timed(f):
            f()
            t = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                f()
                t.append(time.perf_counter() - t0)
            return 1e3 * float(np.median(t))
        Pw = sipx.host.Projector(sipx.set_definitions("l1", "wavelet", 0.0, r, ("matrix", "")), g, TF)
        Pd = sipx.host.Projector(sipx.set_definitions("l1", "DCT", 0.0, r, ("matrix", "")), g, TF)
        e = {"n": list(n), "dtype": "float32", "libsipx_sha16": lib_sha16(), "levels": sipx.host._dwt_check_grid(n),
             "forward_call_ms": timed(lambda: sipx.dwt(x, n)),
             "inverse_call_ms": timed(lambda: sipx.dwt(c, n, inverse=True)),
             "project_l1_wavelet_call_ms": timed(lambda: Pw(x.copy())),
             "project_l1_dct_call_ms": timed(lambda: Pd(x.copy())),
             "first_level_axis_pass_bytes": 2 * N * 4,
             "first_level_axis_pass_ms_at_8TBps": 2 * N * 4 / 8e12 * 1e3}
        print(json.dumps(e), flush=True)
        res.append(e)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
