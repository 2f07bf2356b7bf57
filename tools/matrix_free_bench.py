"""Timing of the matrix-free term of Q (csrc/kernels_sparse.hip): sparse operators whose A'A is not kept as CDS bands.

    python tools/matrix_free_bench.py [--steps 30] [--warmup 5] [--out FILE] [--parent-lib libsipx.so of the parent commit]

Cases, each in a child process of its own under `timeout`; the tool stops at the first one that fails:
  blur    the deblurring example's mask * kron(I, Bx), motion blur of 25 taps, on 2048 x 1536, Float32 (51 diagonals in A'A)
  psf9    a 9 x 9 box point-spread function (81 taps, 289 diagonals) on 2048 x 1536, Float32
  dxz     D_z D_x on 2048 x 2048, Float32 (nine diagonals): the matrix-free route against the CDS route.  With --parent-lib the
          CDS route runs on the parent commit's library: the one comparison that has a baseline.
Per case: iterations per second of the native loop (tolerances zero, so every step runs), and from a second window with
per-kernel statistics (HIP events around every launch) the launches and time of k_mf_fwd / k_mf_adj, and their achieved
bytes per second on nnz (w + 4) + row pointers + vector bytes, beside the 5.98 TB/s copy ceiling."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_CEILING_TBPS = 5.98


def operators(case, TF):
    import scipy.sparse as sp
    if case == "blur":
        n, bkl = (2048, 1536), 25
        n1, n2 = n
        Bx = sp.identity(n1, format="csc") / bkl
        for i in range(2, bkl + 1):
            Bx = Bx + sp.diags([np.ones(n1 - i)], [i], shape=(n1, n1)) / bkl
        Bx = Bx.tocsr()[:n1 - bkl, :]
        mask = np.ones((n1 - bkl) * n2)
        mask[::5] = 0.0
        A = (sp.diags(mask) @ sp.kron(sp.identity(n2), Bx)).tocsc()
        A.eliminate_zeros()
    elif case == "psf9":
        n, k = (2048, 1536), 9

        def box(m):
            return sp.diags([np.ones(m - k + 1)] * k, list(range(k)), shape=(m - k + 1, m)) / k
        A = sp.kron(box(n[1]), box(n[0])).tocsc()
    else:
        n = (2048, 2048)

        def diff(m):
            return sp.diags([-np.ones(m - 1), np.ones(m - 1)], [0, 1], shape=(m - 1, m))
        A = sp.kron(diff(n[1]), diff(n[0])).tocsc()
    A = sp.csc_matrix(A, dtype=TF)
    A.sort_indices()
    return n, A


def child(case, route, steps, warmup):
    from __graft_entry__ import load_package
    sipx = load_package()
    TF = np.float32
    n, A = operators(case, TF)
    N = int(np.prod(n))
    rng = np.random.default_rng(0)
    z = np.linspace(0, 1, n[1]).reshape(1, -1)
    m = (1500 + 2500 * z + 150 * rng.standard_normal(n)).astype(TF).reshape(-1, order="F")
    s = A @ m
    g = sipx.compgrid((1.0, 1.0), n)
    c = [sipx.set_definitions("bounds", "identity", 1600.0, 3900.0, ("matrix", "")),
         sipx.set_definitions("bounds", "identity", float(0.3 * s.min()), float(0.3 * s.max()), ("matrix", ""))]
    c[1].custom_TD_OP = (A, False)
    opt = sipx.PARSDMM_options(FL=TF, maxit=warmup + 2 * steps + 2, evol_rel_tol=0.0, feas_tol=0.0, obj_tol=0.0)
    P, ops, prop = sipx.setup_constraints(c, g, TF)
    if route == "free":
        prop.banded[1] = False
    t0 = time.perf_counter()
    ops, AtA, _, _ = sipx.PARSDMM_precompute_distribute(ops, prop, g, opt)
    t_pre = time.perf_counter() - t0
    ctx = sipx.host.build_context(m, AtA, ops, prop, P, g, opt)
    res = {"case": case, "route": route, "grid": list(n), "dtype": "float32", "rows": int(A.shape[0]), "nnz": int(A.nnz),
           "precompute_s": round(t_pre, 3), "AtA_bands": None if AtA[1] is None else int(AtA[1].shape[1]),
           "library": os.environ.get("SIPX_LIBRARY") or "this tree"}
    if hasattr(sipx.host.lib(), "sipx_q_terms"):
        res["q_terms"] = list(ctx.q_terms())
    ctx.parsdmm_begin(opt)
    ctx.parsdmm_steps(warmup)
    t0 = time.perf_counter()
    ctx.parsdmm_steps(steps)
    dt = time.perf_counter() - t0
    res["iterations_per_s"] = round(steps / dt, 2)
    res["ms_per_iteration"] = round(1e3 * dt / steps, 4)
    ctx.kernel_stats_all(2)                      # a window of its own: two event records around every launch
    ctx.parsdmm_steps(steps)
    st = ctx.kernel_stats_all(0)
    log = ctx.parsdmm_log()
    res["cg_iterations_per_step"] = round(float(np.mean(log.cg_it[warmup:warmup + steps])), 2)
    kern = {k["name"]: k for k in st.get("kernels", [])}
    res["kernels"] = {}
    for name in ("k_mf_fwd", "k_mf_adj", "k_cds<MODE=1>", "k_cds_fused", "k_csr_spmv"):
        if name in kern:
            k = kern[name]
            e = {f: k[f] for f in k if f != "name"}
            res["kernels"][name] = e
    w = 4
    if "k_mf_fwd" in kern:                       # bytes per launch as the launchers book them (kernels_sparse.hip, mf_bytes)
        for name, rows, vec in (("k_mf_fwd", A.shape[0], 2 * A.shape[0]), ("k_mf_adj", N, 3 * N)):
            k = kern[name]
            ms = k.get("total_ms", k.get("ms", 0.0)) / max(1, k.get("launches", 1))
            b = A.nnz * (w + 4) + 4 * (rows + 1) + vec * w
            res["kernels"][name]["bytes_per_launch_min"] = int(b)
            res["kernels"][name]["achieved_TBps"] = round(b / (ms * 1e-3) / 1e12, 3) if ms > 0 else None
            res["kernels"][name]["copy_ceiling_TBps"] = COPY_CEILING_TBPS
    ctx.close()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--cases", nargs="+", default=["blur", "psf9", "dxz"])
    ap.add_argument("--limit", type=int, default=240, help="seconds a case may take")
    ap.add_argument("--child", nargs=2, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child[0], a.child[1], a.steps, a.warmup)
        return
    runs = []
    for case in a.cases:
        runs.append((case, "free", ""))
        if case == "dxz":
            runs.append((case, "cds", ""))
            if a.parent_lib:
                runs.append((case, "cds", os.path.abspath(a.parent_lib)))
    out = []
    for case, route, libpath in runs:
        env = dict(os.environ)
        if libpath:
            env["SIPX_LIBRARY"] = libpath
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--steps", str(a.steps), "--warmup", str(a.warmup),
               "--child", case, route]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
            print(f"case {case} / {route} failed with exit status {r.returncode}: stopping", file=sys.stderr)
            if a.out:
                with open(a.out, "w") as f:
                    json.dump(out, f, indent=1)
            sys.exit(r.returncode or 1)
        e = json.loads(line[0][7:])
        print(json.dumps(e), flush=True)
        out.append(e)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
