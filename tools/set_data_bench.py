"""What a context per image costs the data-fit loop of the reference's application examples (examples/data_fit_loop.py: learned
list + a data-fit box that changes with every image), measured three ways in one process on one GPU with one build:
  (a) host.PARSDMM with a new Projector for the box -- a list with bound vectors is never cached: a new context per image;
  (b) Solver with numpy arrays: set_data (upload + one launch), sipx_reset, solve, download;
  (c) Solver on torch tensors that already live on the GPU: set_data_dev, sipx_reset_dev, solve, sipx_download_dev.
Per image: the wall time of everything the image needs, split into context (build or set_data + reset: up to the start of
the solve), solve (the solve's own timing sections) and the rest (download, Python).  Median, minimum and maximum over
`images` images after `warmup` images; same images, same starts and -- the three ways give the same bits -- same iterations.
usage: python tools/set_data_bench.py [n=256] [images=12] [warmup=2] [maxit=60] [out=profiles/set_data_256.json]"""
import gc
import json
import os
import sys
import time

import numpy as np
import torch                            # before libsipx: one HIP runtime in the process (host._check_one_hip_runtime)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402
from examples.data_fit_loop import build_problem, observe, synthetic_images  # noqa: E402


def stats(v):
    v = np.asarray(v, np.float64) * 1e3
    return {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max())}


def run(sipx, way, problem, i_data, obs, warmup):
    AtA, A, prop, P, g, opt = problem
    TF = np.dtype(opt.FL).type
    dev = torch.device("cuda", 0)
    on_dev = way == "c"
    y = [a @ obs[0][3] for a in A]
    if on_dev:
        y = [torch.from_numpy(v).to(dev) for v in y]
        obs = [tuple(torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in o) for o in obs]
        torch.cuda.synchronize()
    S = sipx.Solver(AtA, A, prop, P, g, opt, TF) if way != "a" else None
    rows, sums, its = [], [], []
    gc.collect()
    gc.disable()
    try:
        for k, (data, lbd, ubd, x_ini) in enumerate(obs):
            m, x0 = (x_ini.clone(), x_ini.clone()) if on_dev else (x_ini.copy(), x_ini.copy())
            t0 = time.perf_counter()
            if way == "a":
                c = sipx.set_definitions("bounds", "identity", lbd, ubd, ("matrix", ""))
                Pk = list(P)
                Pk[i_data] = sipx.Projector(c, g, TF)
                t_set = time.perf_counter() - t0
                x, log, _, y = sipx.PARSDMM(m, AtA, A, prop, Pk, g, opt, x0, None, y)
                assert not log.context_reused
            else:
                S.set_data(i_data, lbd, ubd)
                t_set = time.perf_counter() - t0
                x, log, _, y = S(m, x0, None, y)
                if on_dev:
                    torch.cuda.synchronize()
                assert log.context_reused == (k > 0)
            t_all = time.perf_counter() - t0
            solve = float(sum(v for kk, v in log.timing.items() if kk != "initialization"))
            ctx = t_set + float(log.timing["initialization"])
            if k >= warmup:
                rows.append((t_all, ctx, solve, t_all - ctx - solve))
                its.append(int(len(log.obj)))
                sums.append(float((x.double().sum().item() if on_dev else x.astype(np.float64).sum())))
    finally:
        gc.enable()
        if S is not None:
            S.close()
    r = np.asarray(rows)
    return {"per_image": stats(r[:, 0]), "context_or_reset": stats(r[:, 1]), "solve": stats(r[:, 2]), "download_and_rest": stats(r[:, 3]),
            "iterations": its, "x_sums": sums}


def main():
    kv = dict(a.split("=", 1) for a in sys.argv[1:])
    n, images, warmup, maxit = int(kv.get("n", 256)), int(kv.get("images", 12)), int(kv.get("warmup", 2)), int(kv.get("maxit", 60))
    sipx = load_package()
    TF = np.float32
    problem, i_data = build_problem(sipx, (n, n), TF, maxit=maxit)
    truth = synthetic_images(images + warmup, (n, n), TF, seed=1)
    obs = [observe(t, TF)[:4] for t in truth]
    sipx.clear_context_cache()
    res = {"what": "per-image wall time of the data-fit loop (examples/data_fit_loop.py), three ways, one process",
           "grid": [n, n], "dtype": "float32", "sets": len(problem[3]), "data_set": i_data, "maxit": maxit,
           "images": images, "warmup_images": warmup, "device": torch.cuda.get_device_name(0)}
    for way, name in (("a", "a_parsdmm_new_context_per_image"), ("b", "b_solver_host_arrays"), ("c", "c_solver_tensors")):
        res[name] = run(sipx, way, problem, i_data, obs, warmup)
    a, b, c = (res[k]["x_sums"] for k in ("a_parsdmm_new_context_per_image", "b_solver_host_arrays", "c_solver_tensors"))
    res["same_results"] = bool(a == b == c)
    med = lambda k: res[k]["per_image"]["median_ms"]
    res["a_over_b"] = med("a_parsdmm_new_context_per_image") / med("b_solver_host_arrays")
    res["a_over_c"] = med("a_parsdmm_new_context_per_image") / med("c_solver_tensors")
    txt = json.dumps(res, indent=1)
    print(txt)
    if kv.get("out"):
        os.makedirs(os.path.dirname(os.path.abspath(kv["out"])) or ".", exist_ok=True)
        with open(kv["out"], "w") as f:
            f.write(txt + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
