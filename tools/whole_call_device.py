"""The `whole_call` measurement of bench.py for both forms of the boundary, in one process: PARSDMM on numpy arrays (m in, x / l / y
out over PCIe) and PARSDMM_device on torch tensors that live on the GPU.  Same problem (bench config c3, default options, the
stop rules decide), same models, same sequence of calls per form: a first call (context built), two calls on the reused context
with everything returned (the faster one is the "second call"), a last one that asks for x alone into the caller's own buffer.
The solve alone is the sum of the solve's own timing sections of that call.  A device-form call is timed until the caller's
stream has the results (torch.cuda.synchronize after the call); what the call itself takes on the host is listed beside it.
usage: python tools/whole_call_device.py [n=256] [dtype=f32] [out=profiles/whole_call_device_256.json]
Prints the JSON and, with out=, writes it."""
import gc
import json
import os
import sys
import time

import numpy as np
import torch                            # before libsipx: one HIP runtime in the process (host._check_one_hip_runtime)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench                            # noqa: E402
from __graft_entry__ import load_package  # noqa: E402


def measure(sipx, form, problem, ms, calls=4):
    AtA, A, prop, P, g, opt = problem
    sipx.clear_context_cache()
    rows = []
    dev = form == "device"
    if dev:
        md = [torch.from_numpy(m).cuda() for m in ms]
        dt = md[0].dtype
        xbuf = torch.zeros_like(md[0])
        out_all = (torch.empty_like(md[0]), [torch.empty(a.shape[0], dtype=dt, device="cuda") for a in A],
                   [torch.empty(a.shape[0], dtype=dt, device="cuda") for a in A])
        torch.cuda.synchronize()
    else:
        xbuf = np.zeros_like(ms[0])
    gc.collect()
    gc_on = gc.isenabled()
    gc.disable()
    for k in range(calls):
        last = k == calls - 1
        t0 = time.perf_counter()
        if dev:
            kw = dict(outputs="x", out=(xbuf, None, None)) if last else dict(out=out_all)
            x, log, l, y = sipx.PARSDMM_device(md[k], AtA, A, prop, P, g, opt, **kw)
            t_ret = time.perf_counter() - t0
            torch.cuda.synchronize()
        else:
            kw = dict(x=xbuf, outputs="x") if last else {}
            x, log, l, y = sipx.PARSDMM(ms[k], AtA, A, prop, P, g, opt, **kw)
            t_ret = time.perf_counter() - t0
        t_all = time.perf_counter() - t0
        solve = float(sum(v for kk, v in log.timing.items() if kk != "initialization"))
        xs = x.cpu().numpy() if dev else x
        rows.append({"call": k + 1, "whole_call_s": t_all, "returned_after_s": t_ret, "initialization_s": float(log.timing["initialization"]),
                     "solve_s": solve, "download_and_rest_s": t_all - solve - float(log.timing["initialization"]),
                     "iterations": int(len(log.obj)), "context_reused": bool(log.context_reused), "outputs": "x" if last else "x, l, y",
                     "finite": bool(np.isfinite(xs).all()), "x_sum": float(xs.astype(np.float64).sum())})
        del x, l, y, xs
    if gc_on:
        gc.enable()
    sipx.clear_context_cache()
    again = min(rows[1:calls - 1], key=lambda r: r["whole_call_s"])
    last = rows[-1]
    return {"calls": rows, "first_call_s": rows[0]["whole_call_s"], "second_call_s": again["whole_call_s"],
            "second_call_runs_s": [r["whole_call_s"] for r in rows[1:calls - 1]], "second_call_solve_s": again["solve_s"],
            "second_call_overhead": (again["whole_call_s"] - again["solve_s"]) / again["solve_s"],
            "x_only_call_s": last["whole_call_s"], "x_only_solve_s": last["solve_s"],
            "x_only_call_overhead": (last["whole_call_s"] - last["solve_s"]) / last["solve_s"]}


def main():
    kw = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
    n1 = int(kw.get("n", 256))
    TF = {"f32": np.float32, "f64": np.float64}[kw.get("dtype", "f32")]
    sipx = load_package()
    _, h, kinds = bench.CONFIGS["c3"]
    n = (n1, n1, n1)
    gs = sipx.compgrid(h, n)
    calls = 4
    ms = [bench.synthetic_model(n, TF, 20240601 + 3 + k) for k in range(calls)]

    def radius_of(opname):
        s = sipx.get_TD_operator(gs, opname, TF)[0] @ ms[0]
        return float(0.5 * np.abs(s.astype(np.float64)).sum())
    g, c = bench.build_problem(sipx, n, h, kinds, ms[0], TF, radius_of)
    P, A, prop = sipx.setup_constraints(c, g, TF)
    opt = sipx.PARSDMM_options(FL=TF)
    A, AtA, _, _ = sipx.PARSDMM_precompute_distribute(A, prop, g, opt)
    problem = (AtA, A, prop, P, g, opt)
    res = {"workload": f"c3 {n1}^3 {np.dtype(TF).name}: whole calls of PARSDMM(...) and PARSDMM_device(...), default options (stop rules active)",
           "device": torch.cuda.get_device_name(0), "hip_runtime": torch.version.hip}
    # host form first, then the device form, then the host form again: drift of the machine between the two shows up
    res["host"] = measure(sipx, "host", problem, ms, calls)
    res["device"] = measure(sipx, "device", problem, ms, calls)
    res["host_again"] = measure(sipx, "host", problem, ms, calls)
    same = all(a["x_sum"] == b["x_sum"] and a["iterations"] == b["iterations"] for a, b in zip(res["host"]["calls"], res["device"]["calls"]))
    res["same_results"] = bool(same)
    res["device_second_call_below_host_x_only"] = bool(res["device"]["second_call_s"] < min(res["host"]["x_only_call_s"], res["host_again"]["x_only_call_s"]))
    for form in ("host", "device", "host_again"):
        r = res[form]
        print(f"{form:>10}: first {r['first_call_s'] * 1e3:8.1f} ms   second {r['second_call_s'] * 1e3:7.1f} ms (solve {r['second_call_solve_s'] * 1e3:.1f}, "
              f"+{100 * r['second_call_overhead']:.0f} %)   x only {r['x_only_call_s'] * 1e3:7.1f} ms (solve {r['x_only_solve_s'] * 1e3:.1f}, "
              f"+{100 * r['x_only_call_overhead']:.0f} %)", file=sys.stderr)
    txt = json.dumps(res, indent=1)
    print(txt)
    if "out" in kw:
        os.makedirs(os.path.dirname(os.path.abspath(kw["out"])), exist_ok=True)
        with open(kw["out"], "w") as f:
            f.write(txt + "\n")
    return 0 if same else 3


if __name__ == "__main__":
    sys.exit(main())
