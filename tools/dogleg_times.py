"""ms per iteration of dl_hip_* next to gn_hip_* and lm_hip_* on the same graph and build (the dogleg
section). Per configuration and algorithm: a fresh optimizer, `--warmup` iterations, then `--steps` timed ones.
Iteration time is host wall time around g2ohip_optimize_step without statistics (every iteration ends on a stream
synchronisation: the trial's readback). A second run per dl_* graph takes the HIP-event time of the "dogleg" kernel
class alone (its launches per iteration: alpha pass, post-solve sums, and per trial blend + Hpp product, decision).
    python tools/dogleg_times.py --configs C4,C3 --steps 8 --warmup 2 --out profiles/dogleg_times.json
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

import g2o_amd  # noqa: E402
from g2o_amd import synth  # noqa: E402

SUFFIX = {"C1": "fix6_6", "C3": "fix6_6", "C2": "fix3_3", "C4": "fix6_3", "C5": "fix6_3", "S2": "fix3_2"}


def run(prob, algo, warmup, steps, delta=None, timing=False):
    opt = g2o_amd.SparseOptimizer(0).add_problem(prob)
    opt.set_algorithm(algo)
    if delta:
        opt.set_dogleg_params(initial_delta=delta)
    if timing:
        opt.enable_kernel_timing(True, only="dogleg")
    ms, tries, chi = [], [], []
    for i in range(warmup + steps):
        if timing and i == warmup:
            opt.enable_kernel_timing(True, only="dogleg")  # resets the totals
        t0 = time.perf_counter()
        r, _ = opt.optimize_step(i, stats=False)
        dt = time.perf_counter() - t0
        if i >= warmup:
            ms.append(1e3 * dt)
            tries.append(opt.dogleg_state()["tries"] if algo.startswith("dl_") else 1)
        chi.append(opt.chi2())
        if r != 0:
            break
    out = {"algorithm": algo, "iterations": len(ms), "ms_per_iteration_median": sorted(ms)[len(ms) // 2] if ms else None,
           "ms_per_iteration": ms, "trials": tries, "chi2": chi}
    if timing:
        n = opt.kernel_count("dogleg")
        out["dogleg_class_records"] = n
        out["dogleg_class_ms_per_iteration"] = opt.kernel_ms("dogleg") * n / max(len(ms), 1)
        out["dogleg_class_model_bytes"] = opt.kernel_bytes("dogleg")
        out["dogleg_class_model_flops"] = opt.kernel_flops("dogleg")
    opt.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C4,C3")
    ap.add_argument("--scale", default="full")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--delta", type=float, default=0.0, help="initialDelta of the dl_* runs (0: the default 1e4)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"version": g2o_amd.lib().g2ohip_version().decode(), "scale": a.scale, "steps": a.steps, "warmup": a.warmup,
           "initial_delta": a.delta or 1e4, "configs": {}}
    for cfg in a.configs.split(","):
        prob = synth.by_name(cfg, a.scale)
        rows = []
        for m in ("lm", "gn", "dl"):
            rows.append(run(prob, f"{m}_hip_{SUFFIX[cfg]}", a.warmup, a.steps, a.delta if m == "dl" else None))
        rows.append(run(prob, f"dl_hip_{SUFFIX[cfg]}", a.warmup, a.steps, a.delta, timing=True))
        rows[-1]["kernel_timing"] = "dogleg"
        res["configs"][cfg] = rows
        for r in rows:
            print(f"{cfg} {r['algorithm']:14s} {'(dogleg class timed)' if r.get('kernel_timing') else '':22s}"
                  f"{r['ms_per_iteration_median']:9.3f} ms/iteration (median of {r['iterations']}), trials {r['trials']}"
                  + (f", dogleg class {r['dogleg_class_ms_per_iteration']:.3f} ms/iteration in "
                     f"{r['dogleg_class_records']} records" if r.get("kernel_timing") else ""), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
