"""Time of the structure-only kernel (g2ohip_structure_only_calc, calc(points, 10)) on the full-size BA graphs, next to
one k_linearize pass of an lm_hip_* iteration on the same graph in the same run (the structure-only section).
Both times are HIP-event times from the library's kernel timer. The points are moved by `--sigma` first, so that the
pre-pass has work to do (the generators start 0.05 from the truth).
    python tools/structure_only_times.py --configs C4,C5 --out profiles/structure_only_times.json
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

import g2o_amd  # noqa: E402
from g2o_amd import synth  # noqa: E402


def run(prob, iterations, sigma, repeats):
    pts = next(v for v in prob.vertices if np.any(v.marginalized))
    start = pts.est + np.random.default_rng(11).standard_normal(pts.est.shape) * sigma
    opt = g2o_amd.SparseOptimizer(0).add_problem(prob)
    opt.set_algorithm("lm_hip_fix6_3")
    rows = []
    for k in range(repeats + 1):  # the first call also builds the edge lists and loads the code object: not reported
        opt.set_estimates(pts.vtype, start)
        chi0 = opt.chi2()
        opt.enable_kernel_timing(True, only="structure_only")
        counts = opt.structure_only(iterations=iterations)
        ms = opt.kernel_ms("structure_only")
        opt.enable_kernel_timing(False)
        if k:
            rows.append({"ms": ms, "counts": counts, "chi2_before": chi0, "chi2_after": opt.chi2()})
    out = {"calc_iterations": iterations, "sigma": sigma, "edges": prob.num_edges, "points": int(len(pts.ids)),
           "structure_only_ms": [r["ms"] for r in rows], "counts": rows[-1]["counts"],
           "chi2_before": rows[-1]["chi2_before"], "chi2_after": rows[-1]["chi2_after"],
           "model_bytes_per_pass": opt.kernel_bytes("structure_only")}
    out["model_bytes_per_edge_per_pass"] = out["model_bytes_per_pass"] / prob.num_edges
    # one linearize pass of the LM iteration, for scale
    opt.set_estimates(pts.vtype, start)
    for i in range(6):  # two iterations warm (iteration 0 also builds the structure), four timed
        if i == 2:
            opt.enable_kernel_timing(True, only="linearize")
        opt.optimize_step(i, stats=False)
    out["linearize_ms_per_launch"] = opt.kernel_ms("linearize")
    out["linearize_launches"] = opt.kernel_count("linearize")
    out["linearize_model_bytes"] = opt.kernel_bytes("linearize")
    opt.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C4,C5")
    ap.add_argument("--scale", default="full")
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--sigma", type=float, default=0.2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"version": g2o_amd.lib().g2ohip_version().decode(), "scale": a.scale, "configs": {}}
    for cfg in a.configs.split(","):
        r = run(synth.by_name(cfg, a.scale), a.iterations, a.sigma, a.repeats)
        res["configs"][cfg] = r
        print(f"{cfg}: structure_only calc(points, {a.iterations}) {r['structure_only_ms']} ms, counts {r['counts']}, "
              f"chi2 {r['chi2_before']:.6g} -> {r['chi2_after']:.6g}; linearize {r['linearize_ms_per_launch']:.4f} ms "
              f"per launch ({r['linearize_launches']} launches); model {r['model_bytes_per_edge_per_pass']:.1f} B/edge/pass",
              flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
