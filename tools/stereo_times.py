#!/usr/bin/env python3
"""Stereo bundle adjustment timings: per-kernel-class device time and ms per LM step on synth.ba_stereo, with the
fused assembly (assembly.hip) and with the generic slot path (G2OHIP_ASM_FUSED=0).

    python tools/stereo_times.py [--cameras 1000] [--points 100000] [--steps 20] [--warmup 5] [--out FILE.json]

The LM steps are timed without event records on the stream (wall clock over --steps iterations, device idle at both
ends); the kernel classes come from two further iterations with the per-class HIP-event timer on, as bench.py does.
Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CLASSES = ["linearize", "vreduce", "schur_dinv", "schur_diag", "schur_rows", "chol_factor", "chol_solve", "backsub"]


def run(prob, fused, steps, warmup):
    import g2o_amd
    os.environ["G2OHIP_ASM_FUSED"] = "1" if fused else "0"  # read when the edges are set up
    opt = g2o_amd.SparseOptimizer(0).add_problem(prob)
    opt.set_algorithm("lm_hip_fix6_3")
    opt.set_stats_level(0)
    it = 0
    chi0 = opt.chi2()
    for _ in range(warmup):
        opt.optimize_step(it)
        it += 1
    t0 = time.perf_counter()
    trials = 0
    for _ in range(steps):
        trials += opt.optimize_step(it)[1].levenbergIterations
        it += 1
    dt = time.perf_counter() - t0  # optimize_step returns after the trial's scalar readback: device idle
    opt.enable_kernel_timing(True)
    for _ in range(2):
        opt.optimize_step(it)
        it += 1
    kt = {k: {"avg_ms": opt.kernel_ms(k), "count": opt.kernel_count(k)} for k in CLASSES}
    out = {"fused": bool(fused), "ms_per_lm_step": 1e3 * dt / steps, "lm_it_per_s": steps / dt, "steps": steps,
           "trials": trials, "chi2_initial": chi0, "chi2_final": opt.chi2(), "kernel_ms": kt,
           "linearize_bytes": opt.kernel_bytes("linearize"), "schur_rows_bytes": opt.kernel_bytes("schur_rows")}
    opt.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cameras", type=int, default=1000)
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from g2o_amd import synth
    prob = synth.ba_stereo(args.cameras, args.points)
    res = {"problem": prob.name, "cameras": args.cameras, "points": args.points, "edges": prob.num_edges,
           "runs": [run(prob, fused, args.steps, args.warmup) for fused in (True, False)]}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
