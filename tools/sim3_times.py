"""Device time per launch of `linearize` (k_linearize_sim3 against k_linearize<FamilySE3>), `vreduce` and `error` on two
pose graphs of one topology: synth.sphere(100, 100, extra_lap2=True) (10 000 poses, 49 399 EDGE_SE3:QUAT edges) as it is,
and the same vertices and vertex pairs as a Sim3 graph (VERTEX_SIM3:EXPMAP keyframes at the sphere's poses with scales
near 1, EDGE_SIM3:EXPMAP measurements C = N Sj Si^-1 with a small random similarity N, random SPD 7 x 7 information).
g2ohip_kernel_ms averages over six LM iterations after two of warm-up; one process per run. The figures of DESIGN §11
"Sim3 pose graphs" (profiles/sim3_kernel_ms.json) come from this script.

  python tools/sim3_times.py se3|sim3|sim3_shared [out.json]      (sim3_shared: one information record for all edges)
"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import g2o_amd
from g2o_amd import synth

mode = sys.argv[1]
base = synth.sphere(100, 100, extra_lap2=True)
if mode == "se3":
    prob = base
else:
    vs, es = base.vertices[0], base.edges[0]
    n, m = len(vs.ids), len(es.v0)
    rng = synth._rng(synth.SEED, 81)
    R = synth.quat_to_rot(vs.est[:, 3:7])
    truth = (R, vs.est[:, :3].copy(), np.exp(0.05 * rng.standard_normal(n)))
    ia, ib = np.searchsorted(vs.ids, es.v0), np.searchsorted(vs.ids, es.v1)
    sel = lambda S, k: (S[0][k], S[1][k], S[2][k])  # noqa: E731
    noise = (synth._small_rot(rng, m, 0.01), 0.02 * rng.standard_normal((m, 3)), np.exp(0.01 * rng.standard_normal(m)))
    meas = synth._sim3_vec(synth._sim3_mul(noise, synth._sim3_mul(sel(truth, ib), synth._sim3_inv(sel(truth, ia)))))
    info = synth._spd_info(rng, 1 if mode == "sim3_shared" else m, np.array([0.01] * 3 + [0.02] * 3 + [0.01]))
    info = np.broadcast_to(info, (m, 7, 7)).copy() if mode == "sim3_shared" else info
    verts = synth.VertexSet(synth.V_SIM3, vs.ids, synth._sim3_vec(truth), vs.fixed, vs.marginalized)
    prob = synth.Problem("sphere_as_sim3", [verts], [synth.EdgeSet(synth.E_SIM3, es.v0, es.v1, meas, info)], 7, 0)
opt = g2o_amd.SparseOptimizer(0).add_problem(prob)
opt.set_algorithm("lm_hip_var")
t0 = time.time()
opt.optimize(2)
opt.enable_kernel_timing(True)
nit, st = opt.optimize(6)
classes = ("linearize", "vreduce", "error", "oplus", "chol_factor")
res = {k: {"avg_ms": opt.kernel_ms(k), "count": opt.kernel_count(k)} for k in classes}
res.update(mode=mode, vertices=int(prob.num_vertices), edges=int(prob.num_edges), iterations=nit,
           final_chi2=st[-1].chi2, wall_s=time.time() - t0)
print(json.dumps(res))
if len(sys.argv) > 2 and sys.argv[2] != "-":
    json.dump(res, open(sys.argv[2], "w"), indent=1)
