"""Device time of the assembly launches on a registration graph (Edge_V_V_GICP), per build of the system:
linearize + pair reduce + vertex reduce on the pair-major path, linearize + vertex reduce on the forced slot path and
for the graph's host-Jacobian twin (the only way a tree without the type runs it; the host callback is not counted,
nor is k_offblock_reduce, which runs untimed between the two classes on the slot path and for the twin).
g2ohip_kernel_ms averages over six LM iterations after two of warm-up; one process per run.

  python tools/gicp_times.py pair|slot|twin [out.json] [num_scans neighbours points_per_pair]
"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import g2o_amd
from g2o_amd import synth

mode = sys.argv[1]
shape = [int(x) for x in sys.argv[3:6]] if len(sys.argv) > 5 else [16, 2, 32768]
prob = synth.gicp_scans(*shape)
opt = g2o_amd.SparseOptimizer(0)
if mode == "twin":
    import icp_ref
    g = icp_ref.Graph(prob)
    opt.add_problem(synth.icp_twin(prob))
    opt.set_host_edge_callback(lambda etype, with_jac: g.payload({synth.V_SE3_QUAT: opt.estimates(synth.V_SE3_QUAT)}))
else:
    opt.add_problem(prob)
    opt.set_pair_major(mode == "pair")
opt.set_algorithm("lm_hip_var")
t0 = time.time()
opt.optimize(2)
opt.enable_kernel_timing(True)
n, st = opt.optimize(6)
classes = ("linearize", "pair_reduce", "vreduce", "error")
res = {k: {"avg_ms": opt.kernel_ms(k), "count": opt.kernel_count(k)} for k in classes}
res["assembly_ms_per_build"] = sum(res[k]["avg_ms"] for k in ("linearize", "pair_reduce", "vreduce") if res[k]["count"])
res.update(mode=mode, shape=shape, edges=int(prob.num_edges), final_chi2=st[-1].chi2, wall_s=time.time() - t0,
           pair_major=opt.pair_major_info() if mode != "twin" else None)
print(json.dumps(res))
if len(sys.argv) > 2 and sys.argv[2] != "-":
    json.dump(res, open(sys.argv[2], "w"), indent=1)
