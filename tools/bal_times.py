"""Device time per launch of the kernels a BAL problem runs (EdgeObservationBAL, 9 x 9 camera blocks, the 9/3 Schur
complement) and LM iterations per second, on synth.bal(): 49 cameras, 7776 points, 31843 observations, the shape of
Ladybug's problem-49-7776-pre.txt. Two LM iterations of warm-up, then one measured run of six; g2ohip_kernel_ms averages
over the run's launches. The figures of DESIGN section 11 "BAL problems" (profiles/bal_kernel_ms.json) come from this script.

  python tools/bal_times.py [out.json]
"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import g2o_amd
from g2o_amd import synth

prob = synth.bal()
opt = g2o_amd.SparseOptimizer(0).add_problem(prob)
opt.set_algorithm("lm_hip_fix9_3")
chi0 = opt.chi2()
opt.optimize(2)
# LM iterations per second without the timing events, then the kernels' times with them
g2o_amd.lib().g2ohip_device_synchronize(0)
t0 = time.time()
nit, st = opt.optimize(6)
g2o_amd.lib().g2ohip_device_synchronize(0)
wall = time.time() - t0
opt.enable_kernel_timing(True)
nit2, st2 = opt.optimize(6)
classes = ("linearize", "vreduce", "schur_dinv", "schur_diag", "schur_rows", "chol_factor", "chol_solve", "backsub", "error", "oplus")
res = {k: {"avg_ms": opt.kernel_ms(k), "count": opt.kernel_count(k)} for k in classes}
res.update(problem=prob.name, cameras=49, points=7776, observations=int(prob.num_edges), block_dims=opt.block_dims(),
           iterations=nit, trials=[s.levenbergIterations for s in st], lm_it_per_s=nit / wall, wall_s=wall,
           chi2_start=chi0, chi2=[s.chi2 for s in st + st2])
print(json.dumps(res))
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
