"""linearize / camera pass / error kernel times of the CameraParameters edge types beside their twins, fused and
generic path (g2ohip_kernel_ms averages over ten LM iterations after three of warm-up).

  python tools/camparams_times.py [out.json]
"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import g2o_amd
from g2o_amd import synth

out = {}
for stereo in (False, True):
    prob = synth.ba_camparams(40, 1500, 8, 24, stereo=stereo)
    for name, p in (("camparams", prob), ("twin", synth.camparams_twin(prob))):
        for fused in ("1", "0"):
            os.environ["G2OHIP_ASM_FUSED"] = fused
            opt = g2o_amd.SparseOptimizer(0).add_problem(p)
            opt.set_algorithm("lm_hip_fix6_3")
            opt.optimize(3)
            opt.enable_kernel_timing(True)
            opt.optimize(10)
            out[f"{'stereo' if stereo else 'mono'}/{name}/fused={fused}"] = {
                k: {"avg_ms": opt.kernel_ms(k), "count": opt.kernel_count(k)} for k in ("linearize", "vreduce", "error")}
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
for k, v in out.items():
    print(k, {a: round(b["avg_ms"], 5) for a, b in v.items()})
