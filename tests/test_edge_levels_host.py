"""Edge levels and classification without a GPU: the interface (header, exports, wrapper) and the helpers of
tests/test_gpu_edge_levels.py against each other."""
import ctypes
import os
import re

import numpy as np

import edge_levels_ref as R
import expmap_ref
from g2o_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "g2o_hip.h")
SYMBOLS = ("g2ohip_set_edge_levels", "g2ohip_get_edge_levels", "g2ohip_initialize_level", "g2ohip_edge_chi2",
           "g2ohip_classify_edges")


def test_header_constants_and_exports(g2o_amd_mod):
    text = open(HEADER).read()
    m = re.search(r"#define G2OHIP_LEVEL_KEEP \((-\d+) - (\d+)\)", text)
    assert m and int(m.group(1)) - int(m.group(2)) == g2o_amd_mod.LEVEL_KEEP == R.LEVEL_KEEP == -2 ** 31
    assert g2o_amd_mod.SparseOptimizer.LEVEL_KEEP == g2o_amd_mod.LEVEL_KEEP
    assert ctypes.c_int(g2o_amd_mod.LEVEL_KEEP).value == g2o_amd_mod.LEVEL_KEEP  # fits the C int it is passed as
    declared = set(re.findall(r"\b(g2ohip_[a-z0-9_]+)\s*\(", text))
    for s in SYMBOLS:
        assert s in declared and s in g2o_amd_mod.EXPORTS, s


def test_symbols_in_the_library(g2o_amd_mod):
    L = ctypes.CDLL(g2o_amd_mod.LIB_PATH)
    assert not [s for s in SYMBOLS if not hasattr(L, s)]
    assert not [s for s in SYMBOLS if not hasattr(g2o_amd_mod.lib(), s)]


def test_wrapper_methods_exist(g2o_amd_mod):
    import inspect
    S = g2o_amd_mod.SparseOptimizer
    for name in ("set_edge_levels", "edge_levels", "edge_chi2", "classify_edges", "initialize_optimization"):
        assert callable(getattr(S, name)), name
    assert inspect.signature(S.initialize_optimization).parameters["level"].default == 0
    p = inspect.signature(S.classify_edges).parameters
    assert (p["check_depth"].default, p["inlier_level"].default, p["outlier_level"].default) == (False, 0, 1)
    assert inspect.signature(S.edge_chi2).parameters["depth"].default is False
    assert inspect.signature(S.set_edge_levels).parameters["idx"].default is None


def test_reference_chi2_adds_up_to_the_graph_chi2():
    """The per-edge restatement and the graph chi2 the other tests pin are the same numbers."""
    prob = synth.with_priors(synth.ba(num_cameras=6, num_points=40, obs_per_point=4), synth.E_XYZ_PRIOR, every=3)
    total = sum(R.edge_chi2(prob, es.etype).sum() for es in prob.edges)
    want = expmap_ref.Graph(prob).chi2()
    assert abs(total - want) <= 1e-13 * want


def test_host_rule_and_threshold():
    chi = np.array([1.0, 5.0, np.nan, 2.0, 9.0, 3.0])
    z = np.array([1.0, 1.0, 1.0, -1.0, 0.0, np.nan])
    lv, c = R.classify(chi, 4.0)
    assert lv.tolist() == [0, 1, 0, 0, 1, 0] and c == dict(over_chi2=2, depth_failed=0, bad=2)  # NaN is not "bad"
    lv, c = R.classify(chi, 4.0, z)
    assert lv.tolist() == [0, 1, 0, 1, 1, 1] and c == dict(over_chi2=2, depth_failed=3, bad=4)  # !(z > 0): 0 and NaN
    lv, _ = R.classify(chi, 4.0, None, [1, 0, 1, 0, 0, 2], R.LEVEL_KEEP, 1)
    assert lv.tolist() == [1, 1, 1, 0, 1, 2]
    thr, gap = R.gap_threshold(np.arange(1.0, 101.0))
    assert 70 < thr < 90 and abs(thr - round(thr)) == 0.5 and gap > 0.01
    assert R.gap_threshold(np.array([3.0]))[0] == 1.5


def test_subproblem_and_levels():
    prob = synth.ba(num_cameras=6, num_points=40, obs_per_point=4)
    lv, gone, single = R.ba_levels(prob, 11)
    es = prob.edges[0]
    l0 = lv[es.etype]
    assert np.all(l0[es.v0 == gone] == 1) and int((l0[es.v0 == single] == 0).sum()) == 1
    assert abs(int(l0.sum()) - len(l0) // 3) <= 8
    sub = R.subproblem(prob, {es.etype: l0 == 0})
    assert sub.num_edges == int((l0 == 0).sum()) and sub.num_vertices == prob.num_vertices
    assert gone not in sub.edges[0].v0
    assert R.subproblem(prob, {es.etype: np.zeros(len(l0), bool)}).edges == []


def test_behind_camera_moves_the_chosen_points():
    for stereo in (False, True):
        etype = R.E_STEREO if stereo else R.E_MONO
        prob = synth.pose_only(num_cameras=2, points_per_camera=10, stereo=stereo)
        rows = [0, 7, 13]
        z = R.depth_z(R.behind_camera(prob, etype, rows), etype)
        assert np.allclose(z[rows], -0.5, atol=1e-12) and np.all(np.delete(z, rows) > 0.1)
        assert np.all(R.depth_z(prob, etype) > 0.1)
