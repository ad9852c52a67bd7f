"""CPU checks behind tests/test_gpu_camparams.py: the numpy restatement of EdgeProjectXYZ2UV / EdgeProjectXYZ2UVU
(tests/camparams_ref.py) against g2o's numeric Jacobian, the visibility of the all-double baseline in the single-edge
case, the generators and their twins, the reference-format file writer and reader, and the Python constants against the
header. (A graph handle needs a device, so the library's own loader and writer are checked in test_gpu_camparams.py,
against the files written here.)"""
import os
import re

import numpy as np
import pytest

import camparams_ref as R
import stereo_ref
from camparams_ref import KINDS, UV, UVU
from g2o_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the measured worst relative difference (below), and the project's margin of four (test_expmap_host.test_band_tolerance)
NUMERIC_GAP = 2.72e-7


@pytest.mark.parametrize("etype", KINDS)
def test_analytic_jacobians_vs_g2o_numeric(etype):
    """The analytic Jacobians of both types against central differences with g2o's own step, delta = 1e-9
    (base_binary_edge.hpp), through the vertices' oplus, on ba_camparams(12, 150, 5, 8). For XYZ2UVU this is the
    comparison with what the reference itself computes (it has no linearizeOplus). Per edge and block,
    max|J - N| / max|J|; measured worst over the 750 edges: 2.72e-7 on the point block and 1.00e-7 on the camera
    block, for both types (the rounding estimate eps * |projection| / delta with projections up to 550 px gives
    about 1e-7 absolute on entries of order 1e2..1e3). Asserted at four times the measured value."""
    prob = synth.ba_camparams(12, 150, 5, 8, stereo=etype == UVU)
    g = R.Graph(prob)
    s = g.set_of(etype)
    cam, pt = g._est(s, None, None)
    Ji, Jj = R.edge_jacobians(etype, cam, pt, s.e.params)
    Ni, Nj = R.numeric_jacobians(etype, cam, pt, s.e.meas, s.e.params)
    worst = 0.0
    for name, A, N in (("point", Ji, Ni), ("camera", Jj, Nj)):
        rel = float(np.max(np.max(np.abs(A - N), axis=(1, 2)) / np.max(np.abs(A), axis=(1, 2))))
        print(f"type {etype} {name} block: worst relative difference {rel:.3e}")
        worst = max(worst, rel)
    assert worst <= 4 * NUMERIC_GAP, worst


def test_uvu_row2_is_the_stereo_row_with_bf():
    """Rows 0-1 of XYZ2UVU are XYZ2UV's; all three rows equal EdgeStereoSE3ProjectXYZ's forms with fx = fy = f and
    bf = f * b to rounding (the expression forms differ)."""
    prob = synth.ba_camparams(12, 150, 5, 8, stereo=True, focal=512.0, baseline=0.125)
    g = R.Graph(prob)
    s = g.sets[0]
    cam, pt = g._est(s, None, None)
    K = s.e.params
    Ji, Jj = R.edge_jacobians(UVU, cam, pt, K)
    Mi, Mj = R.edge_jacobians(UV, cam, pt, K)
    assert np.array_equal(Ji[:, :2], Mi) and np.array_equal(Jj[:, :2], Mj)
    K5 = np.stack([K[:, 0], K[:, 0], K[:, 1], K[:, 2], K[:, 0] * K[:, 3]], axis=1)
    Si, Sj = stereo_ref.edge_jacobians(cam, pt, K5)
    for A, B in ((Ji, Si), (Jj, Sj)):
        assert np.max(np.abs(A - B)) <= 64 * np.finfo(np.float64).eps * np.max(np.abs(B))


def test_double_baseline_is_visible_in_the_single_edge_error():
    """f = 1003, b = 0.1, |e| ~ 1e-3: the third row computed the stereo edge's way (u - float(f b) / z) moves chi2 by
    8.9e-4 relative, far above the 1e-12 the device is pinned to in test_gpu_camparams.test_single_edge_pin."""
    g = R.Graph(R.single_edge_case())
    e = g.errors(UVU)
    assert 5e-4 < np.linalg.norm(e) < 2e-3
    a, b = g.chi2(), g.chi2(float_bf=True)
    rel = abs(a - b) / a
    print(f"single XYZ2UVU edge: chi2 all-double {a:.17g}, with a float f*b {b:.17g}, rel {rel:.3e}")
    assert rel >= 1e-6


def test_generators_and_twins():
    for stereo in (False, True):
        a, b = synth.ba_camparams(12, 150, 5, 8, stereo=stereo), synth.ba_camparams(12, 150, 5, 8, stereo=stereo)
        assert len(a.edges) == 1
        e = a.edges[0]
        D = 3 if stereo else 2
        assert e.etype == (UVU if stereo else UV) and e.meas.shape == (750, D) and e.info.shape == (750, D, D)
        assert e.params.shape == (750, 4) and np.all(e.params == [1000.0, 320.0, 240.0, 0.1])
        assert np.array_equal(e.meas, b.edges[0].meas)
        assert int(a.vertices[0].fixed.sum()) == (1 if stereo else 2)
        # ba()'s scene: the same vertices, and with f = 1000 the same left-image measurements to rounding
        base = synth.ba(12, 150, 5, 8, fixed_cameras=1 if stereo else 2)
        assert np.array_equal(a.vertices[1].est, base.vertices[1].est)
        assert np.max(np.abs(e.meas[:, :2] - base.edges[0].meas)) <= 1e-9
        tw = synth.camparams_twin(a)
        t = tw.edges[0]
        if stereo:
            assert t.etype == synth.E_STEREO_SE3_PROJECT_XYZ and np.all(t.params == [1000.0, 1000.0, 320.0, 240.0, 100.0])
        else:
            assert t.etype == synth.E_SE3_PROJECT_XYZ and np.all(t.params == [1000.0, 1000.0, 320.0, 240.0])
        assert np.array_equal(t.meas, e.meas) and np.array_equal(t.v0, e.v0)
    # the stereo measurement is stereocam_uvu_map's: noise-free, the third row vanishes at the true scene
    clean = synth.ba_camparams(12, 150, 5, 8, stereo=True, pixel_noise=0.0, disparity_noise=0.0, cam_rot_noise=0.0,
                               cam_trans_noise=0.0, point_noise=0.0, focal=512.0, baseline=0.125)
    assert np.max(np.abs(R.Graph(clean).errors(UVU))) <= 1e-9
    mixed = synth.ba_camparams(12, 150, 5, 8, stereo_fraction=0.6)
    assert [s.etype for s in mixed.edges] == [UVU, UV] and sum(len(s.v0) for s in mixed.edges) == 750
    assert 0.5 < len(mixed.edges[0].v0) / 750 < 0.7
    # the twin of the all-double graph with bf exact in float has the same chi2 to rounding
    p = synth.ba_camparams(12, 150, 5, 8, stereo=True, focal=512.0, baseline=0.125)
    t = synth.camparams_twin(p)
    a, b = R.Graph(p).chi2(), stereo_ref.StereoGraph(t).chi2()
    assert abs(a - b) <= 1e-12 * b


def test_file_formats_round_trip(tmp_path):
    """The reference-format writer and reader of camparams_ref agree: two distinct records (baselines included), the
    edges' ids, measurements and information come back bit for bit."""
    prob = R.two_record_problem()
    path = str(tmp_path / "a.g2o")
    recs, pid = R.write_g2o(prob, path)
    assert len(recs) == 2 and recs[0][3] != recs[1][3]
    got_recs, got_edges = R.read_g2o(path)
    assert got_recs == dict(enumerate(recs))
    e = prob.edges[0]
    assert len(got_edges) == len(e.v0)
    for k, ge in enumerate(got_edges):
        assert ge[:3] == (e.v0[k], e.v1[k], pid[k])
        assert ge[3:] == (e.meas[k, 0], e.meas[k, 1], e.info[k, 0, 0], e.info[k, 0, 1], e.info[k, 1, 1])
        assert tuple(e.params[k]) == got_recs[ge[2]]


def test_python_constants_equal_the_header():
    import g2o_amd
    text = open(os.path.join(ROOT, "include", "g2o_hip.h")).read()

    def define(name):
        return int(re.search(rf"#define {name}\s+(\d+)u?\b", text).group(1))

    assert g2o_amd.E_PROJECT_XYZ2UV == synth.E_PROJECT_XYZ2UV == define("G2OHIP_E_PROJECT_XYZ2UV") == 23
    assert g2o_amd.E_PROJECT_XYZ2UVU == synth.E_PROJECT_XYZ2UVU == define("G2OHIP_E_PROJECT_XYZ2UVU") == 24
    assert g2o_amd.LOAD_CAMERAPARAMS == define("G2OHIP_LOAD_CAMERAPARAMS") == 32
    assert [synth.ERR_DIM[t] for t in KINDS] == [2, 3] and [synth.MEAS_DIM[t] for t in KINDS] == [2, 3]
    assert [synth.PARAM_DIM[t] for t in KINDS] == [4, 4]
