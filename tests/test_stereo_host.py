"""EdgeStereoSE3ProjectXYZ on the host (no GPU): the numpy restatement the GPU tests compare against
(tests/stereo_ref.py) checked against central differences, the stereo generator, the public constants, and the
size of the float-rounded bf in the error."""
import os
import re

import numpy as np

import stereo_ref
from g2o_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_jacobians_against_central_differences():
    """50 random edges, step 1e-6 through oplus. With |e''| h^2 / 6 and eps |e| / h both around 1e-9 of the largest
    Jacobian entry, 1e-6 of it leaves a thousandfold margin and still catches any wrong term."""
    rng = np.random.default_rng(17)
    n = 50
    ang = rng.standard_normal((n, 3)) * 0.3
    q, _ = stereo_ref.se3_exp(np.concatenate([ang, np.zeros((n, 3))], axis=1))
    cam = np.concatenate([rng.standard_normal((n, 3)) * 0.5, q], axis=1)
    pc = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.0, 1.0, n), rng.uniform(2.0, 6.0, n)], axis=1)
    # world points whose camera-frame coordinates are pc: X = R^T (pc - t)
    R = stereo_ref.quat_to_R(q)
    pt = np.einsum("nji,nj->ni", R, pc - cam[:, :3])
    assert np.allclose(stereo_ref.cam_map(cam, pt), pc, atol=1e-12)
    K = np.stack([rng.uniform(400, 1200, n), rng.uniform(400, 1200, n), rng.uniform(300, 340, n),
                  rng.uniform(220, 260, n), rng.uniform(40, 400, n)], axis=1)
    meas = rng.standard_normal((n, 3))
    Ji, Jj = stereo_ref.edge_jacobians(cam, pt, K)
    h = 1e-6
    # the differenced error uses the double bf, as the analytic Jacobians do (the float rounding is a constant offset
    # of the error's third row and would cancel anyway)
    err = lambda c, p: stereo_ref.edge_error(c, p, meas, K, float_bf=False)
    Ni, Nj = np.empty_like(Ji), np.empty_like(Jj)
    for k in range(3):
        d = np.zeros((n, 3))
        d[:, k] = h
        Ni[:, :, k] = (err(cam, pt + d) - err(cam, pt - d)) / (2 * h)
    for k in range(6):
        d = np.zeros((n, 6))
        d[:, k] = h
        Nj[:, :, k] = (err(stereo_ref.oplus_cam(cam, d), pt) - err(stereo_ref.oplus_cam(cam, -d), pt)) / (2 * h)
    scale = max(np.abs(Ji).max(), np.abs(Jj).max())
    ei, ej = np.abs(Ni - Ji).max() / scale, np.abs(Nj - Jj).max() / scale
    print(f"stereo Jacobians against central differences: point {ei:.2e}, camera {ej:.2e} of the largest entry")
    assert ei <= 1e-6 and ej <= 1e-6


def test_ba_stereo_generator():
    a = synth.ba_stereo(12, 150, obs_per_point=5, window=8)
    b = synth.ba_stereo(12, 150, obs_per_point=5, window=8)
    mono = synth.ba(12, 150, obs_per_point=5, window=8)
    assert len(a.edges) == 1
    ea, eb, em = a.edges[0], b.edges[0], mono.edges[0]
    assert ea.etype == synth.E_STEREO_SE3_PROJECT_XYZ
    for x, y in ((ea.meas, eb.meas), (ea.params, eb.params), (ea.info, eb.info), (ea.v0, eb.v0), (ea.v1, eb.v1)):
        assert np.array_equal(x, y)
    n = 150 * 5
    assert ea.meas.shape == (n, 3) and ea.info.shape == (n, 3, 3) and ea.params.shape == (n, 5)
    assert synth.MEAS_DIM[ea.etype] == 3 and synth.ERR_DIM[ea.etype] == 3
    assert (a.pose_dim, a.landmark_dim) == (6, 3)
    # the scene of ba(): vertices, observation lists, left-image measurements and intrinsics
    for va, vm in zip(a.vertices, mono.vertices):
        assert np.array_equal(va.est, vm.est) and np.array_equal(va.ids, vm.ids) and np.array_equal(va.fixed, vm.fixed)
    assert np.array_equal(ea.v0, em.v0) and np.array_equal(ea.v1, em.v1)
    assert np.array_equal(ea.meas[:, :2], em.meas) and np.array_equal(ea.params[:, :4], em.params)
    assert np.all(ea.params[:, 4] == 100.3)
    assert np.all(ea.meas[:, 0] - ea.meas[:, 2] > 0), "a disparity that is not positive"
    big = synth.ba_stereo(40, 1500)
    assert np.all(big.edges[0].meas[:, 0] - big.edges[0].meas[:, 2] > 0)
    # arguments reach the edges
    c = synth.ba_stereo(12, 150, obs_per_point=5, window=8, bf=55.5, info=np.diag([1.0, 2.0, 3.0]))
    assert np.all(c.edges[0].params[:, 4] == 55.5) and np.array_equal(c.edges[0].info[7], np.diag([1.0, 2.0, 3.0]))
    assert np.array_equal(c.edges[0].meas[:, :2], em.meas)


def test_ba_stereo_mixed_partitions_the_observations():
    mono = synth.ba(12, 150, obs_per_point=5, window=8).edges[0]
    mix = synth.ba_stereo(12, 150, obs_per_point=5, window=8, stereo_fraction=0.6)
    assert [e.etype for e in mix.edges] == [synth.E_STEREO_SE3_PROJECT_XYZ, synth.E_SE3_PROJECT_XYZ]
    st, mo = mix.edges
    assert len(st.v0) + len(mo.v0) == len(mono.v0)
    assert 0.5 * len(mono.v0) < len(st.v0) < 0.7 * len(mono.v0)
    assert mo.meas.shape[1] == 2 and mo.params.shape[1] == 4 and st.meas.shape[1] == 3 and st.params.shape[1] == 5
    key = lambda e: sorted(zip(e.v0.tolist(), e.v1.tolist()))
    both = sorted(key(st) + key(mo))
    assert both == key(mono)
    assert len(set(both)) == len(both)
    # every observation keeps its left-image measurement
    full = {(a, b): tuple(m) for a, b, m in zip(mono.v0.tolist(), mono.v1.tolist(), mono.meas.tolist())}
    for e in (st, mo):
        for a, b, m in zip(e.v0.tolist(), e.v1.tolist(), e.meas.tolist()):
            assert full[(a, b)] == tuple(m[:2])


def test_ba_unchanged_by_the_scene_refactoring():
    """ba() is a view of the scene ba_stereo() shares: same draws in the same order (the golden fixtures and
    test_synth_deterministic_and_shapes guard the values; this guards the call path)."""
    a = synth.ba(12, 150, obs_per_point=5, window=8)
    s, pc, uv_true = synth._ba_scene(12, 150, 5, 8, 1.0, 0.002, 0.01, 0.05, 2, synth.SEED)
    assert np.array_equal(a.edges[0].meas, s.edges[0].meas)
    assert pc.shape == (750, 3) and uv_true.shape == (750, 2) and np.all(pc[:, 2] > 0)


def test_constants_match_the_header():
    import g2o_amd
    text = open(os.path.join(ROOT, "include", "g2o_hip.h")).read()
    m = re.search(r"#define\s+G2OHIP_E_STEREO_SE3_PROJECT_XYZ\s+(\d+)", text)
    assert m, "the header does not define G2OHIP_E_STEREO_SE3_PROJECT_XYZ"
    assert int(m.group(1)) == g2o_amd.E_STEREO_SE3_PROJECT_XYZ == synth.E_STEREO_SE3_PROJECT_XYZ == 6


def test_float_bf_is_visible_in_the_single_edge_error():
    """bf = 100.3 rounded to float moves u_r by (bf - float(bf)) / z; with |e| ~ 1e-3 that is far more than the
    1e-9 relative the GPU pin needs to tell the two apart (it checks chi2 to 1e-12)."""
    prob = stereo_ref.single_edge_case()
    g = stereo_ref.StereoGraph(prob)
    e32, e64 = g.errors(float_bf=True), g.errors(float_bf=False)
    assert 0.5e-3 < np.linalg.norm(e32) < 2e-3
    rel = np.linalg.norm(e32 - e64) / np.linalg.norm(e32)
    print(f"float-rounded bf: relative change of the error {rel:.3e}")
    assert rel > 1e-9
    c32, c64 = g.chi2(float_bf=True), g.chi2(float_bf=False)
    assert abs(c32 - c64) > 1e-9 * c32
