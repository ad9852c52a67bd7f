"""The slam3d landmark edges without a GPU: the constants, the numpy reference (tests/slam3d_ref.py) against central
differences and, for its EdgeSE3 restatement, against the oracle, the generator, and the float64 precision of the chi2
the GPU tests pin at 1e-12."""
import os
import re

import numpy as np
import pytest

import slam3d_ref
import unary_ref
from g2o_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "g2o_hip.h")
RNG = np.random.default_rng(20261020)


def test_constants_agree_with_header(g2o_amd_mod):
    text = open(HEADER).read()
    h = {k: int(v) for k, v in re.findall(r"#define G2OHIP_(E_SE3_XYZ[A-Z_]*) +(\d+)", text)}
    assert h == {"E_SE3_XYZ": 7, "E_SE3_XYZ_DEPTH": 8, "E_SE3_XYZ_DISPARITY": 9}
    for name, val in h.items():
        assert getattr(g2o_amd_mod, name) == val == getattr(synth, name)
        assert synth.MEAS_DIM[val] == 3 and synth.ERR_DIM[val] == 3
    assert int(re.search(r"#define G2OHIP_LOAD_SLAM3D (\d+)u", text).group(1)) == g2o_amd_mod.LOAD_SLAM3D == 2
    assert g2o_amd_mod.LOAD_SLAM3D & g2o_amd_mod.LOAD_UNARY == 0  # the two flags combine


def _rand_iso(scale=1.0):
    aa = RNG.uniform(-1, 1, 3) + RNG.uniform(-1, 1, 3)
    R = synth._axis_angle(aa[None], np.array([np.linalg.norm(aa) * scale]))[0]
    return np.concatenate([RNG.uniform(-1, 1, 3) * scale, synth.rot_to_quat(R[None])[0]])


def _rand_case(etype):
    """A random pose, a non-identity offset, non-square K and a point 1.5 to 6 in front of the sensor."""
    pose, off = _rand_iso(), _rand_iso(0.3)
    par = off if etype == synth.E_SE3_XYZ else np.concatenate([off, [RNG.uniform(200, 600), RNG.uniform(200, 600),
                                                                     RNG.uniform(100, 400), RNG.uniform(100, 300)]])
    pn = np.array([RNG.uniform(-1, 1), RNG.uniform(-1, 1), RNG.uniform(1.5, 6)])
    pt = pose[:3] + unary_ref._R(pose[3:7]) @ (off[:3] + unary_ref._R(off[3:7]) @ pn)
    return pose, pt, par


@pytest.mark.parametrize("etype", slam3d_ref.KINDS)
def test_jacobians_vs_numeric(etype):
    """Analytic against central differences through the vertices' own oplus (unary_ref.oplus), within 1e-6 as
    test_prior_jacobian_vs_numeric. The step is 1e-6, not 1e-9: the camera errors are pixels (up to ~1e3), so their
    rounding (~1e-13) over 2 * 1e-9 would alone be ~1e-4; at 1e-6 it is ~1e-7 and the truncation, step^2 times a third
    derivative of ~1e3, is ~1e-9."""
    worst, delta = 0.0, 1e-6
    for _ in range(500):
        pose, pt, par = _rand_case(etype)
        z = np.zeros(3)
        Ji, Jj = slam3d_ref.jacobians(etype, pose, pt, par)
        Ni, Nj = np.zeros_like(Ji), np.zeros_like(Jj)
        for k in range(6):
            u = np.zeros(6)
            u[k] = delta
            ep = slam3d_ref.error(etype, unary_ref.oplus(synth.V_SE3_QUAT, pose, u), pt, z, par)
            em = slam3d_ref.error(etype, unary_ref.oplus(synth.V_SE3_QUAT, pose, -u), pt, z, par)
            Ni[:, k] = (ep - em) / (2 * delta)
        for k in range(3):
            u = np.zeros(3)
            u[k] = delta
            ep = slam3d_ref.error(etype, pose, unary_ref.oplus(synth.V_XYZ, pt, u), z, par)
            em = slam3d_ref.error(etype, pose, unary_ref.oplus(synth.V_XYZ, pt, -u), z, par)
            Nj[:, k] = (ep - em) / (2 * delta)
        worst = max(worst, np.abs(Ji - Ni).max(), np.abs(Jj - Nj).max())
    print(f"type {etype}: worst |analytic - numeric| {worst:.2e}")
    assert worst < 1e-6, worst


def test_identity_offset_is_none():
    pose, pt, _ = _rand_case(synth.E_SE3_XYZ)
    z = RNG.uniform(-1, 1, 3)
    a = slam3d_ref.error(synth.E_SE3_XYZ, pose, pt, z, None)
    b = slam3d_ref.error(synth.E_SE3_XYZ, pose, pt, z, unary_ref.IDENT7)
    assert np.array_equal(a, b)
    assert np.allclose(a, unary_ref._R(pose[3:7]).T @ (pt - pose[:3]) - z, rtol=0, atol=1e-15)


def test_se3_edge_restatement_equals_oracle(oracle):
    """slam3d_ref.se3_edge (EdgeSE3 through unary_ref's prior forms) against the oracle's analytic linearizeOplus on a
    small sphere: the records agree to 1e-12 of the largest entry."""
    prob = synth.sphere(6, 6)
    es = prob.edges[0]
    n = len(es.v0)
    rec = oracle.OracleGraph(prob).edge_payload(np.arange(n), n * 78, False).reshape(n, 78)
    g = slam3d_ref.Graph(prob)
    worst = 0.0
    for k in range(n):
        e, ((_, Ji), (_, Jj)) = g.edge(es, k)
        mine = np.concatenate([e, Ji.ravel(), Jj.ravel()])
        worst = max(worst, np.abs(mine - rec[k]).max() / np.abs(rec[k]).max())
    print(f"EdgeSE3 restatement against the oracle: {worst:.2e}")
    assert worst <= 1e-12, worst


def test_generator_deterministic_and_pure():
    kw = dict(kind=slam3d_ref.KINDS, offset=slam3d_ref.OFFSET, seed=5)
    a, b = synth.slam3d_landmarks(12, 80, **kw), synth.slam3d_landmarks(12, 80, **kw)
    assert [e.etype for e in a.edges] == [synth.E_SE3_QUAT, *slam3d_ref.KINDS]
    for x, y in zip(a.edges, b.edges):
        assert np.array_equal(x.v0, y.v0) and np.array_equal(x.v1, y.v1)
        assert np.array_equal(x.meas, y.meas) and np.array_equal(x.info, y.info)
    for x, y in zip(a.vertices, b.vertices):
        assert np.array_equal(x.est, y.est)
    c = synth.slam3d_landmarks(12, 80, kind=slam3d_ref.KINDS, offset=slam3d_ref.OFFSET, seed=6)
    assert not np.array_equal(c.edges[1].meas, a.edges[1].meas)
    poses, pts = a.vertices
    assert poses.vtype == synth.V_SE3_QUAT and pts.vtype == synth.V_XYZ
    assert poses.fixed[0] == 1 and poses.fixed[1:].sum() == 0 and pts.marginalized.all() and not poses.marginalized.any()
    odo = a.edges[0]
    assert np.array_equal(odo.v0 + 1, odo.v1) and len(odo.v0) == 11
    for es in a.edges[1:]:
        assert np.isin(es.v0, poses.ids).all() and np.isin(es.v1, pts.ids).all()  # pose first, then the point
        assert np.all(np.linalg.eigvalsh(es.info) > 0) and np.abs(es.info[:, 0, 1]).min() > 0  # SPD, not diagonal
        assert es.params.shape == (len(es.v0), 7 if es.etype == synth.E_SE3_XYZ else 11)
    assert np.array_equal(a.edges[1].v1, a.edges[2].v1)  # the kinds observe the same (pose, point) pairs
    # the measured sensor-frame depth: z >= 1 in the ground truth, so the noisy one is well above 0.9
    assert a.edges[1].meas[:, 2].min() > 0.9 and a.edges[2].meas[:, 2].min() > 0.9
    assert (1 / a.edges[3].meas[:, 2]).min() > 0.9
    assert synth.slam3d_landmarks(5, 10).edges[1].params is None  # XYZ without an offset: NULL params
    # the other generators draw from their own streams: one of them before and after a call here
    s0 = synth.slam2d(20)
    synth.slam3d_landmarks(5, 10)
    s1 = synth.slam2d(20)
    assert all(np.array_equal(x.meas, y.meas) for x, y in zip(s0.edges, s1.edges))


@pytest.mark.parametrize("case", ["one7", "one8", "one9", "traj", "traj_noisy"])
def test_chi2_precision_of_pin_cases(case):
    """The initial chi2 of the cases the GPU tests pin at 1e-12, in float64 and in np.longdouble: they agree to 1e-13,
    so the device pin tests the device and not the cancellation in pi.xy / pi.z - z."""
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps, "np.longdouble is no wider than float64 here"
    prob = slam3d_ref.one_edge(int(case[3:])) if case.startswith("one") else slam3d_ref.traj_problem(case == "traj_noisy")
    g = slam3d_ref.Graph(prob)
    lo, hi = g.chi2_in(np.float64), g.chi2_in(np.longdouble)
    rel = float(abs(hi - np.longdouble(lo)) / hi)
    print(f"{case}: chi2 float64 {float(lo):.17g} longdouble {float(hi):.20g} rel {rel:.2e} (margin {1e-13 / max(rel, 1e-30):.1f}x)")
    assert hi > 0 and rel <= 1e-13, rel
    assert abs(g.chi2(only=slam3d_ref.KINDS) - float(lo)) <= 1e-14 * float(lo)  # chi2_in restates Graph.chi2
