"""EdgeSE3Expmap and the pose-only projections without a GPU: the constants, the numpy reference (tests/expmap_ref.py)
against central differences, SE3Quat's log / exp, the generators, the float64 precision of the chi2 the GPU tests pin at
1e-12 and the measurement behind the tolerance of the one case inside acos' ill-conditioned band.

No part of the .g2o reader or writer runs without a device (a graph cannot be created), so the EDGE_SE3:EXPMAP file
tests are all in tests/test_gpu_expmap.py."""
import os
import re

import numpy as np
import pytest

import expmap_ref as ref
import unary_ref
from g2o_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "g2o_hip.h")
RNG = np.random.default_rng(20261021)


def test_constants_agree_with_header(g2o_amd_mod):
    text = open(HEADER).read()
    want = {"E_SE3_EXPMAP": 10, "E_SE3_PROJECT_XYZ_ONLYPOSE": 21, "E_STEREO_SE3_PROJECT_XYZ_ONLYPOSE": 22}
    for name, val in want.items():
        assert int(re.search(rf"#define G2OHIP_{name} +(\d+)", text).group(1)) == val
        assert getattr(g2o_amd_mod, name) == val == getattr(synth, name)
    assert (synth.MEAS_DIM[10], synth.ERR_DIM[10]) == (7, 6)
    assert (synth.MEAS_DIM[21], synth.ERR_DIM[21]) == (2, 2) and (synth.MEAS_DIM[22], synth.ERR_DIM[22]) == (3, 3)
    assert int(re.search(r"#define G2OHIP_LOAD_EXPMAP (\d+)u", text).group(1)) == g2o_amd_mod.LOAD_EXPMAP == 4
    assert g2o_amd_mod.LOAD_EXPMAP & (g2o_amd_mod.LOAD_UNARY | g2o_amd_mod.LOAD_SLAM3D) == 0  # the flags combine
    # the unary type range of the C ABI stays clear of the host-J escape
    assert 22 < g2o_amd_mod.E_HOSTJ(1) and synth.PRIOR_VERTEX.keys().isdisjoint(synth.POSE_ONLY_VERTEX)


def _rand_T(scale=1.0):
    return ref.exp(np.concatenate([RNG.uniform(-1, 1, 3) * scale, RNG.uniform(-2, 2, 3)]))


@pytest.mark.parametrize("etype", ref.POSE_ONLY)
def test_pose_only_jacobian_vs_numeric(etype):
    """The analytic Jacobian against central differences of the double-precision error (the stereo type with a double
    1/z: the float one is a step function at this scale) under exp(u) * T. Step 1e-6 and bound 1e-6 as
    test_slam3d_host.py: the errors are pixels (up to ~1e3), their rounding ~1e-13 over 2e-6 is ~1e-7, the truncation
    step^2 times a third derivative of ~1e3 is ~1e-9."""
    worst, delta = 0.0, 1e-6
    for _ in range(300):
        T = _rand_T()
        pc = np.array([RNG.uniform(-1, 1), RNG.uniform(-1, 1), RNG.uniform(1.5, 6)])
        xw = ref.qrot(ref.inv(T)[3:7], pc - T[:3])
        par = np.concatenate([xw, [RNG.uniform(200, 600), RNG.uniform(200, 600), RNG.uniform(100, 400),
                                   RNG.uniform(100, 300), RNG.uniform(20, 120)]])
        par = par[:7] if etype == ref.E_MONO else par
        J = ref.pose_only_jacobian(etype, T, par)
        N = np.zeros_like(J)
        z = np.zeros(J.shape[0])
        for k in range(6):
            u = np.zeros(6)
            u[k] = delta
            ep = ref.pose_only_error(etype, unary_ref.oplus(synth.V_SE3_EXPMAP, T, u)[0], par, z, float_invz=False)
            em = ref.pose_only_error(etype, unary_ref.oplus(synth.V_SE3_EXPMAP, T, -u)[0], par, z, float_invz=False)
            N[:, k] = (ep - em) / (2 * delta)
        worst = max(worst, np.abs(J - N).max())
    print(f"type {etype}: worst |analytic - numeric| {worst:.2e}")
    assert worst < 1e-6, worst


def test_stereo_float_invz():
    """The stereo type's error sees 1/z rounded to float: it differs from the double-1/z error, by no more than the
    float rounding (2^-24 relative on terms of up to fx x/z + bf/z)."""
    p = ref.one_pose_only(ref.E_STEREO)
    T, es = p.vertices[0].est[0], p.edges[0]
    a = ref.pose_only_error(ref.E_STEREO, T, es.params[0], es.meas[0])
    b = ref.pose_only_error(ref.E_STEREO, T, es.params[0], es.meas[0], float_invz=False)
    d = np.abs(a - b)
    assert d.max() > 0 and d.max() <= 2.0 ** -24 * (260.0 * 0.4 / 3.7 + 30.0 / 3.7) * 1.01, d


def test_expmap_jacobians_at_zero_residual():
    """At zero residual (C = Tj Ti^-1) the reference's Ji = adj(Tj^-1 C) and Jj = -adj(Ti^-1 C^-1) are the derivative
    of log(Tj^-1 C Ti) under exp(u) * T: central differences with step 1e-6 agree to 1e-6 of the largest entry (the
    rounding of an error of ~1e-6 made of translations of ~5 is ~1e-15 over 2e-6; the truncation ~1e-12)."""
    worst, delta = 0.0, 1e-6
    for _ in range(100):
        Ti, Tj = _rand_T(), _rand_T()
        C = ref.mul(Tj, ref.inv(Ti))
        assert np.abs(ref.expmap_error(Ti, Tj, C)).max() < 1e-14
        Ji, Jj = ref.expmap_jacobians(Ti, Tj, C)
        Ni, Nj = np.zeros((6, 6)), np.zeros((6, 6))
        for k in range(6):
            u = np.zeros(6)
            u[k] = delta
            op = lambda T, s: unary_ref.oplus(synth.V_SE3_EXPMAP, T, s * u)[0]
            Ni[:, k] = (ref.expmap_error(op(Ti, 1), Tj, C) - ref.expmap_error(op(Ti, -1), Tj, C)) / (2 * delta)
            Nj[:, k] = (ref.expmap_error(Ti, op(Tj, 1), C) - ref.expmap_error(Ti, op(Tj, -1), C)) / (2 * delta)
        scale = max(np.abs(Ji).max(), np.abs(Jj).max())
        worst = max(worst, np.abs(Ji - Ni).max() / scale, np.abs(Jj - Nj).max() / scale)
    print(f"EdgeSE3Expmap at zero residual: worst |analytic - numeric| / max|J| {worst:.2e}")
    assert worst < 1e-6, worst


def test_log_exp_both_branches():
    """log(exp(x)) = x. The acos / tan branch to rounding (1e-12 relative; angles 0.05 to 2.5). The series branch
    (d > 0.99999, angles below 0.0044) takes omega = deltaR / 2 = (sin t / t) omega: short by t^2 / 6 relative, and its
    V^-1 is cut after the second-order term; the bound is 1.5 times that leading term."""
    for _ in range(200):
        ang = RNG.uniform(0.05, 2.5)
        ax = RNG.standard_normal(3)
        x = np.concatenate([ax / np.linalg.norm(ax) * ang, RNG.uniform(-2, 2, 3)])
        y = ref.log(ref.exp(x))
        assert np.linalg.norm(y - x) <= 1e-12 * np.linalg.norm(x), (x, y)
    for _ in range(200):
        ang = RNG.uniform(1e-4, 0.004)
        ax = RNG.standard_normal(3)
        x = np.concatenate([ax / np.linalg.norm(ax) * ang, RNG.uniform(-2, 2, 3)])
        T = ref.exp(x)
        R = ref.quat_to_R(T[3:7])
        assert 0.5 * (R[0, 0] + R[1, 1] + R[2, 2] - 1) > 0.99999  # the series branch
        y = ref.log(T)
        assert np.linalg.norm(y - x) <= 1.5 * ang * ang / 6 * np.linalg.norm(x) + 1e-15, (x, y)
    # adj(T) is the matrix of x -> log(T exp(x) T^-1) (what makes the edge's Jacobians the derivative at zero error)
    T, x = _rand_T(), np.array([1e-7, -2e-7, 1.5e-7, 2e-7, 1e-7, -1e-7])
    lhs = ref.log(ref.mul(ref.mul(T, ref.exp(x)), ref.inv(T)))
    assert np.linalg.norm(lhs - ref.adj(T) @ x) <= 1e-6 * np.linalg.norm(lhs)


def test_generators_deterministic_and_pure():
    before = synth.ba(10, 60), synth.sphere(5, 5), synth.slam3d_landmarks(6, 20)
    a, b = synth.expmap_pose_graph(40, 8, seed=5), synth.expmap_pose_graph(40, 8, seed=5)
    (va,), (ea,) = a.vertices, a.edges
    assert np.array_equal(va.est, b.vertices[0].est) and np.array_equal(ea.meas, b.edges[0].meas)
    assert not np.array_equal(synth.expmap_pose_graph(40, 8, seed=6).edges[0].meas, ea.meas)
    assert va.vtype == synth.V_SE3_EXPMAP and va.fixed[0] == 1 and va.fixed[1:].sum() == 0
    assert ea.etype == synth.E_SE3_EXPMAP and len(ea.v0) == 39 + 8
    assert np.array_equal(ea.v0[:39] + 1, ea.v1[:39]) and np.all(ea.v1[39:] > ea.v0[39:] + 1)
    assert np.all(np.linalg.eigvalsh(ea.info) > 0) and np.abs(ea.info[:, 0, 4]).min() > 0  # SPD, not diagonal
    g = ref.Graph(a)
    ang = g.residual_angles()
    assert ang[:39].max() < 1e-12 and ang[39:].max() > 1e-3  # chained odometry: zero error on it, drift on the loops
    t = synth.expmap_pose_graph(40, 8, seed=5, init="truth")
    assert 0 < ref.Graph(t).residual_angles().max() < 0.1  # at the true poses the error is the noise
    for stereo in (False, True):
        p = synth.pose_only(5, 30, stereo=stereo)
        (cams,), (es,) = p.vertices, p.edges
        assert cams.fixed.sum() == 0 and es.v1 is None and len(es.v0) == 150 and p.landmark_dim == 0
        assert es.etype == (ref.E_STEREO if stereo else ref.E_MONO) and es.params.shape == (150, 8 if stereo else 7)
        assert set(es.v0) == set(cams.ids) and np.abs(es.info[:, 0, 1]).min() > 0
        z = np.array([ref.qrot(cams.est[c, 3:7], x)[2] + cams.est[c, 2] for c, x in zip(es.v0, es.params[:, :3])])
        assert z.min() > 2.5  # every point in front of its camera
        tw = synth.pose_only_twin(p)
        assert tw.edges[0].etype == synth.POSE_ONLY_BINARY[es.etype] and tw.vertices[1].fixed.all()
        assert np.array_equal(tw.edges[0].v1, es.v0) and np.array_equal(tw.vertices[1].est, es.params[:, :3])
        gt, gp = ref.Graph(tw), ref.Graph(p)
        assert gt.order == gp.order
        rel = abs(gt.chi2() - gp.chi2()) / gp.chi2()
        assert rel <= (1e-6 if stereo else 1e-14), rel  # exact for the monocular type, float rounding for stereo
    base = synth.ba(12, 100, obs_per_point=4, window=6)
    w = synth.with_pose_only(base, every=3, per_camera=5)
    assert w.edges[0] is base.edges[0] and len(w.edges) == 2 and w.edges[1].etype == ref.E_MONO
    assert set(w.edges[1].v0) <= set(base.vertices[0].ids[::3]) and 0 in w.edges[1].v0  # a fixed camera among them
    after = synth.ba(10, 60), synth.sphere(5, 5), synth.slam3d_landmarks(6, 20)
    for x, y in zip(before, after):  # the other generators' streams are their own
        assert all(np.array_equal(p.est, q.est) for p, q in zip(x.vertices, y.vertices))
        assert all(np.array_equal(p.meas, q.meas) for p, q in zip(x.edges, y.edges))


@pytest.mark.parametrize("case", ["mono", "stereo", "small", "regular", "wneg", "stage65", "stage257"])
def test_chi2_precision_of_pin_cases(case):
    """The chi2 of the cases the GPU tests pin at 1e-12, in float64 and in np.longdouble: they agree to 1e-13, so the
    device pin tests the device and not a cancellation in the case. The EdgeSE3Expmap cases hold no residual angle
    inside acos' band."""
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps, "np.longdouble is no wider than float64 here"
    if case in ("mono", "stereo"):
        prob = ref.one_pose_only(ref.E_MONO if case == "mono" else ref.E_STEREO)
    elif case.startswith("stage"):
        prob = ref.expmap_case(int(case[5:]) - 2, 3, 500 + int(case[5:]))
    else:
        prob = ref.one_expmap(case)
    g = ref.Graph(prob)
    if prob.edges[0].etype == ref.E_EXPMAP:
        ref.assert_outside_band(g.residual_angles())
    lo, hi = g.chi2_in(np.float64), g.chi2_in(np.longdouble)
    rel = float(abs(hi - np.longdouble(lo)) / hi)
    print(f"{case}: chi2 float64 {float(lo):.17g} longdouble {float(hi):.20g} rel {rel:.2e}")
    assert hi > 0 and rel <= 1e-13, rel
    assert abs(g.chi2() - float(lo)) <= 1e-14 * float(lo)  # chi2_in restates Graph.chi2
    if case == "wneg":
        es, est = prob.edges[0], prob.vertices[0].est
        _, (w1, _) = ref.expmap_error(est[0], est[1], es.meas[0], raw=True)
        assert w1 < -0.1, w1  # the quaternion of Tj^-1 * C before normalisation


def test_band_tolerance():
    """acos(d) near 1: the chi2 of the one case whose residual angles all lie inside the band (0.0045, 0.05), in
    float64 and in np.longdouble. Their relative difference is expmap_ref.BAND_MEASURED (the constant holds the value
    rounded up; the measurement must not exceed it nor fall below a quarter of it, or the constant is stale), and
    the GPU test's tolerance for this case is 4 times the constant."""
    assert np.finfo(np.longdouble).eps < np.finfo(np.float64).eps
    g = ref.Graph(ref.band_case())
    ang = g.residual_angles()
    assert ang.min() > 0.0045 and ang.max() < 0.05, (ang.min(), ang.max())
    lo, hi = g.chi2_in(np.float64), g.chi2_in(np.longdouble)
    rel = float(abs(hi - np.longdouble(lo)) / hi)
    print(f"band case: chi2 float64 {float(lo):.17g} longdouble {float(hi):.20g} rel {rel:.3e}; "
          f"BAND_MEASURED {ref.BAND_MEASURED:.2e} BAND_TOL {ref.BAND_TOL:.2e}")
    assert ref.BAND_MEASURED / 4 <= rel <= ref.BAND_MEASURED, rel
    assert ref.BAND_TOL == 4 * ref.BAND_MEASURED
