"""CPU checks of tests/sim3_project_ref.py, the reference the GPU tests of the Sim3 projection edges compare against: its
analytic Jacobians against central differences in longdouble through sim3_ref.oplus (both directions, both fix_scale
states, near and far points, small and large scales, a quaternion that is not unit length and one with w < 0); their
agreement with sim3_ref.project_records; the float64 floor of chi2, in total and per edge, on every case and state the
GPU tests compare at 1e-12; the LM decisions of the trajectory cases in float64 against longdouble; the generators; the
Python constants against the header; the .g2o line formats."""
import os
import re

import numpy as np
import pytest

import sim3_project_ref as P
import sim3_ref as S
from g2o_amd import synth
from test_pose_edges_host import _numeric, _worst
from test_sim3_host import JTOL

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEAR_CAM = P.DEFAULT_CAM  # see jacobian_cases


def _plus(fix_scale):
    return lambda x, u: S.oplus(x, u, fix_scale, LD)[0]


def _point_plus(x, u):
    return x + u


def jacobian_cases():
    """[(label, point, Sim3, camera, inverse)]: the mapped point at depth 3-6 and at depth 0.5, scales 0.5, 1.2 and 3 in
    both directions; a Sim3 as oplus leaves it (the product of an exponential and a unit record: |q| off 1 by
    rounding), one scaled off unit length outright and one with w < 0, none of them normalised before the edge sees
    it.

    The camera of the near cases: the third derivatives of f x / z in the point grow as f s^3 / z^4, and with them the
    truncation error h^2 f''' / 6 of the central differences themselves. At depth 0.5 with f = 420 and s = 0.5 that error
    is 1.16e-9 on entries of 840 (measured; 4.65e-9 at h = 2e-6 and 3.05e-10 at h = 5e-7: it is the differences' own),
    and with f = 60 and s = 3 it is 1.64e-8, both over JTOL. So the near cases take the camera a VertexSim3Expmap is
    constructed with, 1 1 0 0, for which f s^3 h^2 / z^4 stays under 4.4e-10 on entries of order one; the far cases take
    the 400-pixel cameras."""
    rng = np.random.default_rng(8300)
    out = []
    for inverse in (False, True):
        cam = P.CAM2 if inverse else P.CAM1
        for scale in (0.5, 1.2, 3.0):
            for depth, c in (((3.0, 6.0), cam), ((0.5, 0.5), NEAR_CAM)):
                Sv = S._rand_sim3(rng, (scale, scale))
                pts, pc = P._points_seen_by(rng, Sv, 1, inverse, depth)
                out.append((f"inverse={inverse} s={scale} depth={pc[0, 2]:.2f}", pts[0], Sv, c, inverse))
        Sv = S.oplus(S._rand_sim3(rng), 0.3 * rng.standard_normal(7))[0]
        assert Sv[3:7] @ Sv[3:7] != 1.0
        out.append((f"inverse={inverse} after oplus", P._points_seen_by(rng, Sv, 1, inverse)[0][0], Sv, cam, inverse))
        Sv = S._rand_sim3(rng)
        pts = P._points_seen_by(rng, Sv, 1, inverse)[0][0]
        Sv[3:7] *= -1
        assert Sv[6] < 0
        out.append((f"inverse={inverse} w<0", pts, Sv, cam, inverse))
    return out


@pytest.mark.parametrize("fix_scale", [False, True])
def test_jacobians_vs_numeric(fix_scale):
    worst = 0.0
    for label, p, Sv, cam, inverse in jacobian_cases():
        p, Sv = np.asarray(p, LD), np.asarray(Sv, LD)
        Ji, Jj = P.jacobians(p, Sv, cam, inverse, fix_scale, LD)
        Ni, Nj = _numeric(lambda a, b: P.error(a, b, np.zeros(2), cam, inverse, LD)[0], (p, Sv),
                          (_point_plus, _plus(fix_scale)), (3, 7))
        w = _worst([(Ji[0], Ni), (Jj[0], Nj)])
        print(f"{label} fix_scale={fix_scale}: worst entry {w:.2e} of {float(np.abs(Nj).max()):.3g}")
        worst = max(worst, w)
        assert w <= JTOL, (label, w)
        if fix_scale:
            assert not Jj[0][:, 6].any() and not Nj[:, 6].any()
        elif inverse:
            assert Jj[0][:, 6].any()
        else:  # the forward edge's column 6 is -P x = 0 in any state (to rounding): scaling x leaves its projection
            assert np.abs(Jj[0][:, 6]).max() < 1e-12 and np.abs(Nj[:, 6]).max() < JTOL
    print(f"worst {worst:.2e}")


def test_near_points_through_the_pixel_cameras():
    """The depth-0.5 cases of jacobian_cases through the 400-pixel cameras, where plain central differences at h = 1e-6
    are themselves off by more than JTOL: Richardson's (4 D(h) - D(2h)) / 3 cancels their h^2 term and leaves h^4, so
    the near-point Jacobians are pinned at JTOL with realistic focal lengths too."""
    import test_pose_edges_host as T
    near = [c for c in jacobian_cases() if "depth=0.50" in c[0]]
    assert len(near) == 6
    for label, p, Sv, _, inverse in near:
        cam = P.CAM2 if inverse else P.CAM1
        p, Sv = np.asarray(p, LD), np.asarray(Sv, LD)
        Ji, Jj = P.jacobians(p, Sv, cam, inverse, False, LD)
        D = {}
        h0 = T.H
        try:
            for k in (1, 2):
                T.H = h0 * k
                D[k] = _numeric(lambda a, b: P.error(a, b, np.zeros(2), cam, inverse, LD)[0], (p, Sv),
                                (_point_plus, _plus(False)), (3, 7))
        finally:
            T.H = h0
        Ni, Nj = ((4 * D[1][m] - D[2][m]) / 3 for m in range(2))
        w = _worst([(Ji[0], Ni), (Jj[0], Nj)])
        print(f"{label} pixel camera: worst entry {w:.2e} of {float(np.abs(Nj).max()):.3g}")
        assert w <= JTOL, (label, w)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("fix_scale", [False, True])
def test_agrees_with_project_records(inverse, fix_scale):
    """sim3_ref.projection_problem's records are the reference's numeric linearizeOplus (h = 1e-6 in longdouble): the
    Jacobian columns, Ji and Jj, agree to the differences' own h^2 term."""
    prob, rec = S.projection_problem(inverse=inverse)
    est = prob.vertices[1].est[0]
    want = rec(est, fix_scale)[:, 2:]
    n = len(want)
    Sv = np.repeat(est[None], n, 0)
    got = P.records(prob.vertices[0].est, Sv, np.zeros((n, 2)), (420.0, 415.0, 320.0, 240.0), inverse, fix_scale)[:, 2:]
    rel = np.linalg.norm(got - want) / np.linalg.norm(want)
    print(f"inverse={inverse} fix_scale={fix_scale}: {rel:.2e}")
    assert rel <= 1e-12
    if fix_scale:
        assert not got[:, 6:].reshape(n, 2, 7)[:, :, 6].any() and not want[:, 6:].reshape(n, 2, 7)[:, :, 6].any()


def chi2_cases():
    """(name, problem, cameras) of every graph a GPU test takes chi2 of at 1e-12."""
    out = [(f"one inverse={i}", *P.one_edge(i)) for i in (False, True)]
    for inverse in (False, True):
        for two in (False, True):
            out += [(f"kernel ne={ne} inverse={inverse} two_cams={two}", *P.kernel_case(ne, inverse, two))
                    for ne in (1, 63, 64, 65, 257)]
    out.append(("optimize_sim3", *P.optimize_sim3_case()[:2]))
    out.append(("optimize_sim3 outliers", *P.optimize_sim3_case(outliers=6)[:2]))
    out.append(("mixed", *P.mixed_case()))
    return out


def test_chi2_float64_floor():
    """float64 against longdouble: in total on every case, and per edge on every graph and state at which a GPU test
    compares g2ohip_edge_chi2 (sim3_project_ref.edge_chi2_states). Under 1e-13, so the GPU tests compare at the project's
    1e-12 relative. No residual there is shorter than half a pixel (the generator's offsets are 3 to 6 px; the fit takes
    some of that)."""
    worst = 0.0
    for name, prob, cams in chi2_cases():
        g = P.Graph(prob, cams=cams)
        c64, c80 = g.chi2_in(np.float64), g.chi2_in(LD)
        rel = float(abs(LD(c64) - c80) / c80)
        print(f"{name}: chi2 {float(c80):.6g} float64 floor {rel:.2e}")
        worst = max(worst, rel)
    print(f"worst float64 floor {worst:.2e}")
    assert worst <= 1e-13, worst
    for name, prob, cams, est in P.edge_chi2_states():
        g = P.Graph(prob, cams=cams)
        for es in g.project_sets():
            e64, e80 = g.project_chi2(es.etype, est), g.project_chi2(es.etype, est, LD)
            rel = float(np.max(np.abs(e64.astype(LD) - e80) / e80))
            p, Sv, obs, cam, inv = g.project_batch(es, est)
            short = float(np.min(np.linalg.norm(P.error(p, Sv, obs, cam, inv), axis=1)))
            print(f"{name} type {es.etype}: per-edge floor {rel:.2e}, smallest chi2 {float(np.min(e80)):.3g}, "
                  f"shortest residual {short:.3g}")
            assert rel <= 1e-13 and short >= 0.5, (name, rel, short)


def test_generators():
    prob, cams, bad = P.optimize_sim3_case(outliers=6)
    again = P.optimize_sim3_case(outliers=6)[0]
    assert all(np.array_equal(a.meas, b.meas) for a, b in zip(prob.edges, again.edges))
    assert [es.etype for es in prob.edges] == [P.E_FWD, P.E_INV] and [len(es.v0) for es in prob.edges] == [24, 24]
    assert bad.sum() == 6 and cams[48][0] != cams[48][1] and prob.vertices[0].fixed.all()
    g = P.Graph(prob, cams=cams)
    chi = np.concatenate([g.project_chi2(t) for t in P.TYPES])
    assert chi[bad].min() > 9.21 > chi[~bad].max()  # 50 px against 3 to 6 px and the start's few pixels
    # every mapped point lies in front of its camera, in each generator
    for name, prob, cams in chi2_cases():
        g = P.Graph(prob, cams=cams)
        for es in g.project_sets():
            p, Sv, _, _, inv = g.project_batch(es)
            q, t, s = S.parts(S.inv(Sv) if inv else Sv)
            assert np.all((s[:, None] * S.qrot(q, p) + t)[:, 2] > 0.4), name
    prob, cams = P.kernel_case(257, False, True)
    assert len(np.unique(P.Graph(prob, cams=cams).cam_rows(prob.edges[0]), axis=0)) == 3
    prob, cams = P.kernel_case(257, True, False)
    assert len(np.unique(P.Graph(prob, cams=cams).cam_rows(prob.edges[0]), axis=0)) == 1
    tw = P.twin_problem(P.mixed_case()[0])
    assert [es.etype for es in tw.edges] == [S.E_SIM3, P.HJ2] and len(tw.edges[1].v0) == 24


def test_lm_decisions_clear_of_thresholds():
    """LM over the dense system in float64 and in longdouble, on the runs the GPU tests compare with the twin: the same
    accept / reject sequence and no rho within 1e-6 of zero, so the device and its twin take the same trials. The plain
    OptimizeSim3 case, the corrupted one under Huber, and what the chi2 = 9.21 cut leaves of it."""
    prob, cams, _ = P.optimize_sim3_case()
    bad_prob, _, corrupted = P.optimize_sim3_case(outliers=6)
    runs = [("plain", prob, None, 5, None), ("Huber, corrupted", bad_prob, P.HUBER, 5, None)]
    d = P.Dense(bad_prob, cams, robust=P.HUBER)
    S.lm(d, 5)
    g = P.Graph(bad_prob, cams=cams)
    drop = {t: g.project_chi2(t, {S.V_SIM3: d.est}) > 9.21 for t in P.TYPES}
    assert np.array_equal(np.concatenate([drop[t] for t in P.TYPES]), corrupted)  # the cut finds the six, no other
    runs.append(("Huber, inliers", P.without(bad_prob, drop), P.HUBER, 5, d.est))
    for name, pr, robust, iters, est in runs:
        a, b = S.lm(P.Dense(pr, cams, np.float64, robust, est), iters), S.lm(P.Dense(pr, cams, LD, robust, est), iters)
        print(name, [(f"{c:.6g}", t) for c, t, _ in a])
        assert [t for _, t, _ in a] == [t for _, t, _ in b], name
        assert all(abs(r) > 1e-6 for _, _, rs in b for r in rs), name
        assert a[-1][0] < a[0][0], name


def test_python_constants_equal_the_header():
    import g2o_amd
    text = open(os.path.join(ROOT, "include", "g2o_hip.h")).read()

    def define(name):
        return int(re.search(rf"#define {name} (\d+)u?\b", text).group(1))

    assert g2o_amd.E_SIM3_PROJECT == synth.E_SIM3_PROJECT == define("G2OHIP_E_SIM3_PROJECT_XYZ") == 28
    assert g2o_amd.E_SIM3_PROJECT_INVERSE == synth.E_SIM3_PROJECT_INVERSE == define("G2OHIP_E_SIM3_PROJECT_INVERSE_XYZ") == 29
    assert g2o_amd.LOAD_SIM3_PROJECT == define("G2OHIP_LOAD_SIM3_PROJECT") == 256
    assert g2o_amd.SIM3_PROJECT_TAGS == P.TAGS
    for t in P.TYPES:
        assert synth.MEAS_DIM[t] == 2 and synth.ERR_DIM[t] == 2 and t not in synth.PARAM_DIM
        assert t < g2o_amd.E_HOSTJ(1)
    assert "g2ohip_set_sim3_cameras" in g2o_amd.EXPORTS and "g2ohip_set_sim3_cameras" in text


def test_g2o_text_round_trip():
    """EDGE_PROJECT_SIM3_XYZ:EXPMAP / EDGE_PROJECT_INVERSE_SIM3_XYZ:EXPMAP v0 v1 u v i00 i01 i11
    (types_seven_dof_expmap.cpp:146-203); reading the lines back gives the edges."""
    prob, cams, _ = P.optimize_sim3_case()
    text = P.g2o_text(prob, cams)
    assert text.count("VERTEX_XYZ ") == 48 and text.count("FIX ") == 48 and text.count("VERTEX_SIM3:EXPMAP ") == 1
    sim3 = next(l for l in text.splitlines() if l.startswith("VERTEX_SIM3")).split()
    assert len(sim3) == 13 and [float(x) for x in sim3[-4:]] == list(P.CAM1)
    back = P.parse_edge_lines(text)
    for es in prob.edges:
        v0, v1, meas, info = back[es.etype]
        assert np.array_equal(v0, es.v0) and np.array_equal(v1, es.v1)
        assert np.array_equal(meas, es.meas) and np.array_equal(np.triu(info), np.triu(es.info))
        assert text.count(P.TAGS[es.etype] + " ") == 24
    line = P.edge_line(P.E_FWD, 3, 48, [1.5, -2.0], [[2.0, 0.5], [0.5, 3.0]])
    assert line == "EDGE_PROJECT_SIM3_XYZ:EXPMAP 3 48 1.5 -2.0 2.0 0.5 3.0"
