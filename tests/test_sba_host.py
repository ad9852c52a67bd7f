"""CPU checks behind tests/test_gpu_sba.py: the numpy reference of the sba types (tests/sba_ref.py) against central
differences through its oplus in extended precision, the oplus itself, the float64 floor of chi2 for every case the GPU
tests compare at 1e-12, the structure-only cases' decisions in float64 against extended precision, and the Python
constants against the header."""
import os
import re

import numpy as np
import pytest

import sba_ref
import structure_only_ref
from g2o_amd import synth
from sba_ref import KINDS, MONO, STEREO

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_cam(rng, near_zero_w=False):
    q = rng.standard_normal(4)
    if near_zero_w:
        q[3] = 1e-9 * rng.standard_normal()
    cam = np.concatenate([rng.standard_normal(3), q, [500.0 + 50 * rng.random(), 480.0 + 50 * rng.random(), 320.0, 240.0,
                                                      0.1 + 0.1 * rng.random()]])
    return sba_ref.normalized(cam)


def _point_in_front(rng, cam):
    pc = np.array([rng.random() - 0.5, rng.random() - 0.5, 3.0 + 2 * rng.random()])
    return cam[:3] + sba_ref._R(cam[None, 3:7])[0] @ pc


@pytest.mark.parametrize("near_zero_w", [False, True])
@pytest.mark.parametrize("etype", KINDS)
def test_jacobians_against_central_differences(etype, near_zero_w):
    """The analytic Jacobians are exact first derivatives under the oplus: central differences in longdouble with
    h = 1e-7 leave O(h^2) ~ 1e-14 relative."""
    rng = np.random.default_rng(11 + etype + near_zero_w)
    worst = 0.0
    for _ in range(20):
        cam = _random_cam(rng, near_zero_w)
        pt = _point_in_front(rng, cam)
        z = np.zeros(synth.ERR_DIM[etype])
        Ji, Jj = sba_ref.jacobians(etype, pt, cam, LD)
        h = LD(1e-7)
        num = np.zeros((len(z), 9), LD)
        for k in range(9):
            d = np.zeros(9, LD)
            d[k] = h
            ep = sba_ref.error(etype, np.asarray(pt, LD) + d[:3], sba_ref.oplus(cam, d[3:], LD), z, LD)
            em = sba_ref.error(etype, np.asarray(pt, LD) - d[:3], sba_ref.oplus(cam, -d[3:], LD), z, LD)
            num[:, k] = (ep - em) / (2 * h)
        ana = np.concatenate([Ji, Jj], 1)
        worst = max(worst, float(np.max(np.abs(ana - num)) / np.max(np.abs(num))))
    print(f"type {etype} near_zero_w={near_zero_w}: analytic vs central differences {worst:.2e}")
    assert worst <= 1e-9


def test_oplus():
    rng = np.random.default_rng(5)
    cam = _random_cam(rng)
    same = sba_ref.oplus(cam, np.zeros(6))
    assert np.array_equal(same[:3], cam[:3]) and np.allclose(same[3:7], cam[3:7], rtol=0, atol=1e-16)
    assert np.array_equal(same[7:], cam[7:])
    u = np.array([0.1, -0.2, 0.3, 0.5, -0.6, 0.3])  # |v|^2 = 0.7
    moved = sba_ref.oplus(cam, u)
    assert abs(np.linalg.norm(moved[3:7]) - 1) <= 4e-16 and np.allclose(moved[:3], cam[:3] + u[:3])
    # the post-multiplied rotation: R' = R R(qr)
    qr = np.concatenate([u[3:], [np.sqrt(1 - u[3:] @ u[3:])]])
    assert np.allclose(sba_ref._R(moved[None, 3:7])[0], sba_ref._R(cam[None, 3:7])[0] @ sba_ref._R(qr[None])[0], atol=1e-14)
    bad = sba_ref.oplus(cam, np.array([0.1, 0.2, 0.3, 0.8, 0.6, 0.3]))  # |v|^2 = 1.09
    assert np.all(np.isnan(bad[3:7])) and np.allclose(bad[:3], cam[:3] + [0.1, 0.2, 0.3]) and np.array_equal(bad[7:], cam[7:])


def chi2_cases():
    """Every problem whose chi2 the GPU tests compare with sba_ref at the project's 1e-12."""
    out = []
    for et in KINDS:
        out.append((f"one_edge {et}", sba_ref.one_edge(et)))
        for ne in (1, 63, 64, 65, 257):
            out.append((f"edge_case {et} ne={ne}", sba_ref.edge_case(et, ne)))
    return out


def test_chi2_float64_floor():
    """float64 against longdouble on the sba edges of every case: the floor stays under 1e-13, so the GPU tests compare
    at the project's 1e-12 relative."""
    worst = 0.0
    for name, prob in chi2_cases():
        g = sba_ref.Graph(prob)
        c64, c80 = g.chi2_in(np.float64), g.chi2_in(LD)
        rel = float(abs(LD(c64) - c80) / c80)
        print(f"{name}: chi2 {float(c80):.6g} float64 floor {rel:.2e}")
        worst = max(worst, rel)
    assert worst <= 1e-13, worst


def test_edge_chi2_float64_floor():
    """Per edge, on the trajectory graphs whose g2ohip_edge_chi2 the GPU test compares at 1e-12: the float64 floor of
    e^T Omega e of a single edge stays under 1e-13 as well (errors of a pixel or more on image coordinates of a few
    hundred)."""
    for stereo in (False, True):
        prob = synth.sba(12, 300, obs_per_point=4, stereo=stereo)
        g = sba_ref.Graph(prob)
        et = STEREO if stereo else MONO
        c64, c80 = g.edge_chi2(et), g.edge_chi2(et, dtype=LD)
        rel = float(np.max(np.abs(c64.astype(LD) - c80) / c80))
        print(f"sba(12, 300) stereo={stereo}: per-edge chi2 floor {rel:.2e}, smallest chi2 {float(np.min(c80)):.3g}")
        assert rel <= 1e-13, rel


STRUCTURE_CASES =[(et, prior) for et in KINDS for prior in (False, True)]


def _calc_in(prob, dtype, iters=10):
    """structure_only_ref's calc with the sba edges evaluated in dtype (the decisions see float64 or longdouble
    errors)."""
    ev = sba_ref._edge_eval

    def edge_eval(ed, p, jac=True):
        if ed.etype in KINDS:
            e = sba_ref.error(ed.etype, p, ed.other, ed.meas, dtype).astype(np.float64)
            return e, (sba_ref.jacobians(ed.etype, p, ed.other, dtype)[0].astype(np.float64) if jac else None)
        return ev.base(ed, p, jac)

    structure_only_ref.edge_eval = edge_eval
    try:
        return structure_only_ref.Structure(prob).calc(iters)
    finally:
        structure_only_ref.edge_eval = ev.base


@pytest.mark.parametrize("etype,prior", STRUCTURE_CASES)
def test_structure_only_counts_clear_of_thresholds(etype, prior):
    """The five counts are the same with the edges evaluated in float64 and in longdouble: no decision of these cases
    sits on a threshold."""
    prob = sba_ref.tracks_problem(etype, prior=prior)
    c64 = structure_only_ref.counts(_calc_in(prob, np.float64)[1])
    c80 = structure_only_ref.counts(_calc_in(prob, LD)[1])
    print(f"type {etype} prior={prior}: {c64}")
    assert c64 == c80 and c64["accepted"] > 0


def test_python_constants_equal_the_header():
    import g2o_amd
    text = open(os.path.join(ROOT, "include", "g2o_hip.h")).read()

    def define(name):
        return int(re.search(rf"#define {name} (\d+)u?\b", text).group(1))

    assert g2o_amd.V_CAM == synth.V_CAM == define("G2OHIP_V_CAM") == 6
    assert g2o_amd.E_PROJECT_P2MC == synth.E_PROJECT_P2MC == define("G2OHIP_E_PROJECT_P2MC") == 11
    assert g2o_amd.E_PROJECT_P2SC == synth.E_PROJECT_P2SC == define("G2OHIP_E_PROJECT_P2SC") == 12
    assert g2o_amd.LOAD_SBA == define("G2OHIP_LOAD_SBA") == 8
    assert synth.EST_DIM[synth.V_CAM] == 12 and synth.ERR_DIM[MONO] == 2 and synth.ERR_DIM[STEREO] == 3


def test_synth_sba_is_the_ba_scene():
    """synth.sba holds ba()'s scene: the camera-to-world estimate is the inverse of ba()'s, and the monocular error is
    minus the expmap edge's."""
    import stereo_ref
    ba, sb = synth.ba(6, 40, 3, 6), synth.sba(6, 40, 3, 6)
    assert np.array_equal(ba.vertices[1].est, sb.vertices[1].est) and list(sb.vertices[0].fixed) == [1, 1, 0, 0, 0, 0]
    eb, es = ba.edges[0], sb.edges[0]
    cam_b, cam_s = ba.vertices[0].est[eb.v1], sb.vertices[0].est[es.v1]
    pts = ba.vertices[1].est[eb.v0 - 6]
    K = np.concatenate([eb.params, np.zeros((len(eb.v0), 1))], 1)
    e_b = stereo_ref.edge_error(cam_b, pts, np.concatenate([eb.meas, np.zeros((len(eb.v0), 1))], 1), K)[:, :2]
    e_s = sba_ref.batch(MONO, pts, cam_s, es.meas, jac=False)
    assert np.allclose(e_s, -e_b, rtol=0, atol=1e-9)
    st = synth.sba(6, 40, 3, 6, stereo=True)
    assert list(st.vertices[0].fixed) == [1, 0, 0, 0, 0, 0] and st.edges[0].meas.shape[1] == 3
    tw = synth.sba_twin(st)
    assert tw.edges[0].etype == 35 and np.array_equal(tw.edges[0].v0, st.edges[0].v0)
