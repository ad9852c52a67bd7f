"""CPU checks behind tests/test_gpu_offset.py: the numpy restatement of EdgeSE3Offset, EdgeSE2Offset and
EdgeSE2PointXYBearing (tests/offset_ref.py) against central differences through the vertices' oplus in extended precision
(the dq_dR branch targets and margins of pose_edges_ref, the theta wraps, the atan2 cut), the identity-offset cases against
pose_edges_ref's EdgeSE3 / EdgeSE2, the float64 floor of chi2 on every case the GPU tests compare at 1e-12, the
structure-only decisions in float64 against extended precision, the generators, and the Python constants against the
header."""
import os
import re

import numpy as np
import pytest

import offset_ref as O
import pose_edges_ref as R
import structure_only_ref
from g2o_amd import synth
from offset_ref import BEAR, KINDS, OFFSETS, SE2O, SE3O
from test_pose_edges_host import _add, _numeric, _se2_plus, _se3_plus, _unit_pose, _worst

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JTOL = 1e-9  # central differences with h = 1e-6 in longdouble: O(h^2) of third derivatives of order one


def test_se3_offset_jacobians_vs_numeric():
    labels = []
    for label, xi, xj, z, P in O.se3_branch_cases():
        xi, xj = _unit_pose(xi), _unit_pose(xj)
        e, Ji, Jj = O.se3_offset_edge(xi, xj, z, P, LD)
        Re = R.rot(np.concatenate([e[0, 3:], [np.sqrt(1 - e[0, 3:] @ e[0, 3:])]]), LD)[0]
        labels.append(R.branch_of(Re))
        Ni, Nj = _numeric(lambda a, b: O.se3_offset_edge(a, b, z, P, LD, jac=False)[0], (xi, xj), (_se3_plus,) * 2, (6, 6))
        w = _worst([(Ji[0], Ni), (Jj[0], Nj)])
        print(f"EdgeSE3Offset {label} (branch {labels[-1]}): {w:.2e}")
        assert w <= JTOL, (label, w)
    # the error rotations are the targets: every dq_dR branch is met (the four branches, each sign of q_w)
    assert set(R.LABELS) <= set(labels), labels
    # 'wneg': the measurement quaternion has w < 0 and is not of unit length
    z = O.se3_branch_cases()[-1][3]
    assert z[6] < 0 and abs(np.linalg.norm(z[3:]) - 1.3) < 1e-12


def test_se2_offset_jacobians_vs_numeric():
    seen = set()
    for label, xi, xj, z, P in O.se2_wrap_cases():
        seen.add(label)
        xi, xj = np.asarray(xi, LD), np.asarray(xj, LD)
        _, Ji, Jj = O.se2_offset_edge(xi, xj, z, P, LD)
        Ni, Nj = _numeric(lambda a, b: O.se2_offset_edge(a, b, z, P, LD, jac=False)[0], (xi, xj), (_se2_plus,) * 2, (3, 3))
        w = _worst([(Ji[0], Ni), (Jj[0], Nj)])
        print(f"EdgeSE2Offset {label}: {w:.2e}")
        assert w <= JTOL, (label, w)
    assert {"up", "down"} <= seen, seen


def test_bearing_jacobians_vs_numeric():
    for label, xi, l, z in O.bearing_cut_cases():
        xi, l = np.asarray(xi, LD), np.asarray(l, LD)
        e, Ji, Jj = O.bearing_edge(xi, l, z, LD)
        assert abs(float(e[0, 0])) < 1.0  # wrapped: no case sits at +-pi
        Ni, Nj = _numeric(lambda a, b: O.bearing_edge(a, b, z, LD, jac=False)[0], (xi, l), (_se2_plus, _add), (3, 2))
        w = _worst([(Ji[0], Ni), (Jj[0], Nj)])
        print(f"EdgeSE2PointXYBearing {label}: {w:.2e}")
        assert w <= JTOL, (label, w)


def test_random_cases_vs_numeric():
    """Random inputs beside the constructed ones; bearing with |d| >= 1."""
    rng = np.random.default_rng(77)
    worst = 0.0
    for _ in range(10):
        xi, xj = (_unit_pose(R.pose_of(*O._rand_pose(rng))) for _ in range(2))
        z, P = R.pose_of(*O._rand_pose(rng)), O._rand_offsets7(rng, 2).ravel()
        _, Ji, Jj = O.se3_offset_edge(xi, xj, z, P, LD)
        q = O.se3_offset_edge(xi, xj, z, P, LD, jac=False)[0, 3:]
        if 1 - q @ q < 0.02 ** 2:  # q_w under pose_edges_ref's margin
            continue
        Ni, Nj = _numeric(lambda a, b: O.se3_offset_edge(a, b, z, P, LD, jac=False)[0], (xi, xj), (_se3_plus,) * 2, (6, 6))
        worst = max(worst, _worst([(Ji[0], Ni), (Jj[0], Nj)]))
        a, b = (np.asarray(rng.uniform(-3, 3, 3), LD) for _ in range(2))
        z2, P2 = rng.uniform(-1, 1, 3), rng.uniform(-1.5, 1.5, 6)
        if abs(float(O.se2_offset_edge(a, b, z2, P2, LD, jac=False)[0, 2])) > np.pi - 0.01:
            continue
        _, Ji, Jj = O.se2_offset_edge(a, b, z2, P2, LD)
        Ni, Nj = _numeric(lambda u, v: O.se2_offset_edge(u, v, z2, P2, LD, jac=False)[0], (a, b), (_se2_plus,) * 2, (3, 3))
        worst = max(worst, _worst([(Ji[0], Ni), (Jj[0], Nj)]))
        d = rng.uniform(1.0, 3.0) * np.array([np.cos(t := rng.uniform(-3.0, 3.0)), np.sin(t)])
        l = np.asarray(a[:2] + R.rot2(np.float64(a[2])) @ d, LD)
        zb = np.array([t + rng.uniform(-0.5, 0.5)])
        _, Ji, Jj = O.bearing_edge(a, l, zb, LD)
        Ni, Nj = _numeric(lambda u, v: O.bearing_edge(u, v, zb, LD, jac=False)[0], (a, l), (_se2_plus, _add), (3, 2))
        worst = max(worst, _worst([(Ji[0], Ni), (Jj[0], Nj)]))
    print(f"random cases: {worst:.2e}")
    assert worst <= JTOL


def test_identity_offsets_equal_the_plain_edges():
    """EdgeSE3Offset / EdgeSE2Offset with identity offsets are EdgeSE3 / EdgeSE2: to rounding (64 eps of the largest
    entry; the two restatements order their products differently)."""
    tol = 64 * float(np.finfo(np.float64).eps)
    for _, xi, xj, z in R.se3_branch_cases():
        for P in (None, O.IDENT[SE3O]):
            a, b = O.se3_offset_edge(xi, xj, z, P), R.se3_edge(xi, xj, z)
            for u, v in zip(a, b):
                assert np.max(np.abs(u - v)) <= tol * max(1.0, np.max(np.abs(v)))
    for _, xi, xj, z in R.se2_wrap_cases():
        for P in (None, O.IDENT[SE2O]):
            a, b = O.se2_offset_edge(xi, xj, z, P), R.se2_edge(xi, xj, z)
            for u, v in zip(a, b):
                assert np.max(np.abs(u - v)) <= tol * max(1.0, np.max(np.abs(v)))


def chi2_cases():
    """Every problem whose chi2 the GPU tests compare with offset_ref at the project's 1e-12."""
    out = []
    for et in KINDS:
        out.append((f"one_edge {et}", O.one_edge(et)))
        for ne in (1, 63, 64, 65, 257):
            for uniform in ((False, True) if et in OFFSETS else (False,)):
                out.append((f"edge_case {et} ne={ne} uniform={uniform}", O.edge_case(et, ne, uniform)))
    for c in O.se3_branch_cases():
        out.append((f"se3 branch {c[0]}", O.one_edge(SE3O, c)))
    for c in O.se2_wrap_cases():
        out.append((f"se2 wrap {c[0]}", O.one_edge(SE2O, c)))
    for c in O.bearing_cut_cases():
        out.append((f"bearing {c[0]}", O.one_edge(BEAR, c)))
    out.append(("se3_offset_graph", synth.se3_offset_graph()))
    out.append(("se2_offset_graph", synth.se2_offset_graph()))
    out.append(("bearing_scene", synth.bearing_scene()))
    return out


def test_chi2_float64_floor():
    """float64 against longdouble on the new edges of every case: the floor stays under 1e-13, so the GPU tests compare
    at the project's 1e-12 relative."""
    worst = 0.0
    for name, prob in chi2_cases():
        g = O.Graph(prob)
        c64, c80 = g.chi2_in(np.float64), g.chi2_in(LD)
        rel = float(abs(LD(c64) - c80) / c80)
        print(f"{name}: chi2 {float(c80):.6g} float64 floor {rel:.2e}")
        worst = max(worst, rel)
    print(f"worst float64 floor {worst:.2e}")
    assert worst <= 1e-13, worst


def test_edge_chi2_float64_floor():
    """Per edge, on the graphs whose g2ohip_edge_chi2 the GPU test compares at 1e-12."""
    for et, prob in ((SE3O, synth.se3_offset_graph()), (SE2O, synth.se2_offset_graph()), (BEAR, O.per_edge_scene())):
        g = O.Graph(prob)
        c64, c80 = g.edge_chi2(et), g.edge_chi2(et, dtype=LD)
        rel = float(np.max(np.abs(c64.astype(LD) - c80) / c80))
        print(f"type {et}: per-edge chi2 floor {rel:.2e}, smallest chi2 {float(np.min(c80)):.3g}")
        assert rel <= 1e-13, rel


@pytest.mark.parametrize("prior", [False, True])
def test_structure_only_counts_clear_of_thresholds(prior):
    """The five counts are the same with the bearing edges evaluated in float64 and in longdouble: no decision of the
    tracks problem sits on a threshold."""
    prob = O.tracks_problem(prior=prior)
    s = O.Structure(prob)
    c64 = structure_only_ref.counts(s.calc(10)[1])
    c80 = structure_only_ref.counts(s.calc(10, dtype=LD)[1])
    print(f"prior={prior}: {c64}")
    assert c64 == c80 and c64["accepted"] > 0
    assert structure_only_ref.edge_eval is O._edge_eval.base  # the edge table is restored


def test_python_constants_equal_the_header():
    import g2o_amd
    text = open(os.path.join(ROOT, "include", "g2o_hip.h")).read()

    def define(name):
        return int(re.search(rf"#define {name} (\d+)u?\b", text).group(1))

    assert g2o_amd.E_SE3_OFFSET == synth.E_SE3_OFFSET == define("G2OHIP_E_SE3_OFFSET") == 13
    assert g2o_amd.E_SE2_OFFSET == synth.E_SE2_OFFSET == define("G2OHIP_E_SE2_OFFSET") == 14
    assert g2o_amd.E_SE2_XY_BEARING == synth.E_SE2_XY_BEARING == define("G2OHIP_E_SE2_XY_BEARING") == 15
    assert g2o_amd.LOAD_OFFSET == define("G2OHIP_LOAD_OFFSET") == 16
    assert g2o_amd.EDGE_TAGS == O.TAGS
    assert [synth.ERR_DIM[t] for t in KINDS] == [6, 3, 1] and [synth.MEAS_DIM[t] for t in KINDS] == [7, 3, 1]
    assert synth.PARAM_DIM[SE3O] == 14 and synth.PARAM_DIM[SE2O] == 6 and BEAR not in synth.PARAM_DIM


def test_synth_generators():
    """Seeded (the same arrays twice), one or two distinct sensor pairs, every landmark of the bearing scene seen from
    at least three poses under different directions, and the true scene close to the measurements."""
    for gen, et, npar in ((synth.se3_offset_graph, SE3O, 14), (synth.se2_offset_graph, SE2O, 6)):
        a, b = gen(), gen()
        assert all(np.array_equal(x.meas, y.meas) and np.array_equal(x.params, y.params) for x, y in zip(a.edges, b.edges))
        assert np.array_equal(a.vertices[0].est, b.vertices[0].est)
        es = a.edges[0]
        assert es.etype == et and es.params.shape == (len(es.v0), npar) and 110 <= len(es.v0) <= 130
        assert len(np.unique(es.params, axis=0)) == 4 and len(np.unique(es.params.reshape(-1, npar // 2), axis=0)) == 2
        one = gen(num_offsets=1).edges[0]
        assert len(np.unique(one.params, axis=0)) == 1
        chi = O.Graph(a).chi2()
        assert chi < 100.0 * len(es.v0) * synth.ERR_DIM[et]  # the perturbed start is near the measurements' scene
        tw = synth.offset_twin(a)
        assert tw.edges[0].etype == O.HOSTJ[et] and tw.edges[0].meas is None
    sc = synth.bearing_scene()
    poses, lms = sc.vertices
    obs = sc.edges[1]
    assert obs.etype == BEAR and obs.meas.shape == (len(obs.v0), 1) and obs.info.shape == (len(obs.v0), 1, 1)
    assert len(poses.ids) == 12 and len(lms.ids) == 30 and np.all(lms.marginalized == 1) and poses.fixed[0] == 1
    for l in lms.ids:
        sel = obs.v1 == l
        assert sel.sum() >= 3 and len(np.unique(obs.v0[sel])) == sel.sum()
        d = lms.est[l - 12] - poses.est[obs.v0[sel], :2]
        assert np.min(np.linalg.norm(d, axis=1)) >= 1.0
        dirs = np.arctan2(d[:, 1], d[:, 0])
        spread = np.max(np.abs(R.wrap(dirs[:, None] - dirs[None, :])))
        assert spread > 0.2, spread  # parallax: the directions to the landmark differ by more than 0.2 rad
