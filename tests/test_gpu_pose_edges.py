"""The pose-graph families the project started with, pinned at their branch inputs: EdgeSE3 (k_linearize<FamilySE3>),
EdgeSE3Prior (FamilyUnarySE3), EdgeSE2 and EdgeSE2PointXY on the device against tests/pose_edges_ref.py.

The inputs are pose_edges_ref's constructed cases: an error rotation on each of R_to_quat's / dq_dR's four branches with
either sign of q_w before the final flip ('tr+', 'x+', 'x-', 'y+', 'y-', 'z+', 'z-'), a pair at trace = +-1e-3, a
measurement quaternion entered with w < 0 and norm 1.3, SE2 angles at -pi, just under pi and turns away with error
angles that wrap either way. tests/test_pose_edges_host.py proves the reference on the same cases (its Jacobians against
longdouble differences, its float64 floors of ~1e-15, the CPU oracle against it).

Tolerances are the project's single-edge ones (tests/test_gpu_slam3d.py, tests/test_gpu_unary.py): chi2 1e-12 relative,
stage level 1e-9 on b, bschur and x and 1e-11 on Hschur.
"""
import numpy as np
import pytest

import pose_edges_ref as R
from g2o_amd import synth

pytestmark = pytest.mark.gpu

LAM = 1e-3
SE3_CASES = R.se3_branch_cases()
PRIOR_CASES = R.prior_branch_cases()
SE2_CASES = R.se2_wrap_cases()
SE2XY_CASES = R.se2xy_wrap_cases()
_CACHE = {}


def _stage_against(tag, s, r):
    schur = s["nl"] > 0
    assert s["ok"] == 1 and (s["n"], s["np"]) == (r["n"], r["np"]), (tag, s["n"], s["np"], r["n"], r["np"])
    for k in ("b", "x") + (("bschur",) if schur else ()):
        err = np.linalg.norm(s[k] - r[k]) / np.linalg.norm(r[k])
        print(f"{tag} {k}: {err:.2e}")
        assert err <= 1e-9, (tag, k, err)
    err = np.linalg.norm(s["Hschur"] - r["Hschur"]) / np.linalg.norm(r["Hschur"])
    print(f"{tag} Hschur: {err:.2e}")
    assert err <= 1e-11, (tag, err)


def _pin(mod, prob, etype, tag):
    """chi2 to 1e-12, Huber's linear branch, and the stage at lambda = 1e-3 against the numpy dense system."""
    ref = float(R.Graph(prob).chi2(R.LD))
    opt = mod.SparseOptimizer(0).add_problem(prob)
    chi = opt.chi2()
    print(f"{tag}: chi2 device {chi:.17g} numpy {ref:.17g} rel {abs(chi - ref) / ref:.2e}")
    assert ref > 0 and abs(chi - ref) <= 1e-12 * ref, tag
    _stage_against(tag, opt.stage(LAM), R.numpy_stage(prob, LAM))
    delta = 0.5 * np.sqrt(ref)  # sqrt(e2) > delta: Huber's linear branch, chi2 = rho
    opt.set_robust_kernel(etype, "Huber", delta)
    rho = 2 * np.sqrt(ref) * delta - delta * delta
    assert abs(opt.chi2() - rho) <= 1e-12 * rho, tag


# ---------------------------------------------------------------- 1: single-edge pins per branch label
@pytest.mark.parametrize("k", range(len(SE3_CASES)), ids=[c[0] for c in SE3_CASES])
def test_se3_single_edge(g2o_amd_mod, k):
    _pin(g2o_amd_mod, R.se3_problem(SE3_CASES[k], k), synth.E_SE3_QUAT, f"EdgeSE3 {SE3_CASES[k][0]}")


@pytest.mark.parametrize("k", range(len(PRIOR_CASES)), ids=[c[0] for c in PRIOR_CASES])
def test_se3_prior_single_edge(g2o_amd_mod, k):
    _pin(g2o_amd_mod, R.prior_problem(PRIOR_CASES[k], k), synth.E_SE3_PRIOR, f"EdgeSE3Prior {PRIOR_CASES[k][0]}")


@pytest.mark.parametrize("k", range(len(SE2_CASES)), ids=[f"{k}-{c[0]}" for k, c in enumerate(SE2_CASES)])
def test_se2_single_edge(g2o_amd_mod, k):
    _pin(g2o_amd_mod, R.se2_problem(SE2_CASES[k], k), synth.E_SE2, f"EdgeSE2 {k} {SE2_CASES[k][0]}")


@pytest.mark.parametrize("k", range(len(SE2XY_CASES)), ids=[f"{k}-{c[0]}" for k, c in enumerate(SE2XY_CASES)])
def test_se2xy_single_edge(g2o_amd_mod, k):
    _pin(g2o_amd_mod, R.se2xy_problem(SE2XY_CASES[k], k), synth.E_SE2_XY, f"EdgeSE2PointXY {k} {SE2XY_CASES[k][0]}")


def test_census():
    """The cases the pins ran on cover what they claim (tests/test_pose_edges_host.py::test_branch_census proves the
    labels against the longdouble error rotations)."""
    assert [c[0] for c in SE3_CASES][:7] == list(R.LABELS) == [c[0] for c in PRIOR_CASES][:7]
    assert {c[0] for c in SE2_CASES} == {"up", "down"} and {c[0] for c in SE2XY_CASES} == {"edge", "outside"}


# ---------------------------------------------------------------- 2: all branch cases in one graph
NES = [1, 63, 64, 65, 257]


@pytest.mark.parametrize("ne", NES)
def test_se3_chain(g2o_amd_mod, ne):
    """The seven labels side by side in the waves of k_linearize<FamilySE3>: a partial wave, a full one, one edge more,
    one edge past a 256-thread block."""
    prob, labels = R.se3_chain(ne)
    assert ne < 7 or set(labels) == set(R.LABELS)
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    _stage_against(f"se3 chain ne={ne}", opt.stage(LAM), R.numpy_stage(prob, LAM))
    ref = float(R.Graph(prob).chi2(R.LD))
    assert abs(opt.chi2() - ref) <= 1e-12 * ref


@pytest.mark.parametrize("ne", NES)
def test_se2_chain(g2o_amd_mod, ne):
    """FamilySE2 (3/3/3 staging strides) with unwrapped vertex angles and error angles that wrap up and down."""
    prob, labels = R.se2_chain(ne)
    assert ne < 2 or set(labels) == {"up", "down"}
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    _stage_against(f"se2 chain ne={ne}", opt.stage(LAM), R.numpy_stage(prob, LAM))
    ref = float(R.Graph(prob).chi2(R.LD))
    assert abs(opt.chi2() - ref) <= 1e-12 * ref


@pytest.mark.parametrize("ne", NES)
def test_se2xy_fan(g2o_amd_mod, ne):
    """FamilySE2XY (2/3/2 strides, the 3/2 Schur path) with pose angles on and outside the ends of [-pi, pi)."""
    prob = R.se2xy_fan(ne)
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    s = opt.stage(LAM)
    assert s["nl"] == 2 * len(prob.vertices[1].ids)
    _stage_against(f"se2xy fan ne={ne}", s, R.numpy_stage(prob, LAM))
    ref = float(R.Graph(prob).chi2(R.LD))
    assert abs(opt.chi2() - ref) <= 1e-12 * ref


# ---------------------------------------------------------------- 3: the measurement entered three ways
def _g2o_text(prob):
    """The problem as a .g2o file written by hand: repr() round-trips every double."""
    vs, es = prob.vertices[0], prob.edges[0]
    lines = [f"VERTEX_SE3:QUAT {i} " + " ".join(repr(float(v)) for v in e) for i, e in zip(vs.ids, vs.est)]
    for k in range(len(es.v0)):
        up = [repr(float(es.info[k][r, c])) for r in range(6) for c in range(r, 6)]
        lines.append(f"EDGE_SE3:QUAT {es.v0[k]} {es.v1[k]} " + " ".join(repr(float(v)) for v in es.meas[k]) + " " +
                     " ".join(up))
    return "\n".join(lines) + "\n"


def test_measurement_three_ways(g2o_amd_mod, tmp_path):
    """The 'wneg' case through add_edges, through a file, and as the normalized w > 0 quaternion: the loader and
    add_edges normalize the quaternion, so all three hand the same Z^-1 to the device and b is bit-identical."""
    case = SE3_CASES[-1]
    assert case[0] == "wneg"
    raw, qn = R.wneg_quat()
    assert np.array_equal(case[3][3:], raw) and raw[3] < 0 < qn[3] and abs(np.linalg.norm(raw) - 1.3) < 1e-12
    prob = R.se3_problem(case, 9)
    a = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    path = tmp_path / "wneg.g2o"
    path.write_text(_g2o_text(prob))
    b = g2o_amd_mod.SparseOptimizer(0)
    b.load(str(path))
    assert (b.num_vertices(), b.num_edges()) == (2, 1)
    b.set_estimates(synth.V_SE3_QUAT, prob.vertices[0].est)  # the same vertex states, whatever the reader does to them
    es = prob.edges[0]
    norm = synth.EdgeSet(es.etype, es.v0, es.v1, np.concatenate([es.meas[:, :3], qn[None]], 1), es.info)
    c = g2o_amd_mod.SparseOptimizer(0).add_problem(synth.Problem("n", prob.vertices, [norm], 6, 0))
    sa, sb, sc = a.stage(LAM), b.stage(LAM), c.stage(LAM)
    assert np.linalg.norm(sa["b"]) > 0
    assert np.array_equal(sa["b"], sb["b"]) and np.array_equal(sa["b"], sc["b"])
    assert a.chi2() == b.chi2() == c.chi2()
