"""SparseOptimizer::update on the device (k_oplus_multi and the five d_oplus_* maps) against tests/pose_edges_ref.py in
longdouble, with caller-supplied increments that LM and dogleg steps never produce: SE3Quat::exp on both sides of its
theta = 1e-5 threshold and at 2.6 rad about every axis (R_to_quat's branches), a product quaternion with w < 0,
VertexSE3 increments with |dq|^2 up to 4 (the identity fallback above 1), SE2 angles landing on -pi, just under pi and
turns away, the re-orthogonalisation on VertexSE3's 1001st call, fixed vertices, push / pop.

Three graphs, because a solver has one pose and one landmark dimension: cameras (V_SE3_EXPMAP) and points (V_XYZ),
VertexSE3 poses, SE2 poses and XY landmarks. Each has one free vertex per case of pose_edges_ref.oplus_cases and one
fixed vertex per type. The place of every vertex in x is found by probing, one entry at a time.

Tolerance per entry: max(8 * OPLUS_FLOOR[type], 64 eps) * max(1, |value|), OPLUS_FLOOR the float64-against-longdouble
floor that tests/test_pose_edges_host.py measures and explains (device sin, cos, sqrt and the compiler's contraction
each move a result by an ulp or two per operation). Measured on an MI355X: V_SE3_EXPMAP 4.6e-13 (the theta = 2e-5
case, equal to the CPU floor; 5.9e-16 at most on the other cases, which are held to 64 eps), V_SE3_QUAT 4.1e-16,
V_SE2 9.5e-17, V_XYZ 2.8e-17, V_XY 4.8e-17.
"""
import numpy as np
import pytest

import pose_edges_ref as R
from g2o_amd import synth

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
LD = R.LD
DIM = {synth.V_SE3_EXPMAP: 6, synth.V_XYZ: 3, synth.V_SE3_QUAT: 6, synth.V_SE2: 3, synth.V_XY: 2}


def _tol(vtype, value=1.0):
    return max(8 * R.OPLUS_FLOOR[vtype], 64 * EPS) * np.maximum(1.0, np.abs(np.asarray(value, np.float64)))


def _with_fixed(vtype, id0, marg=0):
    """The type's cases as free vertices and a copy of the first as a fixed one at the end."""
    labels, est, u = R.oplus_cases(vtype)
    est = np.concatenate([est, est[:1]])
    fx = np.zeros(len(est), np.int32)
    fx[-1] = 1
    return R._vs(vtype, id0 + np.arange(len(est)), est, fx, marg), u


def _graphs():
    rng = np.random.default_rng(4800)
    out = {}
    cams, ucam = _with_fixed(synth.V_SE3_EXPMAP, 0)
    pts, upt = _with_fixed(synth.V_XYZ, 100, marg=1)
    nc, npt = len(cams.ids), len(pts.ids)
    v1 = np.concatenate([cams.ids, cams.ids])  # EdgeSE3ProjectXYZ: vertex 0 the point, vertex 1 the camera
    v0 = np.concatenate([pts.ids[np.arange(nc) % npt], pts.ids[(np.arange(nc) + 1) % npt]])
    ba = R._es(synth.E_SE3_PROJECT_XYZ, v0, v1, rng.uniform(100, 500, (2 * nc, 2)), R._spd(rng, 2, 2 * nc),
               np.broadcast_to([500.0, 480.0, 320.0, 240.0], (2 * nc, 4)).copy())
    out["ba"] = (synth.Problem("oplus_ba", [cams, pts], [ba], 6, 3), {synth.V_SE3_EXPMAP: ucam, synth.V_XYZ: upt})
    poses, upose = _with_fixed(synth.V_SE3_QUAT, 0)
    n = len(poses.ids)
    ident = np.broadcast_to([0, 0, 0, 0, 0, 0, 1.0], (n - 1, 7)).copy()
    out["se3"] = (synth.Problem("oplus_se3", [poses], [R._es(synth.E_SE3_QUAT, poses.ids[:-1], poses.ids[1:], ident,
                                                             R._spd(rng, 6, n - 1))], 6, 0), {synth.V_SE3_QUAT: upose})
    p2, up2 = _with_fixed(synth.V_SE2, 0)
    l2, ul2 = _with_fixed(synth.V_XY, 100, marg=1)
    n2, nl = len(p2.ids), len(l2.ids)
    odo = R._es(synth.E_SE2, p2.ids[:-1], p2.ids[1:], np.zeros((n2 - 1, 3)), R._spd(rng, 3, n2 - 1))
    v1 = np.concatenate([l2.ids[np.arange(n2) % nl], l2.ids[(np.arange(n2) + 1) % nl]])
    obs = R._es(synth.E_SE2_XY, np.concatenate([p2.ids, p2.ids]), v1, np.zeros((2 * n2, 2)), R._spd(rng, 2, 2 * n2))
    out["se2"] = (synth.Problem("oplus_se2", [p2, l2], [odo, obs], 3, 2), {synth.V_SE2: up2, synth.V_XY: ul2})
    return out


GRAPHS = _graphs()


def _open(mod, name):
    prob, u = GRAPHS[name]
    opt = mod.SparseOptimizer(0).add_problem(prob)
    opt.initialize_optimization()
    opt.build_structure()
    return opt, prob, u


def _all(opt, prob):
    return {vs.vtype: opt.estimates(vs.vtype) for vs in prob.vertices}


def _layout(opt, prob):
    """{vertex type: offsets [rows], -1 for a fixed vertex}: entry k of x is set to 1e-3 alone, between push and pop,
    and the one vertex that moves owns it; a vertex's entries must be contiguous and as many as its dimension."""
    n = opt.vector_size()
    base = _all(opt, prob)
    owner = []
    for k in range(n):
        x = np.zeros(n)
        x[k] = 1e-3
        opt.push()
        opt.update(x)
        now = _all(opt, prob)
        opt.pop()
        moved = [(vt, int(r)) for vt in base for r in np.nonzero(np.any(now[vt] != base[vt], axis=1))[0]]
        assert len(moved) == 1, (k, moved)
        owner.append(moved[0])
    after = _all(opt, prob)
    assert all(np.array_equal(after[vt], base[vt]) for vt in base)
    off = {vs.vtype: np.full(len(vs.ids), -1) for vs in prob.vertices}
    for k, (vt, r) in enumerate(owner):
        if off[vt][r] < 0:
            off[vt][r] = k
        assert owner[off[vt][r]:off[vt][r] + DIM[vt]] == [(vt, r)] * DIM[vt] and k < off[vt][r] + DIM[vt], (k, vt, r)
    for vs in prob.vertices:
        assert np.array_equal(off[vs.vtype] < 0, vs.fixed.astype(bool)), (vs.vtype, off[vs.vtype])
    assert sum(DIM[vs.vtype] * int((off[vs.vtype] >= 0).sum()) for vs in prob.vertices) == n
    return off


def _x_of(opt, prob, off, u):
    x = np.zeros(opt.vector_size())
    for vs in prob.vertices:
        for r, o in enumerate(off[vs.vtype]):
            if o >= 0:
                x[o:o + DIM[vs.vtype]] = u[vs.vtype][r]
    return x


def _compare(vtype, labels, before, got, want, u):
    """got / before: the device's estimates of the free vertices after / before the update; want: the reference."""
    for k, label in enumerate(labels):
        if vtype == synth.V_SE3_QUAT:
            Rw, tw = want[0][k], want[1][k]
            dR = np.abs(R.rot(got[k, 3:], LD)[0] - Rw).astype(np.float64).max()
            dt = (np.abs(got[k, :3] - tw) / np.maximum(1, np.abs(tw))).astype(np.float64).max()
            print(f"type {vtype} {label}: R {dR:.2e} t {dt:.2e}")
            assert dR <= _tol(vtype) and dt <= _tol(vtype), (label, dR, dt)
            assert abs(np.linalg.norm(got[k, 3:]) - 1) <= 4 * EPS
            if u[k, 3:] @ u[k, 3:] > 1:  # the identity fallback: the rotation is not touched at all
                assert np.array_equal(got[k, 3:], before[k, 3:]), label
                assert not np.array_equal(got[k, :3], before[k, :3])
        else:
            d = (np.abs(got[k] - want[k]) / np.maximum(1, np.abs(want[k]))).astype(np.float64).max()
            print(f"type {vtype} {label}: {d:.2e}")
            # the expmap's floor belongs to its theta = 2e-5 case alone (tests/test_pose_edges_host.py)
            assert d <= (_tol(vtype) if label == "th=2e-5" else 64 * EPS), (label, d)
            if vtype == synth.V_SE2:
                assert -R.PI <= got[k, 2] < R.PI, label
            if vtype == synth.V_SE3_EXPMAP:
                assert got[k, 6] >= 0 and abs(np.linalg.norm(got[k, 3:]) - 1) <= 4 * EPS, label


def _reference(vtype, est, u):
    if vtype == synth.V_SE3_QUAT:
        return R.oplus_se3quat(R.rot(est[:, 3:], LD, False), est[:, :3], u, LD)[:2]
    return R.oplus(vtype, est, u, LD)


@pytest.mark.parametrize("name", ["ba", "se3", "se2"])
def test_update_against_reference(g2o_amd_mod, name):
    opt, prob, u = _open(g2o_amd_mod, name)
    off = _layout(opt, prob)
    before = _all(opt, prob)
    for vs in prob.vertices:  # what the device holds is what was entered (VertexSE3: the same rotation, q or -q)
        b, e = before[vs.vtype], vs.est
        if vs.vtype == synth.V_SE3_QUAT:
            assert np.abs(R.rot(b[:, 3:]) - R.rot(e[:, 3:])).max() <= 8 * EPS
            b, e = b[:, :3], e[:, :3]
        assert np.abs(b - e).max() <= 4 * EPS * np.abs(e).max()
    x = _x_of(opt, prob, off, u)
    opt.push()
    opt.update(x)
    after = _all(opt, prob)
    for vs in prob.vertices:
        vt = vs.vtype
        labels = R.oplus_cases(vt)[0]
        free = slice(0, len(labels))
        _compare(vt, labels, before[vt][free], after[vt][free], _reference(vt, vs.est[free], u[vt]), u[vt])
        assert np.array_equal(after[vt][-1], before[vt][-1]), f"fixed vertex of type {vt} moved"
        assert not np.array_equal(after[vt][1], before[vt][1])
    opt.pop()
    restored = _all(opt, prob)
    for vt in before:
        assert np.array_equal(restored[vt], before[vt]), f"pop did not restore type {vt}"
    # the same increment again gives the same bits
    opt.update(x)
    again = _all(opt, prob)
    for vt in before:
        assert np.array_equal(again[vt], after[vt])


def test_update_checks_its_argument(g2o_amd_mod):
    opt, prob, u = _open(g2o_amd_mod, "se3")
    with pytest.raises(ValueError):
        opt.update(np.zeros(opt.vector_size() + 1))
    with pytest.raises(g2o_amd_mod.G2OHipError):
        opt.pop()  # nothing pushed


def _quat_trace_form(Rm):
    """toVectorQT of a matrix with positive trace: w = sqrt(1 + tr) / 2, v from the antisymmetric part, normalized. For
    a matrix that is not orthogonal the result depends on the formula, so the device's own (its trace branch) is used."""
    w = np.sqrt(1 + np.trace(Rm)) / 2
    q = np.array([(Rm[2, 1] - Rm[1, 2]) / (4 * w), (Rm[0, 2] - Rm[2, 0]) / (4 * w), (Rm[1, 0] - Rm[0, 1]) / (4 * w), w])
    return q / np.linalg.norm(q)


def test_reorthogonalisation_on_call_1001(g2o_amd_mod):
    """Three VertexSE3, one fixed. The two free ones start from quaternions of norm 1.002, which fromVectorQT turns
    into matrices with |R^T R - I| ~ 3e-4 (setEstimate does not normalize); products with rotations keep that drift, so
    it is large enough to see through the quaternion that estimates() returns. 1001 updates with one small u: after
    call 1000 the device still carries the drift, after call 1001 it has taken the reference's one step
    R - R (R^T R - I) / 2, and calls 1002 and 1003 leave it alone (the counter restarted). Reference: the same steps in
    float64 with the same rule; tolerance: the oplus tolerance times the number of calls."""
    rng = np.random.default_rng(4900)
    q = np.array([[0.1, -0.05, 0.08, 0.99], [-0.07, 0.1, 0.05, 0.99], [0, 0, 0, 1.0]])
    q[:2] *= 1.002 / np.linalg.norm(q[:2], axis=1, keepdims=True)
    est = np.concatenate([rng.uniform(-1, 1, (3, 3)), q], 1)
    vs = R._vs(synth.V_SE3_QUAT, [0, 1, 2], est, [0, 0, 1])
    ident = np.broadcast_to([0, 0, 0, 0, 0, 0, 1.0], (2, 7)).copy()
    prob = synth.Problem("reorth", [vs], [R._es(synth.E_SE3_QUAT, [0, 1], [1, 2], ident, R._spd(rng, 6, 2))], 6, 0)
    u = np.array([[1e-3, -2e-3, 1.5e-3, 3e-4, -2e-4, 3.5e-4], [-1e-3, 1e-3, 2e-3, -2e-4, 4e-4, 1e-4]])

    def fresh():
        o = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
        o.initialize_optimization()
        o.build_structure()
        assert o.vector_size() == 12
        return o

    # the probe's own updates count as oplus calls (pop does not take them back, in the reference neither): the
    # layout is read from a graph of its own, the 1001 calls go to a fresh one
    off = _layout(fresh(), prob)[synth.V_SE3_QUAT]
    opt = fresh()
    x = np.zeros(12)
    for r in range(2):
        x[off[r]:off[r] + 6] = u[r]

    def drift(Rm):
        return max(np.abs(M.T @ M - np.eye(3)).max() for M in Rm)

    def check(call, Rm, tm):
        got = opt.estimates(synth.V_SE3_QUAT)
        want = np.array([np.concatenate([tm[r], _quat_trace_form(Rm[r])]) for r in range(2)])
        d = np.abs(got[:2] - want).max()
        print(f"call {call}: device against reference {d:.2e}, reference drift {drift(Rm):.2e}")
        assert d <= _tol(synth.V_SE3_QUAT) * call, (call, d)
        assert np.array_equal(got[2], est[2])
        return got

    Rm, tm, calls = R.rot(est[:2, 3:], np.float64, False), est[:2, :3].copy(), 0
    Rn, tn = Rm.copy(), tm.copy()  # the same steps without the rule
    d0 = drift(Rm)
    assert d0 > 1e-4 and all(np.trace(M) > 1 for M in Rm)
    seen = {}
    for call in range(1, 1004):
        opt.update(x)
        Rm, tm, calls = R.oplus_se3quat(Rm, tm, u, calls=calls)
        if call <= 1001:
            Rn, tn, _ = R.oplus_se3quat(Rn, tn, u)
        if call in (1000, 1001, 1003):
            seen[call] = (check(call, Rm, tm), drift(Rm))
        if call == 1001:
            # the rule is visible: the reference without it is far outside the tolerance, in the quaternion as well
            gap = max(np.abs(_quat_trace_form(Rn[r]) - _quat_trace_form(Rm[r])).max() for r in range(2))
            assert gap > 100 * _tol(synth.V_SE3_QUAT) * call, gap
    assert seen[1000][1] > 0.5 * d0 and seen[1001][1] < 2 * d0 * d0 and seen[1003][1] > 0.5 * seen[1001][1]
    assert all(np.trace(M) > 0 for M in Rm)
