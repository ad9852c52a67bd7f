"""The offset and bearing edges on the device (G2OHIP_E_SE3_OFFSET, G2OHIP_E_SE2_OFFSET, G2OHIP_E_SE2_XY_BEARING): the
three families through k_linearize / k_error and the slot reduction, both states of the shared parameter and information
records, the dq_dR branches, theta wraps and the atan2 cut, the 3/2 Schur path, structure-only, levels and
classification, marginals, landmark shards, .g2o files and the refusals.

Two references: tests/offset_ref.py (plain numpy) for chi2, the stage level and structure-only, and the same graph with
each new edge set entered as G2OHIP_E_HOSTJ(6) / (3) / (1) edges whose host callback returns offset_ref's
[e | Ji | Jj] records (the twin) for the trajectories. The twin's stage is pinned against numpy before it serves.

Tolerances are the project's own: chi2 against numpy 1e-12 relative (tests/test_offset_host.py measures a float64 floor
of 2e-15 on these cases, under the 1e-13 that keeps 1e-12), stage level 1e-9 (b, bschur, x) and 1e-11 (Hschur),
trajectories 1e-6 relative with identical trial counts, lm_pcg* tests/test_pcg.py's 1e-5, structure-only 1e-6 on state
and chi2 with equal counts, shards against one rank 1e-9 on the state and 1e-6 on chi2, marginals
tests/test_gpu_marginals.py's 1e-9.
"""
import threading
import uuid

import numpy as np
import pytest

import offset_ref as O
import pose_edges_ref as per
import structure_only_ref
from g2o_amd import synth
from offset_ref import BEAR, HOSTJ, KINDS, OFFSETS, PTAGS, SE2O, SE3O, TAGS

pytestmark = pytest.mark.gpu

RTOL = 1e-6
PCG_RTOL = 1e-5
ERR_ARG, ERR_UNSUPPORTED = -1, -4
_CACHE = {}  # problems and reference runs, computed once, shared, left unchanged


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _est_of(opt, prob):
    return {v.vtype: opt.estimates(v.vtype) for v in prob.vertices}


def _device(mod, prob, robust=None):
    opt = mod.SparseOptimizer(0).add_problem(prob)
    for et, (kind, delta) in (robust or {}).items():
        opt.set_robust_kernel(et, kind, delta)
    return opt


def _twin(mod, prob, robust=None, levels=None):
    """The graph with each offset / bearing edge set entered as an E_HOSTJ(D) set between the same vertices,
    offset_ref's records in the callback. robust: {edge type: (kind, delta)}."""
    g = O.Graph(prob)
    back = {HOSTJ[t]: t for t in KINDS}
    opt = mod.SparseOptimizer(0).add_problem(O.hostj_problem(prob))
    opt.set_host_edge_callback(lambda etype, with_jac: g.payload(back[etype], _est_of(opt, prob)))
    for et, (kind, delta) in (robust or {}).items():
        opt.set_robust_kernel(HOSTJ.get(et, et), kind, delta)
    for et, lv in (levels or {}).items():
        opt.set_edge_levels(HOSTJ[et], lv)
    return opt


def _stage_against(tag, s, r):
    assert s["ok"] == 1 and (s["n"], s["np"]) == (r["n"], r["np"]), (tag, s["n"], s["np"], r["n"], r["np"])
    for k in ("b", "x", "bschur"):
        err = np.linalg.norm(s[k] - r[k]) / np.linalg.norm(r[k])
        print(f"{tag} {k}: {err:.2e}")
        assert err <= 1e-9, (tag, k, err)
    err = np.linalg.norm(s["Hschur"] - r["Hschur"]) / np.linalg.norm(r["Hschur"])
    print(f"{tag} Hschur: {err:.2e}")
    assert err <= 1e-11, (tag, err)


def _stage_both(mod, tag, prob, robust=None):
    """The device and the twin, each against numpy at the handle's own estimates (quaternions as normalised on entry)."""
    for who, opt in (("device", _device(mod, prob, robust)), ("twin", _twin(mod, prob, robust))):
        est = _est_of(opt, prob)
        r = O.numpy_stage(prob, None, robust, est)
        _stage_against(f"{who} {tag}", opt.stage(r["lam"]), r)
        ref = O.Graph(prob).chi2(est=est, robust=robust)
        chi = opt.chi2()
        assert abs(chi - ref) <= 1e-12 * ref, (who, tag, chi, ref)


def _run(opt, iters, algo=None):
    if algo:
        opt.set_algorithm(algo)
    n, st = opt.optimize(iters)
    return n, [s.chi2 for s in st], [s.levenbergIterations for s in st], opt.minimal_state()


def _same_trajectory(a, b, tol=RTOL):
    (na, ca, ta, xa), (nb, cb, tb, xb) = a, b
    assert na == nb and ta == tb, (na, nb, ta, tb)
    for x, y in zip(ca, cb):
        assert abs(x - y) <= tol * abs(y), (x, y)
    assert np.linalg.norm(xa - xb) <= tol * np.linalg.norm(xb), np.linalg.norm(xa - xb) / np.linalg.norm(xb)


def _edge_set(prob, etype):
    return next(es for es in prob.edges if es.etype == etype)


# ---------------------------------------------------------------- 1: single-edge pins
@pytest.mark.parametrize("etype", KINDS)
def test_single_edge_pins(g2o_amd_mod, etype):
    prob = O.one_edge(etype)
    opt = _device(g2o_amd_mod, prob)
    est = _est_of(opt, prob)
    g = O.Graph(prob)
    ref = g.chi2(est=est)
    chi = opt.chi2()
    print(f"edge type {etype}: chi2 device {chi:.17g} numpy {ref:.17g} rel {abs(chi - ref) / ref:.2e}")
    assert ref > 0 and abs(chi - ref) <= 1e-12 * ref
    delta = 0.5 * np.sqrt(ref)  # sqrt(e2) > delta: Huber's linear branch, chi2 = rho
    opt.set_robust_kernel(etype, "Huber", delta)
    rho = 2 * np.sqrt(ref) * delta - delta * delta
    assert abs(opt.chi2() - rho) <= 1e-12 * rho
    assert abs(g.chi2(est=est, robust={etype: ("Huber", delta)}) - rho) <= 1e-12 * rho
    # the sign of the error: the single edge's b = -J^T Omega e
    opt2 = _device(g2o_amd_mod, prob)
    r = O.numpy_stage(prob, None, est=est)
    s = opt2.stage(r["lam"])
    assert np.linalg.norm(s["b"] - r["b"]) <= 1e-9 * np.linalg.norm(r["b"])
    assert np.linalg.norm(s["b"] + r["b"]) > np.linalg.norm(r["b"])


# ---------------------------------------------------------------- 2: stage level at the kernels' edges
@pytest.mark.parametrize("ne", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("etype,uniform", [(SE3O, False), (SE3O, True), (SE2O, False), (SE2O, True), (BEAR, False),
                                           (BEAR, True)])
def test_stage_kernel_edges(g2o_amd_mod, etype, uniform, ne):
    """A partial wave, a full wave, a wave plus one edge, one edge past a 256-thread block; per-edge distinct parameter
    and information records, and one shared record of each (EdgeData::ue bits 1 and 0)."""
    _stage_both(g2o_amd_mod, f"type {etype} ne={ne} uniform={uniform}", O.edge_case(etype, ne, uniform))


def test_stage_huber(g2o_amd_mod):
    """The robust weighting of the information for D = 6, 3 and the single scalar of D = 1."""
    for etype in KINDS:
        prob = O.edge_case(etype, 65)
        chi = O.Graph(prob).edge_chi2(etype)
        delta = float(np.sqrt(np.median(chi)))  # half of the edges on Huber's linear branch
        _stage_both(g2o_amd_mod, f"Huber type {etype}", prob, {etype: ("Huber", delta)})


# ---------------------------------------------------------------- 3: branch inputs
def _branch_cases():
    return ([(SE3O, c) for c in O.se3_branch_cases()] + [(SE2O, c) for c in O.se2_wrap_cases()] +
            [(BEAR, c) for c in O.bearing_cut_cases()])


@pytest.mark.parametrize("k", range(len(_branch_cases())))
def test_branch_inputs(g2o_amd_mod, k):
    """The dq_dR branch cases, the theta wraps and the atan2-cut cases of tests/test_offset_host.py as one-edge graphs."""
    etype, case = _branch_cases()[k]
    prob = O.one_edge(etype, case)
    opt = _device(g2o_amd_mod, prob)
    est = _est_of(opt, prob)
    ref = O.Graph(prob).chi2(est=est)
    chi = opt.chi2()
    print(f"type {etype} {case[0]}: chi2 {chi:.17g} numpy {ref:.17g} rel {abs(chi - ref) / ref:.2e}")
    assert abs(chi - ref) <= 1e-12 * ref
    r = O.numpy_stage(prob, None, est=est)
    s = opt.stage(r["lam"])
    err = np.linalg.norm(s["b"] - r["b"]) / np.linalg.norm(r["b"])
    print(f"b: {err:.2e}")
    assert err <= 1e-9


# ---------------------------------------------------------------- 4: identity offsets
@pytest.mark.parametrize("etype", OFFSETS)
def test_identity_offsets(g2o_amd_mod, etype):
    """params NULL: the chain as the offset type against the same chain as EdgeSE3 / EdgeSE2."""
    off, plain = O.identity_chain(etype)
    a, b = _device(g2o_amd_mod, off), _device(g2o_amd_mod, plain)
    assert abs(a.chi2() - b.chi2()) <= 1e-12 * b.chi2()
    lam = O.numpy_stage(plain, None)["lam"]
    sa, sb = a.stage(lam), b.stage(lam)
    _stage_against(f"identity type {etype}", sa, dict(sb, n=sb["n"], np=sb["np"]))
    _same_trajectory(_run(_device(g2o_amd_mod, off), 4, "lm_hip_var"), _run(_device(g2o_amd_mod, plain), 4, "lm_hip_var"))
    # the explicit identity records give the same numbers as NULL
    es = off.edges[0]
    expl = synth.Problem("explicit", off.vertices, [synth.EdgeSet(etype, es.v0, es.v1, es.meas, es.info,
                                                                  np.broadcast_to(O.IDENT[etype], (len(es.v0), len(O.IDENT[etype]))).copy())],
                         off.pose_dim, 0)
    assert _device(g2o_amd_mod, expl).chi2() == a.chi2()


# ---------------------------------------------------------------- 5: trajectories against the twin
def _graph(etype):
    return _cached(("graph", etype), {SE3O: synth.se3_offset_graph, SE2O: synth.se2_offset_graph,
                                     BEAR: synth.bearing_scene}[etype])


def _twin_run(mod, key, prob, algo, robust=None, iters=4):
    return _cached(("twinrun", key, algo, bool(robust), iters), lambda: _run(_twin(mod, prob, robust), iters, algo))


def test_twin_stage_pin(g2o_amd_mod):
    for key, prob in (("se3", _graph(SE3O)), ("se2", _graph(SE2O)), ("bearing", _graph(BEAR))):
        _stage_both(g2o_amd_mod, key, prob)


@pytest.mark.parametrize("algo", ["lm_hip_var", "gn_hip_var", "dl_hip_var"])
@pytest.mark.parametrize("etype", OFFSETS)
def test_offset_trajectory_against_twin(g2o_amd_mod, etype, algo):
    prob = _graph(etype)
    assert len(np.unique(prob.edges[0].params, axis=0)) == 4  # two sensors: four (from, to) pairs
    dev = _run(_device(g2o_amd_mod, prob), 4, algo)
    print(f"{algo} type {etype}: chi2 {dev[1]} trials {dev[2]}")
    _same_trajectory(dev, _twin_run(g2o_amd_mod, etype, prob, algo))
    assert dev[1][-1] < dev[1][0]


@pytest.mark.parametrize("etype", OFFSETS)
def test_offset_trajectory_huber(g2o_amd_mod, etype):
    prob = _graph(etype)
    delta = float(np.sqrt(np.median(O.Graph(prob).edge_chi2(etype))))
    robust = {etype: ("Huber", delta)}
    dev = _run(_device(g2o_amd_mod, prob, robust), 4, "lm_hip_var")
    print(f"Huber type {etype}: chi2 {dev[1]} trials {dev[2]}")
    _same_trajectory(dev, _twin_run(g2o_amd_mod, etype, prob, "lm_hip_var", robust))
    plain = _twin_run(g2o_amd_mod, etype, prob, "lm_hip_var")
    assert abs(dev[1][0] - plain[1][0]) > 1e-3 * plain[1][0]  # the kernel is at work: another trajectory


@pytest.mark.parametrize("algo", ["lm_hip_var", "lm_hip_fix3_2", "dl_hip_fix3_2", "gn_hip_fix3_2"])
def test_bearing_trajectory_against_twin(g2o_amd_mod, algo):
    """The marginalised scene on the 3/2 Schur path, under the variable-size and the fixed-size algorithm names (a
    graph whose free poses and free landmarks both sit in the pose part mixes block sizes 3 and 2, which the engine's
    one-pose-block-size rule refuses for every edge type)."""
    key, prob = "bearing", _graph(BEAR)
    dev = _run(_device(g2o_amd_mod, prob), 4, algo)
    print(f"{algo}: chi2 {dev[1]} trials {dev[2]}")
    _same_trajectory(dev, _twin_run(g2o_amd_mod, key, prob, algo))
    assert dev[1][-1] < dev[1][0]


def test_bearing_lm_pcg3_2(g2o_amd_mod):
    prob = _graph(BEAR)
    dev = _run(_device(g2o_amd_mod, prob), 4, "lm_pcg3_2")
    print(f"lm_pcg3_2: chi2 {dev[1]} trials {dev[2]}")
    _same_trajectory(dev, _twin_run(g2o_amd_mod, "bearing", prob, "lm_pcg3_2"), PCG_RTOL)


@pytest.mark.parametrize("etype", OFFSETS)
def test_offset_lm_pcg(g2o_amd_mod, etype):
    prob = _graph(etype)
    dev = _run(_device(g2o_amd_mod, prob), 4, "lm_pcg")
    _same_trajectory(dev, _twin_run(g2o_amd_mod, etype, prob, "lm_pcg"), PCG_RTOL)


# ---------------------------------------------------------------- 6: a mixed graph per dimension
def _mixed3d():
    """EdgeSE3 + EdgeSE3Offset + EdgeSE3Prior on one set of poses."""
    def make():
        base = synth.se3_offset_graph(num_poses=30, loops=40)
        es = base.edges[0]
        ev, od = np.arange(0, len(es.v0), 2), np.arange(1, len(es.v0), 2)
        poses = base.vertices[0]
        plain_z = []  # the odd edges as EdgeSE3: Z = Pi Z' Pj^-1
        for k in od:
            P = es.params[k].reshape(2, 7)
            Rpi, Rpj = per.rot(P[:, 3:])
            R, t = O._iso_mul(Rpi, P[0, :3], per.rot(es.meas[k, 3:])[0], es.meas[k, :3])
            R, t = O._iso_mul(R, t, Rpj.T, -Rpj.T @ P[1, :3])
            plain_z.append(per.pose_of(R, t))
        e1 = synth.EdgeSet(SE3O, es.v0[ev], es.v1[ev], es.meas[ev], es.info[ev], es.params[ev])
        e2 = synth.EdgeSet(synth.E_SE3_QUAT, es.v0[od], es.v1[od], np.array(plain_z), es.info[od])
        prob = synth.Problem("mixed3d", [poses], [e2, e1], 6, 0)
        return synth.with_priors(prob, synth.E_SE3_PRIOR, every=5, sigma=0.1)
    return _cached("mixed3d", make)


def _mixed2d():
    """EdgeSE2 + EdgeSE2Offset between the poses, EdgeSE2PointXY + EdgeSE2PointXYBearing on shared landmarks."""
    def make():
        sc = synth.bearing_scene()
        poses, lms = sc.vertices
        odo, obs = sc.edges
        off = synth.se2_offset_graph(num_poses=len(poses.ids), loops=10)
        # the offset graph's measurements for this scene's poses: Z = (Xi Pi)^-1 (Xj Pj) at the start, moved a little
        oe = off.edges[0]
        rng = np.random.default_rng(61)
        ni = synth._se2_compose(poses.est[oe.v0], oe.params[:, :3])
        nj = synth._se2_compose(poses.est[oe.v1], oe.params[:, 3:])
        zo = synth._se2_between(ni, nj) + 0.02 * rng.standard_normal((len(oe.v0), 3))
        e_off = synth.EdgeSet(SE2O, oe.v0, oe.v1, zo, oe.info, oe.params)
        half = np.arange(0, len(obs.v0), 2)
        zxy = per.se2xy_edge(poses.est[obs.v0[half]], lms.est[obs.v1[half] - lms.ids[0]], np.zeros((len(half), 2)), jac=False)
        e_xy = synth.EdgeSet(synth.E_SE2_XY, obs.v0[half], obs.v1[half], zxy + 0.03 * rng.standard_normal(zxy.shape),
                             per._spd(rng, 2, len(half)) * 100.0)
        return synth.Problem("mixed2d", [poses, lms], [odo, e_off, e_xy, obs], 3, 2)
    return _cached("mixed2d", make)


@pytest.mark.parametrize("dim", [3, 2])
def test_mixed_graph_stage(g2o_amd_mod, dim):
    prob = _mixed3d() if dim == 3 else _mixed2d()
    assert {es.etype for es in prob.edges} >= ({SE3O, synth.E_SE3_QUAT, synth.E_SE3_PRIOR} if dim == 3 else
                                               {SE2O, synth.E_SE2, synth.E_SE2_XY, BEAR})
    _stage_both(g2o_amd_mod, f"mixed {dim}d", prob)
    dev = _run(_device(g2o_amd_mod, prob), 3, "lm_hip_var" if dim == 3 else "lm_hip_fix3_2")
    ref = _run(_twin(g2o_amd_mod, prob), 3, "lm_hip_var" if dim == 3 else "lm_hip_fix3_2")
    _same_trajectory(dev, ref)


# ---------------------------------------------------------------- 7: structure-only
@pytest.mark.parametrize("prior", [False, True])
def test_structure_only_tracks(g2o_amd_mod, prior):
    """Bearing tracks of lengths 2, 7, 8, 9 and 65 (eight lanes per landmark), alone and beside an EdgeXYPrior."""
    prob = O.tracks_problem(prior=prior)
    s = O.Structure(prob)
    ref_est, results = s.calc(10)
    opt = _device(g2o_amd_mod, prob)
    poses_before = opt.estimates(synth.V_SE2)
    counts = opt.structure_only(iterations=10)
    print(f"prior={prior}: device {counts} reference {structure_only_ref.counts(results)}")
    assert counts == structure_only_ref.counts(results)
    got, ref = opt.estimates(synth.V_XY), ref_est[synth.V_XY]
    worst = np.max(np.linalg.norm(got - ref, axis=1) / np.linalg.norm(ref, axis=1))
    print(f"worst landmark {worst:.2e}")
    assert worst <= RTOL
    assert np.array_equal(opt.estimates(synth.V_SE2), poses_before)  # the poses are left bit for bit
    chi, chi_ref = opt.chi2(), s.graph_chi2(ref_est)
    assert abs(chi - chi_ref) <= RTOL * chi_ref, (chi, chi_ref)


def test_structure_only_2_algorithm(g2o_amd_mod):
    """optimize(1) under structure_only_2 is calc(points, 1)."""
    prob = O.tracks_problem()
    s = O.Structure(prob)
    ref_est, _ = s.calc(1)
    opt = _device(g2o_amd_mod, prob)
    opt.set_algorithm("structure_only_2")
    n, st = opt.optimize(1)
    chi_ref = s.graph_chi2(ref_est)
    assert n == 1 and abs(st[0].chi2 - chi_ref) <= RTOL * chi_ref
    got, ref = opt.estimates(synth.V_XY), ref_est[synth.V_XY]
    assert np.max(np.linalg.norm(got - ref, axis=1) / np.linalg.norm(ref, axis=1)) <= RTOL


# ---------------------------------------------------------------- 8: levels, per-edge chi2, classification
def _per_edge_problem(etype):
    return _cached(("per_edge", etype), O.per_edge_scene) if etype == BEAR else _graph(etype)


@pytest.mark.parametrize("etype", KINDS)
def test_levels_chi2_classify(g2o_amd_mod, etype):
    prob = _per_edge_problem(etype)
    algo = "lm_hip_fix3_2" if etype == BEAR else "lm_hip_var"
    opt = _device(g2o_amd_mod, prob)
    opt.initialize_optimization()
    ref = O.Graph(prob).edge_chi2(etype, _est_of(opt, prob))
    # some edges set aside first: the per-edge chi2 covers the inactive ones too
    lv = np.zeros(len(ref), np.int32)
    lv[::7] = 2
    opt.set_edge_levels(etype, lv)
    chi = opt.edge_chi2(etype)
    print(f"type {etype}: per-edge chi2 worst {np.max(np.abs(chi - ref) / ref):.2e}")
    assert len(chi) == len(ref) and np.max(np.abs(chi - ref) / ref) <= 1e-12
    srt = np.sort(ref)
    top = srt[len(srt) // 2:]  # a threshold in the upper half: some, not all, edges are outliers
    k = int(np.argmax(np.diff(top)))
    gap = (top[k + 1] - top[k]) / top[k]
    thr = 0.5 * (top[k] + top[k + 1])
    print(f"type {etype}: threshold {thr:.6g} in a gap of {gap:.2e} relative")
    assert gap > 1e-9
    bad = ref > thr
    counts = opt.classify_edges(etype, thr)
    assert counts == dict(over_chi2=int(bad.sum()), depth_failed=0, bad=int(bad.sum())) and 0 < bad.sum() < len(bad)
    assert np.array_equal(opt.edge_levels(etype), bad.astype(np.int32))
    with pytest.raises(g2o_amd_mod.G2OHipError) as ei:
        opt.classify_edges(etype, thr, check_depth=True)
    assert f"({ERR_ARG})" in str(ei.value)
    with pytest.raises(g2o_amd_mod.G2OHipError) as ei:
        opt.edge_chi2(etype, depth=True)
    assert f"({ERR_ARG})" in str(ei.value)
    opt.initialize_optimization(0)
    tw = _twin(g2o_amd_mod, prob, levels={etype: bad.astype(np.int32)})
    tw.initialize_optimization(0)
    dev, twr = _run(opt, 3, algo), _run(tw, 3, algo)
    _same_trajectory(dev, twr)
    assert dev[1][0] < float(np.sum(ref))  # the outliers are out of the system


# ---------------------------------------------------------------- 9: marginals
@pytest.mark.parametrize("etype", OFFSETS)
def test_marginals(g2o_amd_mod, etype):
    prob = _graph(etype)
    opt = _device(g2o_amd_mod, prob)
    opt.set_algorithm("lm_hip_var")
    opt.initialize_optimization()
    opt.build_structure()
    opt.build_system()
    pd, _, npose, _ = opt.block_dims()
    H = O.numpy_stage(prob, 0.0, est=_est_of(opt, prob))["H"]
    assert H.shape == (npose * pd, npose * pd)
    Hinv = np.linalg.inv(H)
    pat = [(0, 0), (3, 3), (3, 7), (npose - 1, npose - 1), (2, npose - 1)]
    blocks = opt.compute_marginals(pat)
    assert blocks is not None and len(blocks) == len(pat)
    num = den = 0.0
    for (r, c), B in blocks.items():
        Rf = Hinv[r * pd:(r + 1) * pd, c * pd:(c + 1) * pd]
        num += float(np.sum((B - Rf) ** 2))
        den += float(np.sum(Rf ** 2))
    print(f"type {etype}: marginals {np.sqrt(num / den):.2e}")
    assert np.sqrt(num / den) <= 1e-9


def test_update_initialization(g2o_amd_mod):
    """Online mode (non-Schur): offset edges added after two iterations join the system through
    update_initialization (no new vertex: the hessian order stays); chi2 and the stage level then are numpy's for the
    whole graph at the handle's estimates."""
    for etype in OFFSETS:
        prob = _graph(etype)
        es = prob.edges[0]
        n0 = len(es.v0) - 20
        first = synth.EdgeSet(etype, es.v0[:n0], es.v1[:n0], es.meas[:n0], es.info[:n0], es.params[:n0])
        rest = synth.EdgeSet(etype, es.v0[n0:], es.v1[n0:], es.meas[n0:], es.info[n0:], es.params[n0:])
        opt = _device(g2o_amd_mod, synth.Problem("first", prob.vertices, [first], prob.pose_dim, 0))
        opt.set_algorithm("lm_hip_var")
        opt.optimize(2)
        opt.add_edges(rest)
        opt.update_initialization()
        assert opt.num_edges() == len(es.v0)
        est = _est_of(opt, prob)
        ref = O.Graph(prob).chi2(est=est)
        assert abs(opt.chi2() - ref) <= 1e-12 * ref
        r = O.numpy_stage(prob, None, est=est)
        _stage_against(f"online type {etype}", opt.stage(r["lam"]), r)


# ---------------------------------------------------------------- 10: landmark shards
def test_two_local_ranks(g2o_amd_mod):
    prob = _graph(BEAR)
    nranks, iters = 2, 4
    key = uuid.uuid4().hex
    opts = [_device(g2o_amd_mod, prob) for _ in range(nranks)]
    for r, o in enumerate(opts):
        o.set_algorithm("lm_hip_fix3_2")
        o.set_comm_local(key, r, nranks)
    res, errs = [None] * nranks, []

    def body(r):
        try:
            res[r] = opts[r].optimize(iters)
        except Exception as ex:  # surfaced below
            errs.append(ex)

    th = [threading.Thread(target=body, args=(r,)) for r in range(nranks)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=600)
    assert not errs, errs
    single = _device(g2o_amd_mod, prob)
    single.set_algorithm("lm_hip_fix3_2")
    n1, st1 = single.optimize(iters)
    for r in range(nranks):
        n, st = res[r]
        assert n == n1
        for a, b in zip(st, st1):
            assert a.levenbergIterations == b.levenbergIterations
            assert abs(a.chi2 - b.chi2) <= RTOL * b.chi2
    held = [len(o.local_landmark_ids()) for o in opts]
    assert all(h > 0 for h in held) and sum(held) == 30, held
    # poses (3 each) from rank 0, each landmark (2 each) from the rank whose shard holds it
    N, lm_ids = prob.vertices[0].ids.size, prob.vertices[1].ids
    states = [o.minimal_state() for o in opts]
    assert np.array_equal(states[1][:3 * N], states[0][:3 * N])
    x = states[0].copy()
    seen = np.zeros(len(lm_ids), np.int32)
    for r, o in enumerate(opts):
        k = np.searchsorted(lm_ids, o.local_landmark_ids())
        seen[k] += 1
        rows = (3 * N + 2 * k[:, None] + np.arange(2)[None, :]).ravel()
        x[rows] = states[r][rows]
    assert np.all(seen == 1)
    xs = single.minimal_state()
    assert np.linalg.norm(x - xs) <= 1e-9 * np.linalg.norm(xs)


# ---------------------------------------------------------------- 11: .g2o files
@pytest.mark.parametrize("etype", KINDS)
def test_g2o_round_trip(g2o_amd_mod, tmp_path, etype):
    prob = _graph(etype)
    src = _device(g2o_amd_mod, prob)
    p1 = str(tmp_path / "a.g2o")
    src.save(p1)
    lines = open(p1).read().splitlines()
    tags = [ln.split()[0] for ln in lines]
    ne = len(_edge_set(prob, etype).v0)
    assert tags.count(TAGS[etype]) == ne
    first = next(ln for ln in lines if ln.startswith(TAGS[etype])).split()
    if etype in OFFSETS:  # one PARAMS line per distinct record (two sensors), ahead of the vertices
        assert tags.count(PTAGS[etype]) == 2 and tags[:2] == [PTAGS[etype]] * 2
        assert sorted(int(ln.split()[1]) for ln in lines[:2]) == [0, 1]
        D = synth.ERR_DIM[etype]
        assert len(first) == 5 + synth.MEAS_DIM[etype] + D * (D + 1) // 2
        assert {first[3], first[4]} <= {"0", "1"}
    else:
        assert len(first) == 5 and not any(t.startswith("PARAMS") for t in tags)
    back = g2o_amd_mod.SparseOptimizer(0)
    back.load(p1, offset=True)
    assert back.num_edges() == src.num_edges() and back.num_vertices() == src.num_vertices()
    assert abs(back.chi2() - src.chi2()) <= 1e-12 * src.chi2()
    s0, s1 = src.stage(1e-3), back.stage(1e-3)
    assert s0["np"] == s1["np"] and s0["nl"] == s1["nl"]
    assert np.linalg.norm(s0["x"] - s1["x"]) <= 1e-9 * np.linalg.norm(s0["x"])
    p2 = str(tmp_path / "b.g2o")
    back.save(p2)
    assert [ln.split()[0] for ln in open(p2).read().splitlines()] == tags
    plain = g2o_amd_mod.SparseOptimizer(0)
    plain.load(p1)  # without the flag the tags are skipped
    assert plain.num_edges() == src.num_edges() - ne and plain.num_vertices() == src.num_vertices()


V3 = "VERTEX_SE3:QUAT 0 0 0 0 0 0 0 1\nVERTEX_SE3:QUAT 1 1 0 0 0 0 0 1\n"
V2 = "VERTEX_SE2 0 0 0 0\nVERTEX_SE2 1 1 0 0.1\nVERTEX_XY 2 3 1\n"
I21 = " ".join(["1 0 0 0 0 0", "1 0 0 0 0", "1 0 0 0", "1 0 0", "1 0", "1"])
LOAD_FAILURES = [
    # (name, file text, what g2ohip_last_error names)
    ("undefined parameter id", "PARAMS_SE3OFFSET 0 0 0 0 0 0 0 1\n" + V3 + f"EDGE_SE3_OFFSET 0 1 0 5 1 0 0 0 0 0 1 {I21}\n",
     ("EDGE_SE3_OFFSET", " 5")),
    ("parameter of the wrong kind", "PARAMS_SE2OFFSET 0 0.1 0 0\nPARAMS_SE3OFFSET 1 0 0 0 0 0 0 1\n" + V3 +
     f"EDGE_SE3_OFFSET 0 1 1 0 1 0 0 0 0 0 1 {I21}\n", ("EDGE_SE3_OFFSET", " 0")),
    ("se2 edge naming an se3 parameter", "PARAMS_SE3OFFSET 4 0 0 0 0 0 0 1\nPARAMS_SE2OFFSET 1 0 0 0\n" + V2 +
     "EDGE_SE2_OFFSET 0 1 1 4 1 0 0.1 1 0 0 1 0 1\n", ("EDGE_SE2_OFFSET", " 4")),
    ("endpoint of the wrong type", "PARAMS_SE2OFFSET 0 0 0 0\n" + V2 + "EDGE_SE2_OFFSET 0 2 0 0 1 0 0.1 1 0 0 1 0 1\n",
     ("EDGE_SE2_OFFSET", "vertex 2")),
    ("bearing onto a pose", V2 + "EDGE_BEARING_SE2_XY 0 1 0.3 100\n", ("EDGE_BEARING_SE2_XY", "vertex 1")),
    ("missing endpoint", V2 + "EDGE_BEARING_SE2_XY 7 2 0.3 100\n", ("EDGE_BEARING_SE2_XY", "vertex 7")),
    ("short edge line", "PARAMS_SE2OFFSET 0 0 0 0\n" + V2 + "EDGE_SE2_OFFSET 0 1 0 0 1 0 0.1 1 0 0 1 0\n", ("EDGE_SE2_OFFSET",)),
    ("short bearing line", V2 + "EDGE_BEARING_SE2_XY 0 2 0.3\n", ("EDGE_BEARING_SE2_XY",)),
    ("short parameter line", "PARAMS_SE2OFFSET 0 0 0\n" + V2, ("PARAMS_SE2OFFSET",)),
]


@pytest.mark.parametrize("name,text,names", LOAD_FAILURES, ids=[c[0] for c in LOAD_FAILURES])
def test_g2o_load_failures(g2o_amd_mod, tmp_path, name, text, names):
    p = tmp_path / "bad.g2o"
    p.write_text(text)
    with pytest.raises(g2o_amd_mod.G2OHipError) as ei:
        g2o_amd_mod.SparseOptimizer(0).load(str(p), offset=True)
    assert f"({ERR_ARG})" in str(ei.value)
    for w in names:
        assert w in g2o_amd_mod.last_error(), (w, g2o_amd_mod.last_error())


def test_g2o_hand_written_file(g2o_amd_mod, tmp_path):
    """A file as the reference writes it, offsets that are no identities: chi2 against numpy."""
    text = ("PARAMS_SE2OFFSET 3 0.3 -0.2 0.7\nPARAMS_SE2OFFSET 9 -0.25 0.4 -1.2\n" + V2 +
            "EDGE_SE2_OFFSET 0 1 3 9 0.9 0.1 0.2 10 1 0 20 2 30\nEDGE_BEARING_SE2_XY 1 2 0.4 50\n")
    p = tmp_path / "hand.g2o"
    p.write_text(text)
    opt = g2o_amd_mod.SparseOptimizer(0)
    opt.load(str(p), offset=True)
    assert opt.num_edges() == 2 and opt.num_vertices() == 3
    e1 = O.se2_offset_edge([0, 0, 0], [1, 0, 0.1], [0.9, 0.1, 0.2], [0.3, -0.2, 0.7, -0.25, 0.4, -1.2], jac=False)[0]
    e2 = O.bearing_edge([1, 0, 0.1], [3, 1], [0.4], jac=False)[0]
    ref = e1 @ np.array([[10, 1, 0], [1, 20, 2], [0, 2, 30.0]]) @ e1 + 50 * e2[0] ** 2
    assert abs(opt.chi2() - ref) <= 1e-12 * ref


# ---------------------------------------------------------------- 12: refusals
def test_refusals(g2o_amd_mod):
    mod = g2o_amd_mod
    # the matrix-free CGLS, on each type
    for etype in KINDS:
        dev = _device(mod, _graph(etype))
        dev.set_algorithm("lm_pcg6_3_eigen")
        with pytest.raises(mod.G2OHipError) as ei:
            dev.optimize(1)
        assert f"({ERR_UNSUPPORTED})" in str(ei.value) and "offset and bearing" in mod.last_error()
        assert f"edge type {etype}" in mod.last_error()
        dev.set_algorithm("lm_hip_fix3_2" if etype == BEAR else "lm_hip_var")  # the graph is still usable
        n, st = dev.optimize(1)
        assert n == 1 and np.isfinite(st[0].chi2)
    # bearing: params must be NULL
    prob = O.one_edge(BEAR)
    es = prob.edges[0]
    opt = mod.SparseOptimizer(0)
    for vs in prob.vertices:
        opt.add_vertices(vs)
    with pytest.raises(mod.G2OHipError) as ei:
        opt.add_edges(synth.EdgeSet(BEAR, es.v0, es.v1, es.meas, es.info, np.zeros((1, 3))))
    assert f"({ERR_ARG})" in str(ei.value) and opt.num_edges() == 0
    # NULL v1: only the unary types take it
    for etype in KINDS:
        p1 = O.one_edge(etype)
        e1 = p1.edges[0]
        o1 = mod.SparseOptimizer(0)
        for vs in p1.vertices:
            o1.add_vertices(vs)
        with pytest.raises(mod.G2OHipError) as ei:
            o1.add_edges(synth.EdgeSet(etype, e1.v0, None, e1.meas, e1.info, e1.params))
        assert f"({ERR_ARG})" in str(ei.value) and o1.num_edges() == 0
    # the wrong parameter stride through the wrapper
    p3 = O.one_edge(SE3O)
    o3 = mod.SparseOptimizer(0)
    o3.add_vertices(p3.vertices[0])
    with pytest.raises(mod.G2OHipError) as ei:
        o3.add_edges(synth.EdgeSet(SE3O, p3.edges[0].v0, p3.edges[0].v1, p3.edges[0].meas, p3.edges[0].info, np.zeros((1, 7))))
    assert "14" in str(ei.value)
    # wrong vertex types: an SE3 offset edge between SE2 poses, a bearing between two poses
    p2 = O.one_edge(SE2O)
    wrong = mod.SparseOptimizer(0)
    wrong.add_vertices(p2.vertices[0])
    wrong.add_edges(synth.EdgeSet(SE3O, p2.edges[0].v0, p2.edges[0].v1, p3.edges[0].meas, p3.edges[0].info, None))
    with pytest.raises(mod.G2OHipError) as ei:
        wrong.initialize_optimization()
    assert f"({ERR_UNSUPPORTED})" in str(ei.value) and "vertex type 4" in str(ei.value)
    wrong = mod.SparseOptimizer(0)
    wrong.add_vertices(p2.vertices[0])
    wrong.add_edges(synth.EdgeSet(BEAR, p2.edges[0].v0, p2.edges[0].v1, es.meas, es.info, None))
    with pytest.raises(mod.G2OHipError) as ei:
        wrong.initialize_optimization()
    assert f"({ERR_UNSUPPORTED})" in str(ei.value) and "vertex type 4" in str(ei.value)
    # structure_only_3 on the 2D scene
    so = _device(mod, _graph(BEAR))
    so.set_algorithm("structure_only_3")
    assert mod.lib().g2ohip_initialize(so.h) == ERR_UNSUPPORTED
    assert "structure_only_3" in mod.last_error() and "dimension" in mod.last_error()
