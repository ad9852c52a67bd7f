"""EdgeSE3Expmap and the pose-only projections on the device (G2OHIP_E_SE3_EXPMAP, G2OHIP_E_SE3_PROJECT_XYZ_ONLYPOSE,
G2OHIP_E_STEREO_SE3_PROJECT_XYZ_ONLYPOSE): FamilyExpmap through k_linearize, the two pose-only families through
k_linearize_unary, chi2, robust kernels, the mixed-group slot path, shards, online updates, .g2o files and the refusals.

References: tests/expmap_ref.py (plain numpy) at the single-edge and stage level; the same graph entered as host-J
edges (G2OHIP_E_HOSTJ(6), G2OHIP_E_HOSTJ_UNARY(D)) with expmap_ref's records in the callback for the LM trajectories;
for the monocular pose-only type also the CPU oracle on synth.pose_only_twin (binary projections to fixed points: the
oracle takes fixed VertexSBAPointXYZ vertices). The stereo twin differs by the float rounding of 1/z and serves no pin.

Tolerances are the project's own (tests/test_gpu_stereo.py, tests/test_gpu_unary.py): chi2 pins 1e-12, stage level 1e-9
(b, bschur, x) and 1e-11 (Hschur), trajectories 1e-6 relative with identical trial counts, shards against one rank 1e-9,
online against a fresh graph 1e-9. acos near 1: every pinned EdgeSE3Expmap case keeps its residual angles below 0.004
rad or inside [0.05, 2.5] (asserted); the one case inside the band is held to expmap_ref.BAND_TOL.
"""
import threading
import uuid

import numpy as np
import pytest

import expmap_ref as ref
import unary_ref
from g2o_amd import synth
from shard_util import gather_sharded_state

pytestmark = pytest.mark.gpu

RTOL = 1e-6
# the tolerance of the case inside acos' band: 4 x the float64 / np.longdouble difference of expmap_ref's chi2 for that
# case, measured 3.75e-15 by tests/test_expmap_host.py::test_band_tolerance and kept (rounded up to 3.8e-15) in
# expmap_ref.BAND_MEASURED: 1.52e-14
BAND_TOL = ref.BAND_TOL
E_MONO, E_STEREO, E_EXPMAP = ref.E_MONO, ref.E_STEREO, ref.E_EXPMAP
_CACHE = {}  # problems and reference runs, computed once, shared, left unchanged


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _est_of(opt, prob):
    return {v.vtype: opt.estimates(v.vtype) for v in prob.vertices}


def _stage_against(tag, s, r, schur=False, keys=("b", "x")):
    for k in keys + (("bschur",) if schur else ()):
        err = np.linalg.norm(s[k] - r[k]) / np.linalg.norm(r[k])
        print(f"{tag} {k}: {err:.2e}")
        assert err <= 1e-9, (tag, k, err)
    if schur:
        err = np.linalg.norm(s["Hschur"] - r["Hschur"]) / np.linalg.norm(r["Hschur"])
        print(f"{tag} Hschur: {err:.2e}")
        assert err <= 1e-11, (tag, err)


def _numpy_stage(prob, lam, ld=0, robust=None):
    g = ref.Graph(prob)
    H, b = g.dense_system(robust=robust)
    Hs, bs, x = unary_ref.solve(H, b, g.npose, lam, ld)
    return dict(b=b, x=x, Hschur=Hs, bschur=bs)


def _run(opt, iters, lambda_init=0.0):
    n, st = opt.optimize(iters, lambda_init=lambda_init)
    return n, [s.chi2 for s in st], [s.levenbergIterations for s in st], opt.minimal_state()


def _same_trajectory(a, b, tol=RTOL):
    (na, ca, ta, xa), (nb, cb, tb, xb) = a, b
    assert na == nb and ta == tb, (na, nb, ta, tb)
    for x, y in zip(ca, cb):
        assert abs(x - y) <= tol * abs(y), (x, y)
    assert np.linalg.norm(xa - xb) <= tol * np.linalg.norm(xb), np.linalg.norm(xa - xb) / np.linalg.norm(xb)


def _hostj(mod, prob, robust=None):
    """The graph with its EdgeSE3Expmap / pose-only sets entered as host-J sets, expmap_ref's records in the callback."""
    hp, back = ref.hostj_version(prob)
    g = ref.Graph(prob)
    opt = mod.SparseOptimizer(0).add_problem(hp)
    opt.set_host_edge_callback(lambda etype, with_jac: g.payload(back[etype], _est_of(opt, prob)))
    for ht, et in back.items():
        if robust and et in robust:
            opt.set_robust_kernel(ht, *robust[et])
    return opt


# ---------------------------------------------------------------- 1: single-edge pins
def _pin(mod, prob, etype):
    g = ref.Graph(prob)
    want = g.chi2()
    opt = mod.SparseOptimizer(0).add_problem(prob)
    chi = opt.chi2()
    print(f"{prob.name}: chi2 device {chi:.17g} numpy {want:.17g} rel {abs(chi - want) / want:.2e}")
    assert want > 0 and abs(chi - want) <= 1e-12 * want
    delta = 0.5 * np.sqrt(want)  # sqrt(e2) > delta: Huber's linear branch, chi2 = rho
    opt.set_robust_kernel(etype, "Huber", delta)
    rho = 2 * np.sqrt(want) * delta - delta * delta
    assert abs(opt.chi2() - rho) <= 1e-12 * rho
    assert abs(g.chi2(robust={etype: ("Huber", delta)}) - rho) <= 1e-12 * rho


@pytest.mark.parametrize("etype", [E_MONO, E_STEREO])
def test_single_edge_pins_pose_only(g2o_amd_mod, etype):
    _pin(g2o_amd_mod, ref.one_pose_only(etype), etype)


@pytest.mark.parametrize("kind", ["small", "regular", "wneg"])
def test_single_edge_pins_expmap(g2o_amd_mod, kind):
    """Both endpoints free. small: the series branch of log (residual angle 0.003); regular: acos / tan; wneg: the
    quaternion of Tj^-1 * C has w < 0 before SE3Quat::operator* normalises it."""
    prob = ref.one_expmap(kind)
    es, est = prob.edges[0], prob.vertices[0].est
    e, (w1, _) = ref.expmap_error(est[0], est[1], es.meas[0], raw=True)
    ang = np.linalg.norm(e[:3])
    ref.assert_outside_band([ang])
    assert (ang < 0.004) == (kind == "small") and (w1 < 0) == (kind == "wneg")
    _pin(g2o_amd_mod, prob, E_EXPMAP)
    # the linearization too: both Jacobians and the error enter b and x
    s = g2o_amd_mod.SparseOptimizer(0).add_problem(prob).stage(1e-3)
    _stage_against(prob.name, s, _numpy_stage(prob, 1e-3))


# ---------------------------------------------------------------- 2: stage level at the kernels' edges
def _other(etype):
    return E_STEREO if etype == E_MONO else E_MONO


def _as_type(es, etype, rows, cams):
    """Rows of a pose-only edge set as an edge set of the given pose-only type (the second group of the stage
    cases): stereo from monocular gets u_r = u - bf / z at the estimates + 1.5 px and bf = 40, monocular from stereo
    drops u_r and bf."""
    rng = np.random.default_rng(len(rows) + etype)
    n = len(rows)
    if etype == es.etype:
        return synth.EdgeSet(etype, es.v0[rows].copy(), None, es.meas[rows].copy(), es.info[rows].copy(), es.params[rows].copy())
    info = np.stack([ref._spd(rng, synth.ERR_DIM[etype]) for _ in range(n)])
    if etype == E_MONO:
        return synth.EdgeSet(etype, es.v0[rows].copy(), None, es.meas[rows, :2].copy(), info, es.params[rows, :7].copy())
    T = cams.est[es.v0[rows] - cams.ids[0]]
    z = ref._map_n(T, es.params[rows, :3])[:, 2]
    meas = np.column_stack([es.meas[rows], es.meas[rows, 0] - 40.0 / z + 1.5])
    return synth.EdgeSet(etype, es.v0[rows].copy(), None, meas, info, np.column_stack([es.params[rows], np.full(n, 40.0)]))


def _pose_only_case(etype, ne, nc):
    """nc free cameras holding ne pose-only edges of the type, dealt round-robin, plus one edge on a further, fixed
    camera (inactive) in the middle of the set. Returns (problem, problem with a second unary group of the other
    pose-only type behind the first: three edges on camera 0 and one on the fixed camera)."""
    need = -(-ne // nc)
    scene = synth.pose_only(nc + 1, 2 * need + 24, stereo=etype == E_STEREO, seed=900 + ne + nc)
    (cams,), (es,) = scene.vertices, scene.edges
    per = [np.nonzero(es.v0 == c)[0] for c in cams.ids]
    assert all(len(p) >= need + 4 for p in per)
    rows = [per[k % nc][k // nc] for k in range(ne)]
    rows.insert(ne // 2, per[nc][0])
    fixed = cams.fixed.copy()
    fixed[nc] = 1
    cams = synth.VertexSet(cams.vtype, cams.ids, cams.est, fixed, cams.marginalized)
    first = _as_type(es, etype, np.array(rows), cams)
    p1 = synth.Problem(f"po{etype}n{ne}c{nc}", [cams], [first], 6, 0)
    second = _as_type(es, _other(etype), np.concatenate([per[0][-3:], per[nc][1:2]]), cams)
    return p1, synth.Problem(p1.name + "+2nd", [cams], [first, second], 6, 0)


# (ne, cameras): see test_stage_pose_only_kernel_edges
POSE_ONLY_LAYOUTS = [(1, 1), (63, 1), (63, 11), (63, 4), (64, 1), (64, 10), (64, 4), (65, 1), (65, 4), (257, 1),
                     (257, 3)]


@pytest.mark.parametrize("ne,nc", POSE_ONLY_LAYOUTS)
@pytest.mark.parametrize("etype", [E_MONO, E_STEREO])
def test_stage_pose_only_kernel_edges(g2o_amd_mod, oracle, etype, ne, nc):
    """k_linearize_unary at a partial wave, a full wave, a wave plus one edge and one edge past a 256-thread block, all
    edges on one camera or spread over several. The slot reduction picks its lanes per vertex from the average number
    of slots per pose vertex (Engine::build_structure): 64 (the wide kernel) from 128, 8 from 16, 4 from 6, else 1.
    The layouts give averages of 1 (1 lane), 63 / 11 = 5.7 (1), 64 / 10 = 6.4 (4), 63 / 4 = 15.75 (4), 64 / 4 = 16 (8),
    65 / 4 = 16.25 (8), 63 to 65 on one camera (8), 257 / 3 = 85.7 (8) and 257 on one camera (64): both sides of 6, 16
    and 128. One more edge sits on a fixed camera (inactive). With a second unary group behind the first (the other
    pose-only type) the second group starts at slot ne of the 27-double arena: an odd offset in doubles for the odd
    ne. The monocular type is also checked against the oracle on the twin. A camera that sees one point has a
    rank-2 H of ~1e6 (J ~ 1e3 px per unit) beside lambda = 1e-3: the rounding of b in H's null space, ~1e-16 |b|,
    reaches x magnified by 1e9, so for ne = 1 x is compared only in the second graph, where camera 0 sees four
    points."""
    lam = 1e-3
    p1, p2 = _pose_only_case(etype, ne, nc)
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(p1)
    s = opt.stage(lam)
    keys = ("b", "x") if ne >= 3 * nc else ("b",)
    _stage_against(f"{p1.name} numpy", s, _numpy_stage(p1, lam), keys=keys)
    assert len(s["b"]) == 6 * nc and opt.num_edges() == ne + 1
    want = ref.Graph(p1).chi2()
    assert abs(opt.chi2() - want) <= 1e-12 * want
    if etype == E_MONO:
        _stage_against(f"{p1.name} twin", s, oracle.OracleGraph(synth.pose_only_twin(p1)).stage(lam), keys=keys)
    s2 = g2o_amd_mod.SparseOptimizer(0).add_problem(p2).stage(lam)
    _stage_against(f"{p2.name} numpy", s2, _numpy_stage(p2, lam))
    assert not np.array_equal(s2["b"][:6], s["b"][:6])


@pytest.mark.parametrize("ne", [1, 63, 64, 65, 257])
def test_stage_expmap_kernel_edges(g2o_amd_mod, ne):
    """k_linearize<FamilyExpmap>: a chain from the fixed pose 0 (its first edge has a fixed endpoint) with up to three
    loop closures, ne edges in all; half the residuals on the series branch of log, half on the acos branch."""
    loops = min(3, ne - 1)
    prob = ref.expmap_case(ne - loops + 1, loops, 500 + ne)
    g = ref.Graph(prob)
    ref.assert_outside_band(g.residual_angles())
    assert prob.num_edges == ne and prob.vertices[0].fixed[0] == 1
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    want = g.chi2()
    chi = opt.chi2()
    print(f"expmap ne={ne}: chi2 device {chi:.17g} numpy {want:.17g} rel {abs(chi - want) / want:.2e}")
    assert abs(chi - want) <= 1e-12 * want
    _stage_against(f"expmap ne={ne}", opt.stage(1e-3), _numpy_stage(prob, 1e-3))


def test_expmap_inside_acos_band(g2o_amd_mod):
    """Every residual angle inside (0.0045, 0.05), where acos(d) is ill-conditioned: chi2 within BAND_TOL of numpy.
    Measured on the MI355X: device 275.39440923355312, numpy 275.39440923355181, 4.7e-15 relative (log's
    omega = theta / (2 sin theta) deltaR is well conditioned in d: an error in d moves theta and sin theta together)."""
    prob = ref.band_case()
    g = ref.Graph(prob)
    ang = g.residual_angles()
    assert ang.min() > 0.0045 and ang.max() < 0.05
    want = g.chi2()
    chi = g2o_amd_mod.SparseOptimizer(0).add_problem(prob).chi2()
    print(f"band case: chi2 device {chi:.17g} numpy {want:.17g} rel {abs(chi - want) / want:.3e} (tolerance {BAND_TOL:.3e})")
    assert abs(chi - want) <= BAND_TOL * want


# ---------------------------------------------------------------- 3: shared and per-edge intrinsics
@pytest.mark.parametrize("etype", [E_MONO, E_STEREO])
def test_shared_and_per_edge_intrinsics(g2o_amd_mod, etype):
    """One intrinsics record for all edges (the device keeps a single record: EdgeData::ue bit 1) and two cameras'
    intrinsics interleaved (per-edge records): each against numpy, and the two differ."""
    base = synth.pose_only(3, 40, stereo=etype == E_STEREO, seed=31)
    es = base.edges[0]
    assert (es.params[:, 3:] == es.params[0, 3:]).all()
    par = es.params.copy()
    par[1::2, 3:7] = [980.0, 1015.0, 310.0, 250.0]
    if etype == E_STEREO:
        par[1::2, 7] = 88.0
    mixed = synth.Problem(base.name + "/2K", base.vertices, [synth.EdgeSet(es.etype, es.v0, None, es.meas, es.info, par)], 6, 0)
    out = []
    for p in (base, mixed):
        opt = g2o_amd_mod.SparseOptimizer(0).add_problem(p)
        s = opt.stage(1e-3)
        _stage_against(p.name, s, _numpy_stage(p, 1e-3))
        want = ref.Graph(p).chi2()
        assert abs(opt.chi2() - want) <= 1e-12 * want
        out.append(s)
    assert np.linalg.norm(out[0]["b"] - out[1]["b"]) > 1e-3 * np.linalg.norm(out[0]["b"])


# ---------------------------------------------------------------- 4: trajectories
# Pose optimisation converges in three iterations from g2o's own initial damping, and the other seven sit at the
# rounding floor, where the sign of the gain ratio, and with it the trial count, is rounding noise (device and oracle
# then differ). A user lambda_init of 1e9 keeps all ten iterations at work (chi2 still falls by 1 % in the tenth), for
# the device, the host-J version and the oracle alike.
POSE_ONLY_LAMBDA0 = 1e9


def _twin_run(oracle, prob, iters):
    def make():
        twin = synth.pose_only_twin(prob)
        og = oracle.OracleGraph(twin)
        n, st = og.optimize(iters, oracle.make_config(threads=8, lambda_init=POSE_ONLY_LAMBDA0))
        extra = sum(3 * len(v.ids) for v in twin.vertices[len(prob.vertices):])
        x = og.minimal_state()
        return n, [s.chi2 for s in st], [s.levenbergIterations for s in st], x[:len(x) - extra]
    return _cached(("twin", prob.name, iters), make)


@pytest.mark.parametrize("stereo", [False, True])
def test_trajectory_pose_only(g2o_amd_mod, oracle, stereo):
    """pose_only(8 cameras x 120 points), ten LM iterations: the device types against the same graph entered as
    G2OHIP_E_HOSTJ_UNARY(D) with expmap_ref's records, the monocular one also against the oracle on the twin."""
    prob = _cached(("po", stereo), lambda: synth.pose_only(8, 120, stereo=stereo, cam_rot_noise=0.01, cam_trans_noise=0.05))
    dev = _run(g2o_amd_mod.SparseOptimizer(0).add_problem(prob), 10, POSE_ONLY_LAMBDA0)
    print(f"pose_only stereo={stereo}: chi2 {dev[1]} trials {dev[2]}")
    assert dev[0] == 10 and dev[1][-1] < 0.5 * ref.Graph(prob).chi2() and dev[1][-1] < 0.995 * dev[1][-2]
    _same_trajectory(dev, _run(_hostj(g2o_amd_mod, prob), 10, POSE_ONLY_LAMBDA0))
    if not stereo:
        _same_trajectory(dev, _twin_run(oracle, prob, 10))


@pytest.mark.parametrize("algo", ["lm_hip_fix6_6", "lm_hip_var"])
def test_trajectory_expmap_pose_graph(g2o_amd_mod, algo):
    """expmap_pose_graph(200 poses) against G2OHIP_E_HOSTJ(6) with expmap_ref's records."""
    prob = _cached("pg200", lambda: synth.expmap_pose_graph(200, 40))
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    opt.set_algorithm(algo)
    dev = _run(opt, 10)
    print(f"expmap_pose_graph {algo}: chi2 {dev[1]} trials {dev[2]}")
    assert dev[1][-1] < 0.5 * ref.Graph(prob).chi2()
    hj = _cached(("pg200hj", algo), lambda: _hostj_run(g2o_amd_mod, prob, algo, 10))
    _same_trajectory(dev, hj)


def _hostj_run(mod, prob, algo, iters):
    opt = _hostj(mod, prob)
    opt.set_algorithm(algo)
    return _run(opt, iters)


def _mixed_problem():
    """A small BA (12 cameras x 300 points) plus pose-only edges on every third camera plus three EdgeSE3Expmap between
    cameras (one from a fixed camera): three device groups of different arity on the slot path."""
    def make():
        base = synth.with_pose_only(synth.ba(12, 300, obs_per_point=4, window=6), every=3, per_camera=10)
        cams = base.vertices[0]
        a, b = np.array([0, 2, 3]), np.array([7, 5, 9])
        rng = np.random.default_rng(41)
        r = rng.standard_normal((3, 6)) * [0.002, 0.002, 0.002, 0.01, 0.01, 0.01]
        C = np.stack([ref.mul(ref.mul(ref.from_vector(cams.est[j]), ref.exp(x)), ref.inv(ref.from_vector(cams.est[i])))
                      for i, j, x in zip(a, b, r)])
        info = np.stack([ref._spd(rng, 6) for _ in range(3)]) * 1e4
        es = synth.EdgeSet(E_EXPMAP, cams.ids[a].copy(), cams.ids[b].copy(), C, info)
        return synth.Problem(base.name + "+expmap3", base.vertices, base.edges + [es], 6, 3)
    return _cached("mixed", make)


def test_trajectory_mixed_groups(g2o_amd_mod):
    """BA + pose-only + EdgeSE3Expmap under lm_hip_fix6_3 (the mixed-group slot path) against the version whose
    pose-only and EdgeSE3Expmap sets are host-J; the stage level against numpy first."""
    prob = _mixed_problem()
    assert [e.etype for e in prob.edges] == [synth.E_SE3_PROJECT_XYZ, E_MONO, E_EXPMAP]
    _stage_against("mixed numpy", g2o_amd_mod.SparseOptimizer(0).add_problem(prob).stage(1e-3),
                   _numpy_stage(prob, 1e-3, 3), True)
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    opt.set_algorithm("lm_hip_fix6_3")
    dev = _run(opt, 10)
    print(f"mixed: chi2 {dev[1]} trials {dev[2]}")
    assert opt.kernel_bytes("linearize_unary") > 0  # the unary class ran: the slot path, not the fused one
    _same_trajectory(dev, _hostj_run(g2o_amd_mod, prob, "lm_hip_fix6_3", 10))


# ---------------------------------------------------------------- 5: robust kernels
@pytest.mark.parametrize("kind", ["Huber", "PseudoHuber", "Cauchy", "GemanMcClure", "Welsch", "Fair", "Tukey",
                                  "Saturated", "DCS"])
def test_robust_kernels_on_pose_only(g2o_amd_mod, kind):
    """Every kernel of the factory on the monocular pose-only type: robust chi2 and the rho'-weighted system."""
    prob = _cached("rk", lambda: synth.pose_only(4, 40, pixel_noise=3.0, seed=51))
    rob = {E_MONO: (kind, 2.5)}
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    opt.set_robust_kernel(E_MONO, kind, 2.5)
    g = ref.Graph(prob)
    want = g.chi2(robust=rob)
    assert abs(opt.chi2() - want) <= 1e-12 * want
    assert want < g.chi2()  # the kernel bites
    _stage_against(f"robust {kind}", opt.stage(1e-3), _numpy_stage(prob, 1e-3, robust=rob))


def test_huber_on_expmap(g2o_amd_mod):
    prob = ref.expmap_case(40, 3, 61)
    g = ref.Graph(prob)
    ref.assert_outside_band(g.residual_angles())
    rob = {E_EXPMAP: ("Huber", 20.0)}
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    opt.set_robust_kernel(E_EXPMAP, "Huber", 20.0)
    want = g.chi2(robust=rob)
    assert abs(opt.chi2() - want) <= 1e-12 * want and want < g.chi2()
    _stage_against("huber expmap", opt.stage(1e-3), _numpy_stage(prob, 1e-3, robust=rob))


# ---------------------------------------------------------------- 6: landmark shards
def test_two_local_ranks(g2o_amd_mod):
    """The mixed graph on two ranks: the pose-only and EdgeSE3Expmap edges touch no free landmark and are assembled
    by rank 0 once; nothing counted twice or dropped."""
    prob = _mixed_problem()
    nranks, iters = 2, 4
    key = uuid.uuid4().hex
    opts = [g2o_amd_mod.SparseOptimizer(0).add_problem(prob) for _ in range(nranks)]
    for r, o in enumerate(opts):
        o.set_algorithm("lm_hip_fix6_3")
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
    single = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    single.set_algorithm("lm_hip_fix6_3")
    n1, st1 = single.optimize(iters)
    for r in range(nranks):
        n, st = res[r]
        assert n == n1
        for a, b in zip(st, st1):
            assert a.levenbergIterations == b.levenbergIterations
            assert abs(a.chi2 - b.chi2) <= RTOL * b.chi2
    x, _ = gather_sharded_state(prob, opts)
    xs = single.minimal_state()
    assert np.linalg.norm(x - xs) <= 1e-9 * np.linalg.norm(xs)


# ---------------------------------------------------------------- 7: online
def test_online_added_poses(g2o_amd_mod):
    """expmap_pose_graph: 60 poses optimised, then ten poses and their edges added through
    g2ohip_update_initialization, against a fresh graph of all 70 started from the same state."""
    full = synth.expmap_pose_graph(70, 14, seed=71)
    (vs,), (es,) = full.vertices, full.edges
    old_v = vs.ids < 60
    old_e = (es.v0 < 60) & (es.v1 < 60)
    assert (~old_e).sum() >= 10

    def vsub(m, est=None):
        return synth.VertexSet(vs.vtype, vs.ids[m], (vs.est if est is None else est)[m], vs.fixed[m], vs.marginalized[m])

    def esub(m):
        return synth.EdgeSet(es.etype, es.v0[m], es.v1[m], es.meas[m], es.info[m])

    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(synth.Problem("before", [vsub(old_v)], [esub(old_e)], 6, 0))
    opt.optimize(3)
    est = vs.est.copy()
    est[old_v] = opt.estimates(vs.vtype)
    opt.add_vertices(vsub(~old_v))
    opt.add_edges(esub(~old_e))
    opt.update_initialization()
    on = _run(opt, 4)
    fresh = synth.Problem("fresh", [vsub(old_v, est), vsub(~old_v)], [esub(old_e), esub(~old_e)], 6, 0)
    fr = _run(g2o_amd_mod.SparseOptimizer(0).add_problem(fresh), 4)
    _same_trajectory(on, fr, 1e-9)
    assert opt.num_edges() == full.num_edges and len(on[3]) == 6 * 70 and on[1][-1] < on[1][0]


# ---------------------------------------------------------------- 8: .g2o files
def test_g2o_round_trip(g2o_amd_mod, tmp_path):
    """Save -> load(expmap=True): counts and chi2 equal, and the file saved again from the loaded graph has the same
    edge lines (shortest round-trip decimals; the comparison of tests/test_gpu_unary.py). The measurement goes through
    two inversions (the file holds cam2world), so the reloaded chi2 agrees to rounding, not bit for bit. Flags 0 skip
    the tag: vertices and no edges."""
    prob = synth.expmap_pose_graph(30, 6, seed=81, init="truth")  # every edge has a residual of the noise's size
    src = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    p1, p2, p3 = (str(tmp_path / n) for n in ("a.g2o", "b.g2o", "c.g2o"))
    src.save(p1)
    text = open(p1).read()
    assert text.count("EDGE_SE3:EXPMAP ") == prob.num_edges == 35
    line = next(ln for ln in text.splitlines() if ln.startswith("EDGE_SE3:EXPMAP"))
    assert len(line.split()) == 1 + 2 + 7 + 21
    # the written seven values are the inverse of the measurement
    w = np.array(line.split()[3:10], float)
    assert np.allclose(ref.inv(ref.from_vector(prob.edges[0].meas[0])), w, rtol=0, atol=1e-14)
    back = g2o_amd_mod.SparseOptimizer(0)
    back.load(p1, expmap=True)
    assert back.num_edges() == src.num_edges() and back.num_vertices() == src.num_vertices()
    c0, c1 = src.chi2(), back.chi2()
    assert abs(c0 - c1) <= 1e-12 * c0, (c0, c1)
    est0, est1 = src.estimates(synth.V_SE3_EXPMAP), back.estimates(synth.V_SE3_EXPMAP)
    assert np.abs(est0 - est1).max() <= 1e-14 * np.abs(est0).max()
    back.save(p2)
    again = g2o_amd_mod.SparseOptimizer(0)
    again.load(p2, expmap=True)
    again.save(p3)

    def rest(t):
        return [ln for ln in t.splitlines() if not ln.startswith("VERTEX")]

    # inverting twice is not bit-exact, so a -> b may move last digits; b -> c is compared to 1e-14 per value
    for la, lb in zip(rest(open(p2).read()), rest(open(p3).read())):
        fa, fb = la.split(), lb.split()
        assert fa[:3] == fb[:3] and np.allclose(np.array(fa[3:], float), np.array(fb[3:], float), rtol=1e-14, atol=1e-14)
    plain = g2o_amd_mod.SparseOptimizer(0)
    plain.load(p1)
    assert plain.num_edges() == 0 and plain.num_vertices() == 30
    both = g2o_amd_mod.SparseOptimizer(0)
    both.load(p1, unary=True, slam3d=True, expmap=True)  # the flags combine
    assert both.num_edges() == 35


def test_g2o_bad_lines_fail(g2o_amd_mod, tmp_path):
    info = " ".join("1" if r == c else "0" for r in range(6) for c in range(r, 6))
    head = "VERTEX_SE3:EXPMAP 0 0 0 0 0 0 0 1\nVERTEX_SE3:EXPMAP 1 1 0 0 0 0 0 1\nVERTEX_SE3:QUAT 2 1 0 0 0 0 0 1\n"
    short = tmp_path / "short.g2o"
    short.write_text(head + f"EDGE_SE3:EXPMAP 0 1 1 0 0 0 0 0 1 {info[:-4]}\n")
    with pytest.raises(g2o_amd_mod.G2OHipError) as ei:
        g2o_amd_mod.SparseOptimizer(0).load(str(short), expmap=True)
    assert "EDGE_SE3:EXPMAP" in str(ei.value)
    wrong = tmp_path / "wrong.g2o"
    wrong.write_text(head + f"EDGE_SE3:EXPMAP 0 2 1 0 0 0 0 0 1 {info}\n")
    with pytest.raises(g2o_amd_mod.G2OHipError) as ei:
        g2o_amd_mod.SparseOptimizer(0).load(str(wrong), expmap=True)
    assert "EDGE_SE3:EXPMAP" in str(ei.value) and "vertex 2" in str(ei.value)
    ok = tmp_path / "ok.g2o"
    ok.write_text(head + f"EDGE_SE3:EXPMAP 0 1 1 0 0 0 0 0 1 {info}\n"
                  "EDGE_SE3_PROJECT_XYZONLYPOSE:EXPMAP 1 10 20 1 0 1\n")
    opt = g2o_amd_mod.SparseOptimizer(0)
    opt.load(str(ok), expmap=True)  # the pose-only tag is skipped
    assert opt.num_edges() == 1
    g2o_amd_mod.SparseOptimizer(0).load(str(short))  # without the flag the short line is a skipped tag


@pytest.mark.parametrize("stereo", [False, True])
def test_save_with_pose_only_is_unsupported(g2o_amd_mod, tmp_path, stereo):
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(synth.pose_only(2, 5, stereo=stereo))
    path = tmp_path / "po.g2o"
    with pytest.raises(g2o_amd_mod.G2OHipError) as ei:
        opt.save(str(path))
    assert "(-4)" in str(ei.value) and "pose-only" in str(ei.value)
    assert not path.exists()


# ---------------------------------------------------------------- 9: refusals
def test_refusals(g2o_amd_mod):
    mod = g2o_amd_mod
    po = synth.pose_only(3, 10)
    e = po.edges[0]
    pg = synth.expmap_pose_graph(6, 0)
    x = pg.edges[0]
    # v1 given for the unary types; v1 missing for EdgeSE3Expmap; NULL params for the pose-only types
    opt = mod.SparseOptimizer(0)
    opt.add_vertices(po.vertices[0])
    with pytest.raises(mod.G2OHipError):
        opt.add_edges(synth.EdgeSet(E_MONO, e.v0, e.v0, e.meas, e.info, e.params))
    st = synth.pose_only(3, 10, stereo=True).edges[0]
    with pytest.raises(mod.G2OHipError):
        opt.add_edges(synth.EdgeSet(E_STEREO, st.v0, st.v0, st.meas, st.info, st.params))
    with pytest.raises(mod.G2OHipError):
        opt.add_edges(synth.EdgeSet(E_EXPMAP, x.v0[:2], None, x.meas[:2], x.info[:2], None))
    with pytest.raises(mod.G2OHipError):
        opt.add_edges(synth.EdgeSet(E_MONO, e.v0, None, e.meas, e.info, None))
    with pytest.raises(mod.G2OHipError):
        opt.add_edges(synth.EdgeSet(E_STEREO, st.v0, None, st.meas, st.info, None))
    assert opt.num_edges() == 0
    # an endpoint of the wrong vertex type: a pose-only edge on a VertexSE3, EdgeSE3Expmap to a point
    sp = synth.sphere(4, 4)
    opt = mod.SparseOptimizer(0).add_problem(sp)
    ids = sp.vertices[0].ids[1:4]
    opt.add_edges(synth.EdgeSet(E_MONO, ids, None, e.meas[:3], e.info[:3], e.params[:3]))
    with pytest.raises(mod.G2OHipError) as ei:
        opt.initialize_optimization()
    assert "(-4)" in str(ei.value)
    ba = synth.ba(6, 40, obs_per_point=3, window=4)
    opt = mod.SparseOptimizer(0).add_problem(ba)
    cam, pt = ba.vertices[0].ids, ba.vertices[1].ids
    opt.add_edges(synth.EdgeSet(E_EXPMAP, cam[2:3], pt[0:1], x.meas[:1], x.info[:1], None))
    with pytest.raises(mod.G2OHipError) as ei:
        opt.initialize_optimization()
    assert "(-4)" in str(ei.value)
    # the CGLS solver is BA-only: unary edges, and EdgeSE3Expmap with a message of its own
    opt = mod.SparseOptimizer(0).add_problem(synth.with_pose_only(ba, every=2, per_camera=3))
    opt.set_algorithm("lm_pcg6_3_eigen")
    with pytest.raises(mod.G2OHipError) as ei:
        opt.optimize(1)
    assert "(-4)" in str(ei.value) and "unary" in str(ei.value)
    opt = mod.SparseOptimizer(0).add_problem(ba)
    opt.add_edges(synth.EdgeSet(E_EXPMAP, cam[2:3], cam[4:5], x.meas[:1], x.info[:1], None))
    opt.set_algorithm("lm_pcg6_3_eigen")
    with pytest.raises(mod.G2OHipError) as ei:
        opt.optimize(1)
    assert "(-4)" in str(ei.value) and "EdgeSE3Expmap" in str(ei.value)
