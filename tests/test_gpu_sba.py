"""The sba types on the device (G2OHIP_V_CAM, G2OHIP_E_PROJECT_P2MC, G2OHIP_E_PROJECT_P2SC): the two families through
k_linearize / k_error and the slot reduction, the vertex's oplus, the 6/3 Schur path, structure-only, levels and
classification, landmark shards, host-Jacobian edges between cameras, .g2o files and the refusals.

Two references: tests/sba_ref.py (plain numpy) for chi2, the stage level, the oplus and structure-only, and the same
graph with its projections entered as G2OHIP_E_HOSTJ(2) / (3) edges whose host callback returns sba_ref's
[e | Ji | Jj] records (the twin) for the trajectories. The twin's stage is pinned against numpy before it serves.

Tolerances are the project's own (tests/test_gpu_slam3d.py): chi2 against numpy 1e-12 relative
(tests/test_sba_host.py measures a float64 floor of at most 5e-15 on these cases, under the 1e-13 that keeps 1e-12),
stage level 1e-9 (b, bschur, x) and 1e-11 (Hschur), trajectories 1e-6 relative with identical trial counts, lm_pcg6_3
tests/test_pcg.py's 1e-5, structure-only 1e-6 on state and chi2 with equal counts, shards against one rank 1e-9 on the
state and 1e-6 on chi2. The oplus is held to 64 eps per entry relative to max(1, |value|): a quaternion product, one
square root and one division per entry, each good to an ulp or two (the bound tests/test_gpu_oplus.py gives the
cases without a transcendental function).
"""
import threading
import uuid

import numpy as np
import pytest

import sba_ref
import structure_only_ref
import unary_ref
from g2o_amd import synth
from sba_ref import KINDS, MONO, STEREO, TAGS
from shard_util import gather_sharded_state

pytestmark = pytest.mark.gpu

RTOL = 1e-6
PCG_RTOL = 1e-5
EPS = float(np.finfo(np.float64).eps)
HUBER = 3.0
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
    """The graph with each sba edge set entered as an E_HOSTJ(D) set between the same vertices, sba_ref's records in
    the callback; an EdgeSBACam set (E_HOSTJ(6)) is served by the same callback. robust: {sba type: (kind, delta)}."""
    g = sba_ref.Graph(prob)
    tw, _ = sba_ref.hostj_problem(prob)
    back = {sba_ref.HOSTJ[t]: t for t in KINDS}
    back[sba_ref.E_SBACAM] = sba_ref.E_SBACAM
    opt = mod.SparseOptimizer(0).add_problem(tw)
    opt.set_host_edge_callback(lambda etype, with_jac: g.payload(back[etype], _est_of(opt, prob)))
    for et, (kind, delta) in (robust or {}).items():
        opt.set_robust_kernel(sba_ref.HOSTJ[et], kind, delta)
    for et, lv in (levels or {}).items():
        opt.set_edge_levels(sba_ref.HOSTJ[et], lv)
    return opt


def _with_tie_callback(opt, prob):
    """A device graph that also holds the EdgeSBACam tie (edge_case): its records from sba_ref."""
    g = sba_ref.Graph(prob)
    opt.set_host_edge_callback(lambda etype, with_jac: g.payload(etype, _est_of(opt, prob)))
    return opt


def _stage_against(tag, s, r):
    for k in ("b", "x", "bschur"):
        err = np.linalg.norm(s[k] - r[k]) / np.linalg.norm(r[k])
        print(f"{tag} {k}: {err:.2e}")
        assert err <= 1e-9, (tag, k, err)
    err = np.linalg.norm(s["Hschur"] - r["Hschur"]) / np.linalg.norm(r["Hschur"])
    print(f"{tag} Hschur: {err:.2e}")
    assert err <= 1e-11, (tag, err)


def _numpy_stage(prob, lam, robust=None, est=None):
    """lam None: LM's own first lambda, computeLambdaInit's tau * max diag(H) with tau = 1e-5. A monocular point seen
    from one camera has no depth information (Hll of rank 2): at a lambda far under the scale of H the stage level then
    answers rounding with 1e-7 of x in numpy itself, at LM's lambda with 1e-13 (measured by perturbing H by eps)."""
    g = sba_ref.Graph(prob)
    H, b = g.dense_system(est=est, robust=robust)
    if lam is None:
        lam = 1e-5 * float(np.max(np.diag(H)))
    Hs, bs, x = unary_ref.solve(H, b, g.npose, lam, 3)
    return dict(b=b, x=x, Hschur=Hs, bschur=bs, np=g.npose, n=g.n, lam=lam)


def _run(opt, iters, algo=None, lambda_init=0.0):
    if algo:
        opt.set_algorithm(algo)
    n, st = opt.optimize(iters, lambda_init=lambda_init)
    return n, [s.chi2 for s in st], [s.levenbergIterations for s in st], opt.minimal_state()


def _same_trajectory(a, b, tol=RTOL):
    (na, ca, ta, xa), (nb, cb, tb, xb) = a, b
    assert na == nb and ta == tb, (na, nb, ta, tb)
    for x, y in zip(ca, cb):
        assert abs(x - y) <= tol * abs(y), (x, y)
    assert np.linalg.norm(xa - xb) <= tol * np.linalg.norm(xb), np.linalg.norm(xa - xb) / np.linalg.norm(xb)


# ---------------------------------------------------------------- 1: single-edge pins
@pytest.mark.parametrize("etype", KINDS)
def test_single_edge_pins(g2o_amd_mod, etype):
    prob = sba_ref.one_edge(etype)
    g = sba_ref.Graph(prob)
    ref = g.chi2()
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    chi = opt.chi2()
    print(f"edge type {etype}: chi2 device {chi:.17g} numpy {ref:.17g} rel {abs(chi - ref) / ref:.2e}")
    assert ref > 0 and abs(chi - ref) <= 1e-12 * ref
    delta = 0.5 * np.sqrt(ref)  # sqrt(e2) > delta: Huber's linear branch, chi2 = rho
    opt.set_robust_kernel(etype, "Huber", delta)
    rho = 2 * np.sqrt(ref) * delta - delta * delta
    assert abs(opt.chi2() - rho) <= 1e-12 * rho
    assert abs(g.chi2(robust={etype: ("Huber", delta)}) - rho) <= 1e-12 * rho
    # the sign of the error: the single edge's b = -J^T Omega e
    opt2 = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    r = _numpy_stage(prob, None)
    s = opt2.stage(r["lam"])
    assert np.linalg.norm(s["b"] - r["b"]) <= 1e-9 * np.linalg.norm(r["b"])


# ---------------------------------------------------------------- 2: stage level at the kernel's edges
@pytest.mark.parametrize("ne", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("etype", KINDS)
def test_stage_kernel_edges(g2o_amd_mod, etype, ne):
    """A partial wave, a full wave, a wave plus one edge, one edge past a 256-thread block; the host-J twin of the same
    graph beside the device."""
    prob = sba_ref.edge_case(etype, ne)
    for tag, opt in (("device", _with_tie_callback(_device(g2o_amd_mod, prob), prob)), ("twin", _twin(g2o_amd_mod, prob))):
        # numpy at the handle's own estimates (the quaternions as normalised on entry): the chain's records are central
        # differences, which turn a last-bit difference of the input into 1e-10 of the Jacobian
        est = _est_of(opt, prob)
        r = _numpy_stage(prob, None, est=est)
        ref = sba_ref.Graph(prob).chi2(est=est)
        s = opt.stage(r["lam"])
        assert s["ok"] == 1 and (s["n"], s["np"]) == (r["n"], r["np"]), (s["n"], s["np"], r["n"], r["np"])
        _stage_against(f"{tag} type {etype} ne={ne}", s, r)
        chi = opt.chi2()
        assert abs(chi - ref) <= 1e-12 * ref, (tag, chi, ref)
    assert r["np"] == 66  # the 11 free cameras, NOLM among them


# ---------------------------------------------------------------- 3: oplus
@pytest.mark.parametrize("ncam", [1, 255, 256, 257])
def test_oplus(g2o_amd_mod, ncam):
    """update() on ncam free cameras (and one fixed) against sba_ref.oplus: random increments, |v|^2 = 0.99, a zero
    update, the |v|^2 > 1 vertex (rotation NaN, translation moved, the others unaffected), push / pop."""
    rng = np.random.default_rng(40 + ncam)
    n = ncam + 1
    cam = np.zeros((n, 12))
    cam[:, :3] = rng.standard_normal((n, 3))
    cam[:, 3:7] = rng.standard_normal((n, 4))
    cam[:, 7:] = [500.0, 480.0, 320.0, 240.0, 0.1]
    cam = sba_ref.normalized(cam)
    fixed = np.zeros(n, np.int32)
    fixed[n // 2] = 1
    pt = np.array([[0.1, 0.2, 50.0]])
    cams = synth.VertexSet(synth.V_CAM, np.arange(n, dtype=np.int32), cam, fixed, np.zeros(n, np.int32))
    pts = synth.VertexSet(synth.V_XYZ, np.array([10000], np.int32), pt, np.zeros(1, np.int32), np.ones(1, np.int32))
    es = synth.EdgeSet(MONO, np.full(n, 10000, np.int32), np.arange(n, dtype=np.int32), np.zeros((n, 2)),
                       np.broadcast_to(np.eye(2), (n, 2, 2)).copy(), None)
    prob = synth.Problem(f"oplus{ncam}", [cams, pts], [es], 6, 3)
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    opt.initialize_optimization()
    opt.build_structure()
    assert opt.vector_size() == 6 * ncam + 3
    free = np.nonzero(fixed == 0)[0]  # hessian order: free poses by id, then the point
    u = 0.1 * rng.standard_normal((ncam, 6))
    u[0, 3:] *= np.sqrt(0.99) / np.linalg.norm(u[0, 3:])
    if ncam > 1:
        u[1] = 0.0
    nan_row = 2 if ncam > 2 else None
    if nan_row is not None:
        u[nan_row, 3:] = [0.8, 0.6, 0.3]
    x = np.concatenate([u.ravel(), [0.5, -0.25, 1.0]])
    given = cam
    cam = opt.estimates(synth.V_CAM)  # unit quaternions with w >= 0 come back as given, to the rounding of 1 / |q|
    assert np.max(np.abs(cam - given)) <= 2 * EPS and np.array_equal(cam[:, :3], given[:, :3])
    opt.push()
    opt.update(x)
    got, gpt = opt.estimates(synth.V_CAM), opt.estimates(synth.V_XYZ)
    assert np.array_equal(got[n // 2], cam[n // 2])  # the fixed camera
    assert np.array_equal(gpt, pt + [0.5, -0.25, 1.0])
    worst = 0.0
    for k, r in enumerate(free):
        ref = sba_ref.oplus(cam[r], u[k], np.longdouble).astype(np.float64)
        if k == nan_row:
            assert np.all(np.isnan(got[r, 3:7])) and np.all(np.isnan(ref[3:7]))
            assert np.array_equal(got[r, :3], cam[r, :3] + u[k, :3]) and np.array_equal(got[r, 7:], cam[r, 7:])
            continue
        err = np.max(np.abs(got[r] - ref) / np.maximum(1.0, np.abs(ref)))
        worst = max(worst, err)
        assert abs(np.linalg.norm(got[r, 3:7]) - 1) <= 4 * EPS
    print(f"{ncam} cameras: oplus worst entry {worst:.2e} ({worst / EPS:.1f} eps)")
    assert worst <= 64 * EPS
    if ncam > 1:
        assert np.array_equal(got[free[1], :3], cam[free[1], :3]) and np.array_equal(got[free[1], 7:], cam[free[1], 7:])
        assert np.max(np.abs(got[free[1], 3:7] - cam[free[1], 3:7])) <= 2 * EPS  # the zero update
    opt.pop()
    assert np.array_equal(opt.estimates(synth.V_CAM), cam) and np.array_equal(opt.estimates(synth.V_XYZ), pt)


def test_estimate_normalised_on_entry(g2o_amd_mod):
    """A quaternion of length 2 with w < 0 comes back unit with w >= 0; minimal_state is x y z qx qy qz."""
    prob = sba_ref.one_edge(MONO)
    cam = prob.vertices[0].est.copy()
    raw = cam.copy()
    raw[0, 3:7] *= -2.0
    prob = synth.Problem("raw", [synth.VertexSet(synth.V_CAM, prob.vertices[0].ids, raw, prob.vertices[0].fixed,
                                                 prob.vertices[0].marginalized), prob.vertices[1]], prob.edges, 6, 3)
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    got = opt.estimates(synth.V_CAM)
    assert np.allclose(got, cam, rtol=0, atol=4 * EPS) and got[0, 6] > 0
    assert np.array_equal(opt.minimal_state()[:6], got[0, :6])
    opt.set_estimates(synth.V_CAM, raw)
    assert np.allclose(opt.estimates(synth.V_CAM), cam, rtol=0, atol=4 * EPS)


# ---------------------------------------------------------------- 4: trajectories
def _traj(stereo):
    return _cached(("traj", stereo), lambda: synth.sba(12, 300, obs_per_point=4, stereo=stereo))


def _twin_run(mod, stereo, algo, robust=False, iters=4):
    et = STEREO if stereo else MONO
    return _cached(("twinrun", stereo, algo, robust, iters),
                   lambda: _run(_twin(mod, _traj(stereo), {et: ("Huber", HUBER)} if robust else None), iters, algo))


def test_twin_stage_pin(g2o_amd_mod):
    for stereo in (False, True):
        prob = _traj(stereo)
        r = _numpy_stage(prob, None)
        _stage_against(f"twin stereo={stereo}", _twin(g2o_amd_mod, prob).stage(r["lam"]), r)
        _stage_against(f"device stereo={stereo}", _device(g2o_amd_mod, prob).stage(r["lam"]), r)


@pytest.mark.parametrize("algo", ["lm_hip_fix6_3", "lm_hip_var", "gn_hip_fix6_3", "dl_hip_fix6_3"])
@pytest.mark.parametrize("stereo", [False, True])
def test_trajectory_against_twin(g2o_amd_mod, stereo, algo):
    dev = _run(_device(g2o_amd_mod, _traj(stereo)), 4, algo)
    print(f"{algo} stereo={stereo}: chi2 {dev[1]} trials {dev[2]}")
    _same_trajectory(dev, _twin_run(g2o_amd_mod, stereo, algo))
    assert dev[1][-1] < dev[1][0]


def test_trajectory_huber(g2o_amd_mod):
    prob = _traj(True)
    dev = _run(_device(g2o_amd_mod, prob, {STEREO: ("Huber", HUBER)}), 4, "lm_hip_fix6_3")
    print(f"Huber: chi2 {dev[1]} trials {dev[2]}")
    _same_trajectory(dev, _twin_run(g2o_amd_mod, True, "lm_hip_fix6_3", robust=True))
    plain = _twin_run(g2o_amd_mod, True, "lm_hip_fix6_3")
    assert abs(dev[1][0] - plain[1][0]) > 1e-3 * plain[1][0]  # the kernel is at work: another trajectory


def _mixed():
    """The scene seen by both vocabularies: VertexCam cameras 0..11 with P2MC edges on the even observations and
    VertexSE3Expmap cameras 1000..1011 (ba()'s estimates) with EdgeSE3ProjectXYZ on the odd ones, the same points."""
    def make():
        sb, ba = synth.sba(12, 300, obs_per_point=4), synth.ba(12, 300, obs_per_point=4)
        cams_e = ba.vertices[0]
        cams_e = synth.VertexSet(cams_e.vtype, cams_e.ids + 1000, cams_e.est, cams_e.fixed, cams_e.marginalized)
        es, eb = sb.edges[0], ba.edges[0]
        ev, od = np.arange(0, len(es.v0), 2), np.arange(1, len(es.v0), 2)
        e1 = synth.EdgeSet(MONO, es.v0[ev], es.v1[ev], es.meas[ev], es.info[ev], None)
        e2 = synth.EdgeSet(synth.E_SE3_PROJECT_XYZ, eb.v0[od], eb.v1[od] + 1000, eb.meas[od], eb.info[od], eb.params[od])
        return synth.Problem("sba+ba", [sb.vertices[0], cams_e, sb.vertices[1]], [e1, e2], 6, 3)
    return _cached("mixed", make)


def test_mixed_with_expmap_cameras(g2o_amd_mod):
    prob = _mixed()
    r = _numpy_stage(prob, None)
    _stage_against("mixed device", _device(g2o_amd_mod, prob).stage(r["lam"]), r)
    dev = _run(_device(g2o_amd_mod, prob), 4, "lm_hip_fix6_3")
    ref = _run(_twin(g2o_amd_mod, prob), 4, "lm_hip_fix6_3")
    print(f"mixed: chi2 {dev[1]} trials {dev[2]}")
    _same_trajectory(dev, ref)
    assert dev[1][-1] < dev[1][0]


def test_lm_pcg6_3_against_twin(g2o_amd_mod):
    dev = _run(_device(g2o_amd_mod, _traj(False)), 4, "lm_pcg6_3")
    print(f"lm_pcg6_3: chi2 {dev[1]} trials {dev[2]}")
    _same_trajectory(dev, _twin_run(g2o_amd_mod, False, "lm_pcg6_3"), PCG_RTOL)


# ---------------------------------------------------------------- 5: structure-only
@pytest.mark.parametrize("prior", [False, True])
@pytest.mark.parametrize("etype", KINDS)
def test_structure_only_tracks(g2o_amd_mod, etype, prior):
    """Track lengths 1, 7, 8, 9 and 65 (eight lanes per landmark), alone and beside an EdgeXYZPrior."""
    prob = sba_ref.tracks_problem(etype, prior=prior)
    s = sba_ref.Structure(prob)
    ref_est, results = s.calc(10)
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    cams_before = opt.estimates(synth.V_CAM)
    counts = opt.structure_only(iterations=10)
    print(f"type {etype} prior={prior}: device {counts} reference {structure_only_ref.counts(results)}")
    assert counts == structure_only_ref.counts(results)
    got, ref = opt.estimates(synth.V_XYZ), ref_est[synth.V_XYZ]
    worst = np.max(np.linalg.norm(got - ref, axis=1) / np.linalg.norm(ref, axis=1))
    print(f"worst point {worst:.2e}")
    assert worst <= RTOL
    assert np.array_equal(opt.estimates(synth.V_CAM), cams_before)  # the cameras are left bit for bit
    chi, chi_ref = opt.chi2(), s.graph_chi2(ref_est)
    assert abs(chi - chi_ref) <= RTOL * chi_ref, (chi, chi_ref)


@pytest.mark.parametrize("stereo", [False, True])
def test_sba_demo_sequence(g2o_amd_mod, stereo):
    """structure_only(10), then LM on the same handle: bit for bit the same calls on a fresh handle."""
    prob = synth.sba(8, 120, obs_per_point=4, stereo=stereo, point_noise=0.2)
    out = []
    for _ in range(2):
        opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
        c0 = opt.chi2()
        counts = opt.structure_only(iterations=10)
        c1 = opt.chi2()
        opt.set_algorithm("lm_hip_fix6_3")
        n, st = opt.optimize(3)
        out.append((counts, c1, [x.chi2 for x in st], opt.minimal_state()))
        assert counts["accepted"] > 0 and c1 < c0 and st[-1].chi2 < c1
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1] and out[0][2] == out[1][2]
    assert np.array_equal(out[0][3], out[1][3])


# ---------------------------------------------------------------- 6: levels, per-edge chi2, classification
@pytest.mark.parametrize("etype", KINDS)
def test_levels_chi2_classify(g2o_amd_mod, etype):
    prob = _traj(etype == STEREO)
    g = sba_ref.Graph(prob)
    ref = g.edge_chi2(etype)
    opt = _device(g2o_amd_mod, prob)
    opt.initialize_optimization()
    chi = opt.edge_chi2(etype)
    assert np.max(np.abs(chi - ref) / ref) <= 1e-12
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
    dev, twr = _run(opt, 3, "lm_hip_fix6_3"), _run(tw, 3, "lm_hip_fix6_3")
    _same_trajectory(dev, twr)
    assert dev[1][0] < float(np.sum(ref))  # the outliers are out of the system


# ---------------------------------------------------------------- 7: landmark shards
def test_two_local_ranks(g2o_amd_mod):
    prob = _traj(False)
    nranks, iters = 2, 4
    key = uuid.uuid4().hex
    opts = [_device(g2o_amd_mod, prob) for _ in range(nranks)]
    for r, o in enumerate(opts):
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
    n1, st1 = single.optimize(iters)
    for r in range(nranks):
        n, st = res[r]
        assert n == n1
        for a, b in zip(st, st1):
            assert a.levenbergIterations == b.levenbergIterations
            assert abs(a.chi2 - b.chi2) <= RTOL * b.chi2
    held = [len(o.local_landmark_ids()) for o in opts]
    assert all(h > 0 for h in held) and sum(held) == 300, held
    x, _ = gather_sharded_state(prob, opts)
    xs = single.minimal_state()
    assert np.linalg.norm(x - xs) <= 1e-9 * np.linalg.norm(xs)


# ---------------------------------------------------------------- 8: host-J edges between cameras
def test_hostj_chain_on_cameras(g2o_amd_mod):
    """An EdgeSBACam chain (E_HOSTJ(6)) between VertexCam vertices only, the records numpy central differences:
    lm_hip_fix6_6 lowers chi2 every iteration and ends at numpy's value for the end state."""
    rng = np.random.default_rng(8)
    n = 10
    truth = np.zeros((n, 12))
    truth[:, 0] = 0.5 * np.arange(n)
    truth[:, 3:6] = 0.05 * rng.standard_normal((n, 3))
    truth[:, 6] = 1.0
    truth[:, 7:] = [500.0, 480.0, 320.0, 240.0, 0.1]
    truth = sba_ref.normalized(truth)
    a, b = np.arange(n - 1), np.arange(1, n)
    meas = []
    for i, j in zip(a, b):
        t1, q1 = sba_ref._inv(truth[i, :3], truth[i, 3:7])
        td, qd = sba_ref._mul(t1, q1, truth[j, :3], truth[j, 3:7])
        meas.append(np.concatenate([td, qd]))
    est = truth.copy()
    est[1:, :3] += 0.05 * rng.standard_normal((n - 1, 3))
    est[1:, 3:7] += 0.02 * rng.standard_normal((n - 1, 4))
    est = sba_ref.normalized(est)
    fixed = np.zeros(n, np.int32)
    fixed[0] = 1
    cams = synth.VertexSet(synth.V_CAM, np.arange(n, dtype=np.int32), est, fixed, np.zeros(n, np.int32))
    es = synth.EdgeSet(sba_ref.E_SBACAM, a.astype(np.int32), b.astype(np.int32), np.array(meas),
                       np.broadcast_to(np.diag([100.0] * 3 + [400.0] * 3), (n - 1, 6, 6)).copy(), None)
    prob = synth.Problem("sbacam_chain", [cams], [es], 6, 0)
    g = sba_ref.Graph(prob)
    dev_es = synth.EdgeSet(es.etype, es.v0, es.v1, None, es.info, None)
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(synth.Problem("chain", [cams], [dev_es], 6, 0))
    opt.set_host_edge_callback(lambda etype, with_jac: g.payload(etype, _est_of(opt, prob)))
    c0 = g.chi2()
    n_it, chis, trials, _ = _run(opt, 5, "lm_hip_fix6_6")
    print(f"EdgeSBACam chain: chi2 {c0:.6g} -> {chis}")
    assert n_it >= 1 and chis[0] < c0 and all(y <= x for x, y in zip(chis, chis[1:])) and chis[-1] < 1e-3 * c0
    end = g.chi2(est=_est_of(opt, prob))
    assert abs(chis[-1] - end) <= 1e-9 * max(end, c0 * 1e-12), (chis[-1], end)


# ---------------------------------------------------------------- 9: .g2o files
@pytest.mark.parametrize("etype", KINDS)
def test_g2o_round_trip(g2o_amd_mod, tmp_path, etype):
    prob = synth.sba(6, 40, obs_per_point=3, stereo=etype == STEREO)
    src = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    p1 = str(tmp_path / "a.g2o")
    src.save(p1)
    lines = open(p1).read().splitlines()
    tags = [ln.split()[0] for ln in lines]
    ne = len(prob.edges[0].v0)
    assert tags.count("VERTEX_CAM") == 6 and tags.count("VERTEX_XYZ") == 40 and tags.count(TAGS[etype]) == ne
    assert tags.count("FIX") == (1 if etype == STEREO else 2)
    first = next(ln for ln in lines if ln.startswith(TAGS[etype])).split()
    assert len(first) == 3 + synth.ERR_DIM[etype]  # the measurement alone
    assert len(next(ln for ln in lines if ln.startswith("VERTEX_CAM")).split()) == 14
    back = g2o_amd_mod.SparseOptimizer(0)
    back.load(p1, sba=True)
    assert back.num_edges() == src.num_edges() == ne and back.num_vertices() == src.num_vertices() == 46
    ids = np.zeros(6, np.int32)
    assert g2o_amd_mod.lib().g2ohip_get_estimates(back.h, synth.V_CAM, None, g2o_amd_mod._p(ids)) == 6
    assert list(ids) == list(range(6))
    # the file holds shortest round-trip decimals: every value comes back bit for bit, and the loader's normalisation
    # of the (unit) quaternion moves it by the rounding of 1 / |q| at most
    assert np.array_equal(back.estimates(synth.V_XYZ), src.estimates(synth.V_XYZ))
    cb, cs = back.estimates(synth.V_CAM), src.estimates(synth.V_CAM)
    assert np.array_equal(cb[:, [0, 1, 2, 7, 8, 9, 10, 11]], cs[:, [0, 1, 2, 7, 8, 9, 10, 11]])
    assert np.max(np.abs(cb - cs)) <= 2 * EPS
    assert abs(back.chi2() - src.chi2()) <= 1e-12 * src.chi2()
    s0, s1 = src.stage(1e-3), back.stage(1e-3)
    assert s0["nl"] == s1["nl"] == 120 and s0["np"] == s1["np"]
    assert np.linalg.norm(s0["x"] - s1["x"]) <= 1e-9 * np.linalg.norm(s0["x"])
    plain = g2o_amd_mod.SparseOptimizer(0)
    plain.load(p1)  # without the flag the sba tags are skipped
    assert plain.num_vertices() == 40 and plain.num_edges() == 0


def test_g2o_vertex_cam_lengths(g2o_amd_mod, tmp_path):
    body = "VERTEX_XYZ 1 0.1 0.2 4\nEDGE_PROJECT_P2MC 1 0 330 250\n"
    p7 = tmp_path / "seven.g2o"
    p7.write_text("VERTEX_CAM 0 0.1 0.2 0.3 0 0 0 2\n" + body)
    opt = g2o_amd_mod.SparseOptimizer(0)
    opt.load(str(p7), sba=True)
    assert np.array_equal(opt.estimates(synth.V_CAM), [[0.1, 0.2, 0.3, 0, 0, 0, 1, 300, 300, 320, 320, 0.1]])
    assert opt.num_edges() == 1
    ref = sba_ref.error(MONO, [0.1, 0.2, 4], opt.estimates(synth.V_CAM)[0], [330, 250])
    assert abs(opt.chi2() - ref @ ref) <= 1e-12 * (ref @ ref)  # identity information
    p9 = tmp_path / "nine.g2o"
    p9.write_text("VERTEX_CAM 0 0.1 0.2 0.3 0 0 0 1 300 300\n" + body)
    with pytest.raises(g2o_amd_mod.G2OHipError) as ei:
        g2o_amd_mod.SparseOptimizer(0).load(str(p9), sba=True)
    assert "VERTEX_CAM" in str(ei.value) and "VERTEX_CAM" in g2o_amd_mod.last_error()
    pw = tmp_path / "wrong.g2o"  # the camera end names a VERTEX_SE3:EXPMAP
    pw.write_text("VERTEX_SE3:EXPMAP 0 0 0 0 0 0 0 1\n" + body)
    with pytest.raises(g2o_amd_mod.G2OHipError) as ei:
        g2o_amd_mod.SparseOptimizer(0).load(str(pw), sba=True)
    assert "EDGE_PROJECT_P2MC" in str(ei.value)


def test_save_refuses_non_identity_information(g2o_amd_mod, tmp_path):
    prob = sba_ref.one_edge(STEREO)  # a full information matrix
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    path = tmp_path / "no.g2o"
    with pytest.raises(g2o_amd_mod.G2OHipError) as ei:
        opt.save(str(path))
    assert f"({ERR_UNSUPPORTED})" in str(ei.value) and "information" in g2o_amd_mod.last_error()
    assert not path.exists()


# ---------------------------------------------------------------- 10: refusals
def test_refusals(g2o_amd_mod):
    prob = sba_ref.one_edge(MONO)
    es = prob.edges[0]
    opt = g2o_amd_mod.SparseOptimizer(0)
    for vs in prob.vertices:
        opt.add_vertices(vs)
    with pytest.raises(g2o_amd_mod.G2OHipError) as ei:  # params must be NULL
        opt.add_edges(synth.EdgeSet(MONO, es.v0, es.v1, es.meas, es.info, np.array([[260.0, 250.0, 160.0, 120.0]])))
    assert f"({ERR_ARG})" in str(ei.value) and opt.num_edges() == 0
    # v1 a VertexSE3Expmap
    cam_e = synth.VertexSet(synth.V_SE3_EXPMAP, np.array([3], np.int32), np.array([[0, 0, 0, 0, 0, 0, 1.0]]),
                            np.zeros(1, np.int32), np.zeros(1, np.int32))
    wrong = g2o_amd_mod.SparseOptimizer(0).add_problem(synth.Problem("wrong", [cam_e, prob.vertices[1]], [es], 6, 3))
    with pytest.raises(g2o_amd_mod.G2OHipError) as ei:
        wrong.initialize_optimization()
    assert f"({ERR_UNSUPPORTED})" in str(ei.value) and "vertex type 1" in str(ei.value)
    # the matrix-free CGLS
    dev = _device(g2o_amd_mod, _traj(False))
    dev.set_algorithm("lm_pcg6_3_eigen")
    with pytest.raises(g2o_amd_mod.G2OHipError) as ei:
        dev.optimize(1)
    assert f"({ERR_UNSUPPORTED})" in str(ei.value) and "sba" in str(ei.value) and "lm_pcg6_3" in g2o_amd_mod.last_error()
    dev.set_algorithm("lm_hip_fix6_3")  # the graph is still usable
    n, st = dev.optimize(1)
    assert n == 1 and np.isfinite(st[0].chi2)
    # the wrong estimate length through the wrapper
    short = synth.VertexSet(synth.V_CAM, np.array([0], np.int32), np.array([[0, 0, 0, 0, 0, 0, 1.0]]),
                            np.zeros(1, np.int32), np.zeros(1, np.int32))
    with pytest.raises(g2o_amd_mod.G2OHipError) as ei:
        g2o_amd_mod.SparseOptimizer(0).add_vertices(short)
    assert "12" in str(ei.value)
