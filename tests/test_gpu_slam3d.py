"""The slam3d landmark edges on the device (G2OHIP_E_SE3_XYZ, _DEPTH, _DISPARITY): the three families through
k_linearize / k_error and the slot reduction, the 6/3 Schur path, mixed graphs, the iterative solver, landmark shards,
the solver-mode consumers, .g2o files and the refusals.

Two references: tests/slam3d_ref.py (plain numpy: the three edges, EdgeSE3 and, through tests/unary_ref.py, the priors
and the dense normal equations) for chi2 and the stage level, and the same graph with its landmark edges entered as
G2OHIP_E_HOSTJ(3) edges whose host callback returns slam3d_ref's [e | Ji | Jj] records (the twin) for the LM
trajectories and the solver-mode consumers. The twin's stage is pinned against numpy before it serves.

Tolerances are the project's own, as listed at the top of tests/test_gpu_stereo.py and tests/test_gpu_unary.py: initial
chi2 1e-12 (tests/test_slam3d_host.py shows that float64 holds these cases' chi2 to ~1e-14), stage level 1e-9 (b,
bschur, x) and 1e-11 (Hschur), trajectories 1e-6 relative with identical trial counts, multiplyHessian 1e-8, marginals
1e-9, shards against one rank 1e-9 on the state and 1e-6 on chi2, file round trips exact on ids and counts.
"""
import threading
import uuid

import numpy as np
import pytest

import slam3d_ref
import unary_ref
from g2o_amd import synth
from shard_util import gather_sharded_state
from slam3d_ref import KINDS, OFFSET, TAGS

pytestmark = pytest.mark.gpu

RTOL = 1e-6
CAM = [260.0, 250.0, 160.0, 120.0]
OFFSET2 = [-0.05, 0.1, 0.2, -0.1, 0.2, 0.1, 0.96]
SE3_SIGMA = [0.05] * 3 + [0.01] * 3
HUBER = 3.0
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


def _stage_against(tag, s, r, schur):
    for k in ("b", "x") + (("bschur",) if schur else ()):
        err = np.linalg.norm(s[k] - r[k]) / np.linalg.norm(r[k])
        print(f"{tag} {k}: {err:.2e}")
        assert err <= 1e-9, (tag, k, err)
    if schur:
        err = np.linalg.norm(s["Hschur"] - r["Hschur"]) / np.linalg.norm(r["Hschur"])
        print(f"{tag} Hschur: {err:.2e}")
        assert err <= 1e-11, (tag, err)


def _numpy_stage(prob, lam, ld=3, robust=None):
    g = slam3d_ref.Graph(prob)
    H, b = g.dense_system(robust=robust)
    Hs, bs, x = unary_ref.solve(H, b, g.npose, lam, ld)
    return dict(b=b, x=x, Hschur=Hs, bschur=bs, np=g.npose, n=g.n)


# ---------------------------------------------------------------- 1: single-edge pins
@pytest.mark.parametrize("etype", KINDS)
def test_single_edge_pins(g2o_amd_mod, etype):
    prob = slam3d_ref.one_edge(etype)
    g = slam3d_ref.Graph(prob)
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


# ---------------------------------------------------------------- 2: stage level at the kernel's edges
NOLM = 5  # the free pose that no landmark edge touches


def _edge_case(etype, ne, distinct=False, null_params=False):
    """12 poses with their odometry and exactly ne landmark edges of one type, picked from slam3d_landmarks(12, 200)
    (three observations per point): three edges on one (pose, point) pair (one shared off-diagonal block), a point seen
    only from the fixed pose 0 (an Hll block, no Hpl block), a point seen once, then whole observations of other points;
    no edge touches pose NOLM. ne = 1 holds the once-seen point's edge alone. distinct: a different offset (and camera)
    on every edge; otherwise every edge carries the same record."""
    base = synth.slam3d_landmarks(12, 200, kind=etype, offset=None if null_params else OFFSET, camera=CAM,
                                  obs_per_point=3, seed=31 + etype)
    poses, pts = base.vertices
    odo, obs = base.edges
    # the generator chains the odometry into the initial poses, so the odometry residuals are zero to rounding; with few
    # landmark edges b would then be little more than rounding (and bschur the cancellation residue of one observation).
    # Move the free poses off the chain: b and bschur are then set by odometry residuals of ordinary size.
    rng = np.random.default_rng(1000 + ne)
    est = poses.est.copy()
    est[1:, :3] += 0.05 * rng.standard_normal((11, 3))
    est[1:, 3:] += 0.02 * rng.standard_normal((11, 4))
    est[:, 3:] /= np.linalg.norm(est[:, 3:], axis=1, keepdims=True)
    poses = synth.VertexSet(poses.vtype, poses.ids, est, poses.fixed, poses.marginalized)
    usable = (obs.v0 != NOLM) & (obs.v0 != 0)
    by_fixed = np.unique(obs.v1[obs.v0 == 0])
    free_pts = [p for p in np.unique(obs.v1) if p not in by_fixed and usable[obs.v1 == p].all()]
    p_once, p_tri, p_fix = free_pts[0], free_pts[1], by_fixed[0]
    r_once = np.nonzero(obs.v1 == p_once)[0][0]
    r_tri = np.nonzero(obs.v1 == p_tri)[0][0]
    r_fix = np.nonzero((obs.v1 == p_fix) & (obs.v0 == 0))[0][0]
    rest = np.nonzero((obs.v0 != NOLM) & ~np.isin(obs.v1, [p_once, p_tri, p_fix]))[0]
    sel = np.array([r_once] if ne == 1 else [r_tri, r_tri, r_tri, r_fix, r_once] + list(rest[:ne - 5]))
    assert len(sel) == ne
    meas = obs.meas[sel].copy()
    if ne > 1:  # the three edges of one pair differ in their measurement
        meas[1] *= 1.01
        meas[2] *= 0.99
    par = None if obs.params is None else obs.params[sel].copy()
    if distinct:
        par[:, :3] += 0.02 * rng.standard_normal((ne, 3))
        par[:, 3:7] += 0.02 * rng.standard_normal((ne, 4))
        par[:, 3:7] /= np.linalg.norm(par[:, 3:7], axis=1, keepdims=True)
        par[:, 7:] *= 1.0 + 0.02 * rng.standard_normal((ne, par.shape[1] - 7))
    es = synth.EdgeSet(etype, obs.v0[sel].copy(), obs.v1[sel].copy(), meas, obs.info[sel].copy(), par)
    assert NOLM not in es.v0 and (ne == 1 or (es.v0 == 0).any())
    return synth.Problem(f"{base.name}/ne{ne}{'d' if distinct else ''}", [poses, pts], [odo, es], 6, 3)


@pytest.mark.parametrize("ne", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("etype", KINDS)
def test_stage_kernel_edges(g2o_amd_mod, etype, ne):
    """A partial wave, a full wave, a wave plus one edge, one edge past a 256-thread block; one shared parameter record
    (the uniform bit) and per-edge distinct offsets / cameras."""
    lam = 1e-3
    lin = {}
    for distinct in (False, True):
        prob = _edge_case(etype, ne, distinct)
        opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
        s = opt.stage(lam)
        r = _numpy_stage(prob, lam)
        assert s["ok"] == 1 and (s["n"], s["np"]) == (r["n"], r["np"]) == (r["n"], 66)  # NOLM is a free pose block
        _stage_against(f"type {etype} ne={ne} distinct={distinct}", s, r, True)
        ref = slam3d_ref.Graph(prob).chi2()
        assert abs(opt.chi2() - ref) <= 1e-12 * ref
        lin[distinct] = opt.kernel_bytes("linearize")
    # the shared record is read once: the accounting of the linearize pass differs by the per-edge records
    rec = 12 if etype == synth.E_SE3_XYZ else 16
    assert lin[True] - lin[False] == (ne * rec * 8.0 if ne > 1 else 0.0), lin


@pytest.mark.parametrize("ne", [1, 63, 64, 65, 257])
def test_stage_xyz_null_params(g2o_amd_mod, ne):
    """G2OHIP_E_SE3_XYZ with params = NULL against the identity offset."""
    prob = _edge_case(synth.E_SE3_XYZ, ne, null_params=True)
    assert prob.edges[1].params is None
    s = g2o_amd_mod.SparseOptimizer(0).add_problem(prob).stage(1e-3)
    _stage_against(f"xyz NULL ne={ne}", s, _numpy_stage(prob, 1e-3), True)
    es = prob.edges[1]
    ident = synth.EdgeSet(es.etype, es.v0, es.v1, es.meas, es.info, np.broadcast_to(unary_ref.IDENT7, (ne, 7)).copy())
    s2 = g2o_amd_mod.SparseOptimizer(0).add_problem(
        synth.Problem("ident", prob.vertices, [prob.edges[0], ident], 6, 3)).stage(1e-3)
    assert np.array_equal(s["b"], s2["b"]) and np.array_equal(s["x"], s2["x"])


# ---------------------------------------------------------------- 3: mixed graph
def _mixed_problem(fixed_points=False):
    def make():
        base = synth.slam3d_landmarks(12, 120, kind=KINDS, offset=OFFSET, camera=CAM, seed=33)
        p = synth.with_priors(base, synth.E_SE3_PRIOR, every=4, sigma=SE3_SIGMA, seed=34, offset=OFFSET2, start=1)
        p = synth.with_priors(p, synth.E_XYZ_PRIOR, every=5, sigma=0.2, seed=35)
        if fixed_points:
            poses, pts = p.vertices
            pts = synth.VertexSet(pts.vtype, pts.ids, pts.est, np.ones_like(pts.fixed), pts.marginalized)
            p = synth.Problem(p.name + "/fixedpts", [poses, pts], p.edges, 6, 0)
        return p
    return _cached(("mixed", fixed_points), make)


@pytest.mark.parametrize("fixed_points", [False, True])
def test_stage_mixed_graph(g2o_amd_mod, fixed_points):
    """All three types on the same points beside SE3 odometry, SE3 priors (with an offset) and XYZ priors, Huber on the
    depth edges; marginalized, and with every point fixed (no Schur complement: pose blocks only, the XYZ priors
    inactive)."""
    prob, lam = _mixed_problem(fixed_points), 1e-3
    robust = {synth.E_SE3_XYZ_DEPTH: ("Huber", HUBER)}
    assert [e.etype for e in prob.edges] == [synth.E_SE3_QUAT, *KINDS, synth.E_SE3_PRIOR, synth.E_XYZ_PRIOR]
    opt = _device(g2o_amd_mod, prob, robust)
    s = opt.stage(lam)
    r = _numpy_stage(prob, lam, 0 if fixed_points else 3, robust)
    assert (s["n"], s["np"]) == (r["n"], r["np"]) and (s["nl"] == 0) == fixed_points
    _stage_against(f"mixed fixed_points={fixed_points}", s, r, not fixed_points)
    g = slam3d_ref.Graph(prob)
    ref = g.chi2(robust=robust)
    assert abs(opt.chi2() - ref) <= 1e-12 * ref and ref < g.chi2()


# ---------------------------------------------------------------- 4: the host-J twin
def _twin(mod, prob, robust=None):
    """The graph with its landmark edge sets entered as one G2OHIP_E_HOSTJ(3) set (in their order), slam3d_ref's
    records in the callback. robust: one (kind, delta) for the set."""
    g = slam3d_ref.Graph(prob)
    lm = [e for e in prob.edges if e.etype in KINDS]
    hj = synth.EdgeSet(mod.E_HOSTJ(3), np.concatenate([e.v0 for e in lm]), np.concatenate([e.v1 for e in lm]), None,
                       np.concatenate([e.info for e in lm]), None)
    edges = [e for e in prob.edges if e.etype not in KINDS] + [hj]
    opt = mod.SparseOptimizer(0).add_problem(synth.Problem(prob.name + "_hostj", prob.vertices, edges, prob.pose_dim,
                                                           prob.landmark_dim))
    opt.set_host_edge_callback(lambda etype, with_jac: g.payload(KINDS, _est_of(opt, prob)))
    if robust:
        opt.set_robust_kernel(mod.E_HOSTJ(3), *robust)
    return opt


def _traj(noisy=False):
    return _cached(("traj", noisy), lambda: slam3d_ref.traj_problem(noisy))


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


# the noisy case starts LM at a user lambda of 1e-3: from computeLambdaInit's value every trial of its first five
# iterations is accepted; from 1e-3 the fourth iteration rejects several
NOISY_LAMBDA = 1e-3


def _twin_run(mod, noisy, algo, iters=5):
    robust = ("Huber", HUBER) if noisy else None
    return _cached(("twinrun", noisy, algo, iters),
                   lambda: _run(_twin(mod, _traj(noisy), robust), iters, algo, NOISY_LAMBDA if noisy else 0.0))


def test_twin_stage_pin(g2o_amd_mod):
    """The host-J twin against numpy before it serves as a reference, and the device beside it: 40 poses, 600 points,
    the three types on the same observations."""
    prob, lam = _traj(), 1e-3
    r = _cached("traj_numpy", lambda: (_numpy_stage(prob, lam), slam3d_ref.Graph(prob).chi2()))
    tw = _twin(g2o_amd_mod, prob)
    assert g2o_amd_mod.lib().g2ohip_host_payload_len(tw.h, g2o_amd_mod.E_HOSTJ(3)) == sum(len(e.v0) for e in prob.edges if e.etype in KINDS) * 3 * (1 + 6 + 3)
    _stage_against("twin", tw.stage(lam), r[0], True)
    assert abs(tw.chi2() - r[1]) <= 1e-12 * r[1]
    dev = _device(g2o_amd_mod, prob)
    _stage_against("device", dev.stage(lam), r[0], True)
    chi = dev.chi2()
    print(f"traj: chi2 device {chi:.17g} numpy {r[1]:.17g} rel {abs(chi - r[1]) / r[1]:.2e}")
    assert abs(chi - r[1]) <= 1e-12 * r[1]


@pytest.mark.parametrize("algo,noisy", [("lm_hip_fix6_3", False), ("gn_hip_fix6_3", False), ("lm_hip_fix6_3", True)])
def test_trajectory_against_twin(g2o_amd_mod, algo, noisy):
    prob = _traj(noisy)
    robust = {k: ("Huber", HUBER) for k in KINDS} if noisy else None
    dev = _run(_device(g2o_amd_mod, prob, robust), 5, algo, NOISY_LAMBDA if noisy else 0.0)
    print(f"{algo} noisy={noisy}: chi2 {dev[1]} trials {dev[2]}")
    ref = _twin_run(g2o_amd_mod, noisy, algo)
    _same_trajectory(dev, ref)
    assert dev[1][-1] < dev[1][0]
    if noisy:  # a rejected LM trial in both runs
        assert any(t > 1 for t in dev[2]) and any(t > 1 for t in ref[2]), (dev[2], ref[2])


# ---------------------------------------------------------------- 5: the iterative solver
def test_lm_pcg6_3_against_twin(g2o_amd_mod):
    dev = _run(_device(g2o_amd_mod, _traj()), 5, "lm_pcg6_3")
    print(f"lm_pcg6_3: chi2 {dev[1]} trials {dev[2]}")
    _same_trajectory(dev, _twin_run(g2o_amd_mod, False, "lm_pcg6_3"))


def test_lm_pcg6_3_eigen_refuses(g2o_amd_mod):
    opt = _device(g2o_amd_mod, _traj())
    opt.set_algorithm("lm_pcg6_3_eigen")
    with pytest.raises(g2o_amd_mod.G2OHipError) as ei:
        opt.optimize(1)
    assert "(-4)" in str(ei.value) and "slam3d" in str(ei.value) and "lm_pcg6_3" in g2o_amd_mod.last_error()
    opt.set_algorithm("lm_hip_fix6_3")  # the graph is still usable
    n, st = opt.optimize(1)
    assert n == 1 and np.isfinite(st[0].chi2)


# ---------------------------------------------------------------- 6: reproducibility
def test_bitwise_reproducible(g2o_amd_mod):
    runs = [_run(_device(g2o_amd_mod, _traj()), 4) for _ in range(2)]
    assert runs[0][1] == runs[1][1]
    assert np.array_equal(runs[0][3], runs[1][3])


# ---------------------------------------------------------------- 7: solver-mode consumers
def test_solver_mode_consumers_against_twin(g2o_amd_mod, tmp_path):
    prob = _traj()
    dev, tw = _device(g2o_amd_mod, prob), _twin(g2o_amd_mod, prob)
    outs = []
    for tag, opt in (("dev", dev), ("twin", tw)):
        n, _ = opt.optimize(3)
        assert n == 3
        opt.build_system()
        npose = opt.block_dims()[2] * 6
        v = np.random.default_rng(0).standard_normal(npose)
        pat = [(0, 0), (3, 7), (npose // 6 - 1, npose // 6 - 1)]
        path = tmp_path / f"H_{tag}.txt"
        assert opt.save_hessian(str(path))
        outs.append((opt.multiply_hessian(v), opt.compute_marginals(pat), path.read_text().splitlines()))
    (ya, ma, ta), (yb, mb, tb) = outs
    assert np.linalg.norm(ya - yb) <= 1e-8 * np.linalg.norm(yb)
    num = sum(float(np.sum((ma[k] - mb[k]) ** 2)) for k in mb)
    den = sum(float(np.sum(mb[k] ** 2)) for k in mb)
    assert np.sqrt(num / den) <= 1e-9, np.sqrt(num / den)

    def pattern(lines):  # the header without the file's name, then (row, column) of every entry
        return [ln for ln in lines if ln.startswith("#") and "name" not in ln] + \
               [" ".join(ln.split()[:2]) for ln in lines if ln and not ln.startswith("#")]

    assert pattern(ta) == pattern(tb) and len(ta) > 39 * 36
    # push / pop around an optimization
    lib = g2o_amd_mod.lib()
    c0 = dev.chi2()
    assert lib.g2ohip_push(dev.h) == 0
    dev.optimize(1)
    assert lib.g2ohip_pop(dev.h) == 0
    assert dev.chi2() == c0


# ---------------------------------------------------------------- 8: landmark shards
def test_two_local_ranks(g2o_amd_mod):
    prob = _traj()
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
    assert all(h > 0 for h in held) and sum(held) == 600, held
    x, _ = gather_sharded_state(prob, opts)
    xs = single.minimal_state()
    assert np.linalg.norm(x - xs) <= 1e-9 * np.linalg.norm(xs)


# ---------------------------------------------------------------- 9: .g2o files
def _file_problem():
    """The mixed graph with a second camera on half of the disparity edges and a second offset on some XYZ edges."""
    p = _mixed_problem()
    edges = []
    for e in p.edges:
        if e.etype == synth.E_SE3_XYZ_DISPARITY:
            par = e.params.copy()
            par[::2, 7:] = [300.0, 310.0, 150.0, 110.0]
            e = synth.EdgeSet(e.etype, e.v0, e.v1, e.meas, e.info, par)
        elif e.etype == synth.E_SE3_XYZ:
            par = e.params.copy()
            par[::3] = _unit(OFFSET2)
            e = synth.EdgeSet(e.etype, e.v0, e.v1, e.meas, e.info, par)
        edges.append(e)
    return synth.Problem(p.name + "/file", p.vertices, edges, 6, 3)


def _unit(off):
    off = np.asarray(off, np.float64).copy()
    off[3:7] /= np.linalg.norm(off[3:7])
    return off


def test_g2o_round_trip(g2o_amd_mod, tmp_path):
    """save -> load(unary=True, slam3d=True): counts and chi2 equal; the file saved again from the loaded graph has the
    same parameter, FIX and edge lines (shortest round-trip decimals: ids, parameter records, measurements and
    information bit-exact). Parameters come first, one line per distinct record, in one id space."""
    prob = _file_problem()
    src = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    p1, p2 = str(tmp_path / "a.g2o"), str(tmp_path / "b.g2o")
    src.save(p1)
    lines = open(p1).read().splitlines()
    tags = [ln.split()[0] for ln in lines]
    npar = sum(t.startswith("PARAMS_") for t in tags)
    assert all(t.startswith("PARAMS_") for t in tags[:npar])  # parameters first
    # offsets: OFFSET2 (the priors' and a third of the XYZ edges', one record) and OFFSET; cameras: (OFFSET, CAM) and
    # (OFFSET, the second camera)
    assert tags.count("PARAMS_CAMERACALIB") == 2 and tags.count("PARAMS_SE3OFFSET") == 2
    ids = [int(ln.split()[1]) for ln in lines[:npar]]
    assert len(set(ids)) == npar  # one id space
    assert tags.count("VERTEX_TRACKXYZ") == 120 and tags.count("VERTEX_XYZ") == 0
    for et in KINDS:
        assert tags.count(TAGS[et]) == len(prob.edges[1].v0)
    back = g2o_amd_mod.SparseOptimizer(0)
    back.load(p1, unary=True, slam3d=True)
    assert back.num_edges() == src.num_edges() == prob.num_edges
    assert back.num_vertices() == src.num_vertices() == prob.num_vertices
    c0, c1 = src.chi2(), back.chi2()
    assert abs(c0 - c1) <= 1e-9 * c0, (c0, c1)
    for vt in (synth.V_SE3_QUAT, synth.V_XYZ):
        assert np.allclose(back.estimates(vt), src.estimates(vt), rtol=0, atol=1e-9)
    s0, s1 = src.stage(1e-3), back.stage(1e-3)  # the points came back marginalized
    assert s0["nl"] == s1["nl"] == 360 and np.linalg.norm(s0["x"] - s1["x"]) <= 1e-9 * np.linalg.norm(s0["x"])
    back.save(p2)

    def rest(path):
        return [ln for ln in open(path).read().splitlines() if not ln.startswith("VERTEX")]

    assert rest(p2) == rest(p1)
    # the plain loader and the unary-only one skip the slam3d tags: poses, odometry (and priors on poses) only
    plain = g2o_amd_mod.SparseOptimizer(0)
    plain.load(p1)
    assert plain.num_vertices() == 12 and plain.num_edges() == 11
    un = g2o_amd_mod.SparseOptimizer(0)
    with pytest.raises(g2o_amd_mod.G2OHipError):  # its EDGE_POINTXYZ_PRIOR lines name VERTEX_TRACKXYZ points it skipped
        un.load(p1, unary=True)


HAND = """# a hand-written file in the reference's field order
PARAMS_SE3OFFSET 5 0.1 -0.2 0.3 0 0 0.19866933079506122 0.98006657784124163
PARAMS_CAMERACALIB 9 0.1 -0.2 0.3 0 0 0.19866933079506122 0.98006657784124163 260 250 160 120
VERTEX_SE3:QUAT 0 0 0 0 0 0 0 1
VERTEX_SE3:QUAT 1 1 0.1 -0.1 0 0.0998334166468282 0 0.9950041652780258
FIX 0
VERTEX_TRACKXYZ 2 0.5 -0.4 4
VERTEX_TRACKXYZ 3 -0.6 0.3 5
EDGE_SE3:QUAT 0 1 1.02 0.09 -0.1 0 0.1 0 0.99498743710662 100 0 0 0 0 0 100 0 0 0 0 100 0 0 0 400 0 0 400 0 400
EDGE_SE3_TRACKXYZ 0 2 5 0.3 -0.9 3.6 50 5 0 40 2 30
EDGE_SE3_TRACKXYZ 1 2 5 -0.1 -0.6 3.9 50 5 0 40 2 30
EDGE_PROJECT_DEPTH 1 2 9 150 80 3.9 1 0.1 0 1 0.2 100
EDGE_PROJECT_DEPTH 0 3 9 95 190 4.8 1 0.1 0 1 0.2 100
EDGE_PROJECT_DISPARITY 1 3 9 60 170 0.21 1 0.1 0 1 0.2 2500
EDGE_PROJECT_DISPARITY 0 2 9 175 60 0.27 1 0.1 0 1 0.2 2500
"""


def _hand_problem():
    off = np.array([0.1, -0.2, 0.3, 0, 0, 0.19866933079506122, 0.98006657784124163])
    cam = np.concatenate([off, CAM])
    poses = synth.VertexSet(synth.V_SE3_QUAT, np.array([0, 1], np.int32),
                            np.array([[0, 0, 0, 0, 0, 0, 1.0], [1, 0.1, -0.1, 0, 0.0998334166468282, 0, 0.9950041652780258]]),
                            np.array([1, 0], np.int32), np.zeros(2, np.int32))
    pts = synth.VertexSet(synth.V_XYZ, np.array([2, 3], np.int32), np.array([[0.5, -0.4, 4.0], [-0.6, 0.3, 5.0]]),
                          np.zeros(2, np.int32), np.ones(2, np.int32))
    i6 = np.diag([100.0] * 3 + [400.0] * 3)
    odo = synth.EdgeSet(synth.E_SE3_QUAT, np.array([0], np.int32), np.array([1], np.int32),
                        np.array([[1.02, 0.09, -0.1, 0, 0.1, 0, 0.99498743710662]]), i6[None])

    def sym(a, b, c, d, e, f):
        return np.array([[a, b, c], [b, d, e], [c, e, f]], np.float64)

    ix, ic, idp = sym(50, 5, 0, 40, 2, 30), sym(1, 0.1, 0, 1, 0.2, 100), sym(1, 0.1, 0, 1, 0.2, 2500)
    xyz = synth.EdgeSet(synth.E_SE3_XYZ, np.array([0, 1], np.int32), np.array([2, 2], np.int32),
                        np.array([[0.3, -0.9, 3.6], [-0.1, -0.6, 3.9]]), np.array([ix, ix]), np.array([off, off]))
    dep = synth.EdgeSet(synth.E_SE3_XYZ_DEPTH, np.array([1, 0], np.int32), np.array([2, 3], np.int32),
                        np.array([[150, 80, 3.9], [95, 190, 4.8]]), np.array([ic, ic]), np.array([cam, cam]))
    dis = synth.EdgeSet(synth.E_SE3_XYZ_DISPARITY, np.array([1, 0], np.int32), np.array([3, 2], np.int32),
                        np.array([[60, 170, 0.21], [175, 60, 0.27]]), np.array([idp, idp]), np.array([cam, cam]))
    return synth.Problem("hand", [poses, pts], [odo, xyz, dep, dis], 6, 3)


def test_g2o_hand_written_file(g2o_amd_mod, tmp_path):
    """A file in the reference's field order (v0 v1 paramId m0 m1 m2, the six upper-triangle information values)
    against the same graph built through add_edges."""
    path = tmp_path / "hand.g2o"
    path.write_text(HAND)
    a = g2o_amd_mod.SparseOptimizer(0)
    a.load(str(path), slam3d=True)
    prob = _hand_problem()
    b = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    assert a.num_vertices() == b.num_vertices() == 4 and a.num_edges() == b.num_edges() == 7
    ca, cb, ref = a.chi2(), b.chi2(), slam3d_ref.Graph(prob).chi2()
    print(f"hand-written file: chi2 loaded {ca:.17g} built {cb:.17g} numpy {ref:.17g}")
    assert abs(ca - cb) <= 1e-12 * cb and abs(cb - ref) <= 1e-12 * ref
    sa, sb = a.stage(1e-3), b.stage(1e-3)
    assert (sa["np"], sa["nl"]) == (sb["np"], sb["nl"]) == (6, 6)
    _stage_against("hand", sa, sb, True)
    _stage_against("hand numpy", sb, _numpy_stage(prob, 1e-3), True)
    # marginalize = False: the points are pose-class blocks of another size, which a BlockSolver refuses
    c = g2o_amd_mod.SparseOptimizer(0)
    c.load(str(path), marginalize_xyz=False, slam3d=True)
    with pytest.raises(g2o_amd_mod.G2OHipError) as ei:
        c.initialize_optimization()
    assert "(-4)" in str(ei.value)


def test_g2o_missing_parameter_fails(g2o_amd_mod, tmp_path):
    mod = g2o_amd_mod
    bad = tmp_path / "bad.g2o"
    bad.write_text(HAND.replace("PARAMS_CAMERACALIB 9 ", "PARAMS_CAMERACALIB 8 "))
    with pytest.raises(mod.G2OHipError) as ei:
        mod.SparseOptimizer(0).load(str(bad), slam3d=True)
    assert "parameter id 9" in str(ei.value) and "PARAMS_CAMERACALIB" in str(ei.value)
    kind = tmp_path / "kind.g2o"  # an offset where a camera is needed, and the other way round
    kind.write_text(HAND.replace("EDGE_PROJECT_DEPTH 1 2 9 ", "EDGE_PROJECT_DEPTH 1 2 5 "))
    with pytest.raises(mod.G2OHipError) as ei:
        mod.SparseOptimizer(0).load(str(kind), slam3d=True)
    assert "parameter id 5" in str(ei.value)
    kind.write_text(HAND.replace("EDGE_SE3_TRACKXYZ 0 2 5 ", "EDGE_SE3_TRACKXYZ 0 2 9 "))
    with pytest.raises(mod.G2OHipError) as ei:
        mod.SparseOptimizer(0).load(str(kind), slam3d=True)
    assert "parameter id 9" in str(ei.value) and "PARAMS_SE3OFFSET" in str(ei.value)
    short = tmp_path / "short.g2o"
    short.write_text(HAND.replace(" 1 0.1 0 1 0.2 2500\n", " 1 0.1 0 1\n", 1))
    with pytest.raises(mod.G2OHipError) as ei:
        mod.SparseOptimizer(0).load(str(short), slam3d=True)
    assert "EDGE_PROJECT_DISPARITY" in str(ei.value)
    # the plain loader still skips the tags: the two poses and the odometry edge, as before
    ok = mod.SparseOptimizer(0)
    ok.load(str(bad))
    assert ok.num_vertices() == 2 and ok.num_edges() == 1


# ---------------------------------------------------------------- 10: refusals
def test_refusals(g2o_amd_mod):
    mod = g2o_amd_mod
    prob = _hand_problem()
    poses, pts = prob.vertices
    odo, xyz, dep, dis = prob.edges

    def fresh():
        opt = mod.SparseOptimizer(0)
        opt.add_vertices(poses)
        opt.add_vertices(pts)
        opt.add_edges(odo)
        return opt

    def works(opt):
        for e in (xyz, dep, dis):
            opt.add_edges(e)
        n, st = opt.optimize(2)
        assert n == 2 and np.isfinite(st[-1].chi2) and opt.num_edges() == 7

    # NULL params for Depth / Disparity, NULL v1: G2OHIP_ERR_ARG, nothing added, the graph usable
    opt = fresh()
    for e in (dep, dis):
        with pytest.raises(mod.G2OHipError) as ei:
            opt.add_edges(synth.EdgeSet(e.etype, e.v0, e.v1, e.meas, e.info, None))
        assert "(-1)" in str(ei.value)
    for e in (xyz, dep, dis):
        with pytest.raises(mod.G2OHipError) as ei:
            opt.add_edges(synth.EdgeSet(e.etype, e.v0, None, e.meas, e.info, e.params))
        assert "(-1)" in str(ei.value)
    assert opt.num_edges() == 1
    works(opt)
    # a wrong vertex type on either end: G2OHIP_ERR_UNSUPPORTED from initialize, with the vertex in the message
    for e in (xyz, dep, dis):
        for v0, v1 in ((e.v1, e.v1), (e.v0, e.v0)):  # a point as the pose; a pose as the point
            opt = fresh()
            opt.add_edges(synth.EdgeSet(e.etype, v0, v1, e.meas, e.info, e.params))
            with pytest.raises(mod.G2OHipError) as ei:
                opt.initialize_optimization()
            assert "(-4)" in str(ei.value) and f"edge type {e.etype} on vertex" in str(ei.value)
            works(fresh())
    # unmarginalized points: pose-class blocks of dimension 3 beside the 6-dimensional poses
    free = synth.VertexSet(pts.vtype, pts.ids, pts.est, pts.fixed, np.zeros_like(pts.marginalized))
    for algo in ("lm_hip_var", "lm_hip_fix6_6"):
        opt = mod.SparseOptimizer(0)
        opt.add_vertices(poses)
        opt.add_vertices(free)
        for e in prob.edges:
            opt.add_edges(e)
        opt.set_algorithm(algo)
        with pytest.raises(mod.G2OHipError) as ei:
            opt.optimize(1)
        assert "(-4)" in str(ei.value)
        works(fresh())
