"""Unary edges on the device (G2OHIP_E_*_PRIOR, G2OHIP_E_HOSTJ_UNARY): k_linearize_unary, the one-vertex groups of the
generic slot path, chi2, shards, online updates, .g2o files and the refusals.

Two references: the binary twin of a prior graph run by the CPU oracle (synth.twin_of: EdgeSE2(I, v), EdgeSE3(I, v),
EdgeSE2PointXY(I, l) with a fixed identity vertex I), and tests/unary_ref.py (plain numpy) for what has no twin; the
same graph entered as G2OHIP_E_HOSTJ_UNARY(D) edges with unary_ref's records for the LM trajectories of those.

Tolerances are the project's own, as listed at the top of tests/test_gpu_stereo.py: initial chi2 1e-12, stage level 1e-9
(b, bschur, x) and 1e-11 (Hschur), trajectories 1e-6 relative with identical trial counts, multiplyHessian 1e-8,
marginals at one linearization point 1e-9 (tests/test_gpu_marginals.py), shards against one rank 1e-9 on the state and
1e-6 on chi2, online against a fresh graph 1e-9 (tests/test_online.py).

A prior on a fixed vertex is inactive on the device (sparse_optimizer.cpp:241); the oracle's chi2 counts its twin (an
edge between two fixed vertices, which adds nothing to H or b), so the trajectory cases against the twin hold no such
prior; the stage cases do.
"""
import threading
import uuid

import numpy as np
import pytest

import unary_ref
from g2o_amd import synth
from shard_util import gather_sharded_state

pytestmark = pytest.mark.gpu

RTOL = 1e-6
PRIOR_VT = synth.PRIOR_VERTEX
_CACHE = {}  # problems and reference runs, computed once, shared, left unchanged


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _est_of(opt, prob):
    return {v.vtype: opt.estimates(v.vtype) for v in prob.vertices}


def _one_vertex(etype, marg=0):
    """One free vertex and one prior of the type, non-diagonal information, for SE3 a non-identity offset."""
    rng = np.random.default_rng(etype)
    vt = PRIOR_VT[etype]
    if vt == synth.V_SE3_QUAT:
        est = np.array([[0.3, -1.2, 2.0, 0.1, -0.2, 0.3, 0.9]])
        est[0, 3:] /= np.linalg.norm(est[0, 3:])
    elif vt == synth.V_SE2:
        est = np.array([[0.5, -0.25, 0.7]])
    else:
        est = rng.uniform(-1, 1, (1, synth.EST_DIM[vt]))
    vs = synth.VertexSet(vt, np.array([7], np.int32), est, np.zeros(1, np.int32), np.full(1, marg, np.int32))
    base = synth.Problem("one", [vs], [], unary_ref.V_DIM[vt], 0)
    off = [0.1, -0.2, 0.3, 0.2, 0.1, -0.1, 0.95] if etype == synth.E_SE3_PRIOR else None
    return synth.with_priors(base, etype, every=1, sigma=0.3, seed=etype, offset=off)


# ---------------------------------------------------------------- 1: single-edge pins
@pytest.mark.parametrize("etype", list(PRIOR_VT))
def test_single_edge_pins(g2o_amd_mod, etype):
    prob = _one_vertex(etype)
    g = unary_ref.Graph(prob)
    ref = g.chi2()
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    chi = opt.chi2()
    print(f"prior {etype}: chi2 device {chi:.17g} numpy {ref:.17g} rel {abs(chi - ref) / ref:.2e}")
    assert ref > 0 and abs(chi - ref) <= 1e-12 * ref
    delta = 0.5 * np.sqrt(ref)  # sqrt(e2) > delta: Huber's linear branch, chi2 = rho
    opt.set_robust_kernel(etype, "Huber", delta)
    rho = 2 * np.sqrt(ref) * delta - delta * delta
    assert abs(opt.chi2() - rho) <= 1e-12 * rho
    assert abs(g.chi2(robust={etype: ("Huber", delta)}) - rho) <= 1e-12 * rho


@pytest.mark.parametrize("kind", ["Huber", "PseudoHuber", "Cauchy", "GemanMcClure", "Welsch", "Fair", "Tukey",
                                  "Saturated", "DCS"])
def test_robust_kernels_on_priors(g2o_amd_mod, kind):
    """Every kernel of the factory through g2ohip_set_robust_kernel on a prior type: robust chi2 and the rho'-weighted
    system (stage) against unary_ref."""
    prob = _cached("rk", lambda: synth.with_priors(synth.se2_grid(60), synth.E_SE2_PRIOR, every=2, sigma=0.5, start=1,
                                                   seed=21))
    rob = {synth.E_SE2_PRIOR: (kind, 1.5)}
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    opt.set_robust_kernel(synth.E_SE2_PRIOR, kind, 1.5)
    g = unary_ref.Graph(prob)
    ref = g.chi2(robust=rob)
    assert abs(opt.chi2() - ref) <= 1e-12 * ref
    assert ref < g.chi2()  # the kernel bites
    H, b = g.dense_system(robust=rob)
    _, _, x = unary_ref.solve(H, b, g.npose, 1e-3)
    s = opt.stage(1e-3)
    assert np.linalg.norm(s["b"] - b) <= 1e-9 * np.linalg.norm(b)
    assert np.linalg.norm(s["x"] - x) <= 1e-9 * np.linalg.norm(x)


# ---------------------------------------------------------------- 2: stage level at the kernel's edges
def _stage_against(tag, s, r, schur):
    for k in ("b", "x") + (("bschur",) if schur else ()):
        err = np.linalg.norm(s[k] - r[k]) / np.linalg.norm(r[k])
        print(f"{tag} {k}: {err:.2e}")
        assert err <= 1e-9, (tag, k, err)
    if schur:
        err = np.linalg.norm(s["Hschur"] - r["Hschur"]) / np.linalg.norm(r["Hschur"])
        print(f"{tag} Hschur: {err:.2e}")
        assert err <= 1e-11, (tag, err)


def _numpy_stage(prob, lam, ld=0, binary=None):
    g = unary_ref.Graph(prob)
    H, b = g.dense_system(binary=binary)
    Hs, bs, x = unary_ref.solve(H, b, g.npose, lam, ld)
    return dict(b=b, x=x, Hschur=Hs, bschur=bs)


def _se2_edge_case(ne):
    """se2_grid(300) with ne active SE2 priors, three of them on one vertex (ne >= 4), and one more on the fixed
    vertex 0, which is inactive: the device group holds ne edges."""
    p = synth.with_priors(synth.se2_grid(300), synth.E_SE2_PRIOR, every=1, sigma=[0.2, 0.2, 0.1], seed=31, start=0,
                          count=ne + 1)
    if ne >= 4:
        p.edges[-1].v0[1:4] = p.edges[-1].v0[2]
    return p


@pytest.mark.parametrize("ne", [1, 63, 64, 65, 257])
def test_stage_se2_kernel_edges(g2o_amd_mod, oracle, ne):
    """One partial wave, a full wave, a wave plus one edge, one edge past a 256-thread block. With a second prior type
    behind it (SE2-XY) the second unary group starts at slot 2 * binary + ne of the 9-double arena: an odd offset in
    doubles for the odd ne (wave_copy_out's peel)."""
    lam = 1e-3
    p1 = _se2_edge_case(ne)
    s = g2o_amd_mod.SparseOptimizer(0).add_problem(p1).stage(lam)
    _stage_against(f"se2 ne={ne} numpy", s, _numpy_stage(p1, lam), False)
    _stage_against(f"se2 ne={ne} twin", s, oracle.OracleGraph(synth.twin_of(p1)).stage(lam), False)
    p2 = synth.with_priors(p1, synth.E_SE2_XY_PRIOR, every=41, sigma=0.3, seed=32, start=0)
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(p2)
    _stage_against(f"se2+xy ne={ne} numpy", opt.stage(lam), _numpy_stage(p2, lam), False)
    assert opt.num_edges() == p2.num_edges


def _slam2d_case():
    def make():
        p = synth.with_priors(synth.slam2d(80), synth.E_SE2_PRIOR, every=6, sigma=[0.2, 0.2, 0.1], seed=41)
        p = synth.with_priors(p, synth.E_XY_PRIOR, every=4, sigma=0.3, seed=42)
        # one landmark that has only a prior
        poses, lms = p.vertices
        nid = int(max(poses.ids.max(), lms.ids.max())) + 1
        lms2 = synth.VertexSet(lms.vtype, np.append(lms.ids, nid).astype(np.int32), np.vstack([lms.est, [[3.0, -2.0]]]),
                               np.append(lms.fixed, 0).astype(np.int32), np.append(lms.marginalized, 1).astype(np.int32))
        xy = p.edges[-1]
        xy2 = synth.EdgeSet(xy.etype, np.append(xy.v0, nid).astype(np.int32), None, np.vstack([xy.meas, [[3.1, -2.2]]]),
                            np.concatenate([xy.info, [[[4.0, 1.0], [1.0, 3.0]]]]), None)
        return synth.Problem(p.name + "+lone", [poses, lms2], p.edges[:-1] + [xy2], 3, 2)
    return _cached("slam2d_stage", make)


def test_stage_slam2d_schur(g2o_amd_mod, oracle):
    """BlockSolver_3_2: SE2 priors on poses (one on the fixed pose), XY priors on landmarks, a landmark with only a
    prior."""
    prob, lam = _slam2d_case(), 1e-3
    s = g2o_amd_mod.SparseOptimizer(0).add_problem(prob).stage(lam)
    _stage_against("slam2d numpy", s, _numpy_stage(prob, lam, 2), True)
    _stage_against("slam2d twin", s, oracle.OracleGraph(synth.twin_of(prob)).stage(lam), True)


def _binary_only(prob):
    return synth.Problem(prob.name + "/binary", prob.vertices, [e for e in prob.edges if e.v1 is not None],
                         prob.pose_dim, prob.landmark_dim)


def _oracle_records(oracle, prob, est=None):
    """[e | Ji | Jj] of the problem's first (binary) edge set from the oracle's analytic linearizeOplus."""
    og = oracle.OracleGraph(_binary_only(prob))
    for vt, e in (est or {}).items():
        og.set_estimates(vt, e)
    es = prob.edges[0]
    D = synth.ERR_DIM[es.etype]
    di = {synth.E_SE3_QUAT: 6, synth.E_SE3_PROJECT_XYZ: 3}[es.etype]
    n = len(es.v0)
    return {es.etype: og.edge_payload(np.arange(n), n * D * (1 + di + 6), False)}


SE3_SIGMA = [0.05] * 3 + [0.01] * 3
OFFSET = [0.1, -0.2, 0.3, 0.2, 0.1, -0.1, 0.95]


def test_stage_sphere_se3(g2o_amd_mod, oracle):
    """C1-small with SE3 priors: identity offset against the twin, a non-identity offset against unary_ref."""
    lam = 1e-3
    base = synth.by_name("C1", "small")
    p = synth.with_priors(base, synth.E_SE3_PRIOR, every=3, sigma=SE3_SIGMA, seed=51)
    s = g2o_amd_mod.SparseOptimizer(0).add_problem(p).stage(lam)
    _stage_against("sphere twin", s, oracle.OracleGraph(synth.twin_of(p)).stage(lam), False)
    q = synth.with_priors(base, synth.E_SE3_PRIOR, every=3, sigma=SE3_SIGMA, seed=51, offset=OFFSET)
    s = g2o_amd_mod.SparseOptimizer(0).add_problem(q).stage(lam)
    _stage_against("sphere offset numpy", s, _numpy_stage(q, lam, 0, _oracle_records(oracle, q)), False)


# ---------------------------------------------------------------- 3: LM trajectories against the oracle's twin
def _run(opt, iters):
    n, st = opt.optimize(iters)
    return n, [s.chi2 for s in st], [s.levenbergIterations for s in st], opt.minimal_state()


def _same_trajectory(a, b, tol=RTOL):
    (na, ca, ta, xa), (nb, cb, tb, xb) = a, b
    assert na == nb and ta == tb, (na, nb, ta, tb)
    for x, y in zip(ca, cb):
        assert abs(x - y) <= tol * abs(y), (x, y)
    assert np.linalg.norm(xa - xb) <= tol * np.linalg.norm(xb), np.linalg.norm(xa - xb) / np.linalg.norm(xb)


def _twin_state(oracle, prob, iters, gn):
    """The oracle's run of the twin; its state without the identity vertices (the last ids)."""
    def make():
        twin = synth.twin_of(prob)
        og = oracle.OracleGraph(twin)
        n, st = og.optimize(iters, oracle.make_config(threads=8, gauss_newton=gn))
        extra = sum(unary_ref.V_DIM[v.vtype] for v in twin.vertices[len(prob.vertices):])
        x = og.minimal_state()
        return n, [s.chi2 for s in st], [s.levenbergIterations for s in st], x[:len(x) - extra]
    return _cached(("twin", prob.name, iters, gn), make)


def _traj_cases(name):
    if name == "se2_gauge":  # the priors alone hold the gauge
        return _cached(name, lambda: synth.with_priors(synth.se2_grid(300), synth.E_SE2_PRIOR, every=10,
                                                       sigma=[0.2, 0.2, 0.1], seed=61, drop_fixed=True))
    if name == "sphere":
        return _cached(name, lambda: synth.with_priors(synth.by_name("C1", "small"), synth.E_SE3_PRIOR, every=5,
                                                       sigma=SE3_SIGMA, seed=62, start=1))
    return _cached(name, lambda: synth.with_priors(
        synth.with_priors(synth.slam2d(300), synth.E_SE2_PRIOR, every=7, sigma=[0.2, 0.2, 0.1], seed=63, start=1),
        synth.E_XY_PRIOR, every=5, sigma=0.3, seed=64))


@pytest.mark.parametrize("algo", ["lm_hip_var", "gn_hip_var"])
@pytest.mark.parametrize("name", ["se2_gauge", "sphere", "slam2d"])
def test_trajectory_against_twin(g2o_amd_mod, oracle, name, algo):
    prob = _traj_cases(name)
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    opt.set_algorithm(algo)
    dev = _run(opt, 5)
    print(f"{name} {algo}: chi2 {dev[1]} trials {dev[2]}")
    _same_trajectory(dev, _twin_state(oracle, prob, 5, algo.startswith("gn")))


def test_trajectory_pcg_against_twin(g2o_amd_mod, oracle):
    """The SE2 case under the block-Jacobi PCG (lm_pcg, the registry's variable-block-size name; it has no pcg3_3).
    An iterative solve stops at its residual tolerance, so the twin is run by the oracle under the PCG's restatement
    (oracle/pcg_ref.py, as tests/test_pcg.py does), not under its Cholesky."""
    import pcg_ref
    prob = _traj_cases("se2_gauge")
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    opt.set_algorithm("lm_pcg")
    n, chi, trials, x = _run(opt, 5)
    og = oracle.OracleGraph(synth.twin_of(prob))
    ref = pcg_ref.pcg_lm(og, 5, 3)
    print(f"se2_gauge lm_pcg: chi2 {chi} trials {trials}; restatement {[(r[0], r[1]) for r in ref]}")
    xr = og.minimal_state()[:-3]
    _same_trajectory((n, chi, trials, x), (len(ref), [r[0] for r in ref], [r[1] for r in ref], xr))


def test_bitwise_reproducible(g2o_amd_mod):
    prob = _traj_cases("slam2d")
    runs = [_run(g2o_amd_mod.SparseOptimizer(0).add_problem(prob), 4) for _ in range(2)]
    assert runs[0][1] == runs[1][1]
    assert np.array_equal(runs[0][3], runs[1][3])


# ---------------------------------------------------------------- 4: against the host-J unary path
def _hostj_unary(mod, prob, records=None, robust=None):
    """The graph with its prior sets entered as G2OHIP_E_HOSTJ_UNARY(D) (one prior type per D), unary_ref's records in
    the callback."""
    g = unary_ref.Graph(prob)
    back = {}
    edges = []
    for e in prob.edges:
        if e.v1 is None:
            ht = mod.E_HOSTJ_UNARY(synth.ERR_DIM[e.etype])
            assert ht not in back
            back[ht] = e.etype
            e = synth.EdgeSet(ht, e.v0, None, None, e.info, None)
        edges.append(e)
    opt = mod.SparseOptimizer(0).add_problem(synth.Problem(prob.name + "_hostj", prob.vertices, edges, prob.pose_dim,
                                                           prob.landmark_dim))

    def cb(etype, with_jac):
        return g.prior_payload(back[etype], _est_of(opt, prob))

    opt.set_host_edge_callback(cb)
    for ht, et in back.items():
        if robust and et in robust:
            opt.set_robust_kernel(ht, *robust[et])
    return opt, back


def test_hostj_unary_stage_pin(g2o_amd_mod):
    """The host-J unary path against unary_ref's dense system, before it serves as a reference: SE2-XY priors (D = 2 on
    a 3-vector vertex), one of them on the fixed vertex."""
    prob = _cached("hj_pin", lambda: synth.with_priors(synth.se2_grid(120), synth.E_SE2_XY_PRIOR, every=3, sigma=0.3,
                                                       seed=71))
    opt, back = _hostj_unary(g2o_amd_mod, prob)
    (ht,) = back
    n = len(prob.edges[-1].v0)
    assert g2o_amd_mod.lib().g2ohip_host_payload_len(opt.h, ht) == n * 2 * (1 + 3)
    _stage_against("hostj unary", opt.stage(1e-3), _numpy_stage(prob, 1e-3), False)
    ref = unary_ref.Graph(prob).chi2()
    assert abs(opt.chi2() - ref) <= 1e-12 * ref


def _ba_priors(noisy=False):
    def make():
        kw = dict(cam_rot_noise=0.02, cam_trans_noise=0.05, point_noise=0.1, pixel_noise=200.0, seed=11) if noisy else {}
        base = synth.ba(40, 1500, obs_per_point=8, window=24, **kw)
        return synth.with_priors(base, synth.E_XYZ_PRIOR, every=10, sigma=0.5 if noisy else 0.05, seed=81)
    return _cached(("ba", noisy), make)


@pytest.mark.parametrize("name", ["sphere_offset", "se2_xy", "ba_xyz", "ba_noisy_huber"])
def test_trajectory_against_hostj_unary(g2o_amd_mod, name):
    robust = None
    if name == "sphere_offset":
        prob = _cached(name, lambda: synth.with_priors(synth.by_name("C1", "small"), synth.E_SE3_PRIOR, every=5,
                                                       sigma=SE3_SIGMA, seed=72, offset=OFFSET))
    elif name == "se2_xy":
        prob = _cached(name, lambda: synth.with_priors(synth.se2_grid(300), synth.E_SE2_XY_PRIOR, every=4, sigma=0.3,
                                                       seed=73))
    elif name == "ba_xyz":
        prob = _ba_priors()
    else:
        prob = _ba_priors(noisy=True)
        robust = {synth.E_XYZ_PRIOR: ("Huber", 1.0)}
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    for et, (kind, delta) in (robust or {}).items():
        opt.set_robust_kernel(et, kind, delta)
    dev = _run(opt, 5)
    print(f"{name}: chi2 {dev[1]} trials {dev[2]}")
    ref, _ = _hostj_unary(g2o_amd_mod, prob, robust=robust)
    _same_trajectory(dev, _run(ref, 5))
    if name == "ba_noisy_huber":
        assert any(t > 1 for t in dev[2]), f"no rejected trial: {dev[2]}"


# ---------------------------------------------------------------- 5: BA with priors takes the generic path
def test_ba_with_priors_generic_path(g2o_amd_mod, oracle):
    """A BA graph with XYZ priors is assembled on the slot path (its linearize pass writes the 36 slot doubles per
    observation the fused pass never writes; the unary class runs) and its reduced system is unary_ref's, the BA
    edges' records being the oracle's analytic ones."""
    prob = _ba_priors()
    base = _binary_only(prob)
    plain = g2o_amd_mod.SparseOptimizer(0).add_problem(base)
    plain.stage(1e-3)
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    s = opt.stage(1e-3)
    assert plain.kernel_bytes("linearize_unary") == 0
    nobs = base.num_edges
    assert opt.kernel_bytes("linearize") - plain.kernel_bytes("linearize") >= nobs * 36 * 8.0 - 1500 * 12 * 8.0
    assert opt.kernel_bytes("linearize_unary") == len(prob.edges[-1].v0) * (8 + (3 + 6 + 3 + 9) * 8.0)
    _stage_against("ba+xyz numpy", s, _numpy_stage(prob, 1e-3, 3, _oracle_records(oracle, prob)), True)


# ---------------------------------------------------------------- 6: consumers of Hpp
def test_hpp_consumers_after_optimize(g2o_amd_mod):
    prob = _traj_cases("se2_gauge")
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    n, st = opt.optimize(3)
    assert n == 3 and st[0].numEdges == prob.num_edges == opt.num_edges()  # the batch statistics count the priors
    opt.build_system()
    g = unary_ref.Graph(prob)
    H, _ = g.dense_system(est=_est_of(opt, prob))
    v = np.random.default_rng(0).standard_normal(g.npose)
    y = opt.multiply_hessian(v)
    assert np.linalg.norm(y - H @ v) <= 1e-8 * np.linalg.norm(H @ v)
    pat = [(0, 0), (5, 9), (g.npose // 3 - 1, g.npose // 3 - 1)]
    blocks = opt.compute_marginals(pat)
    Hinv = np.linalg.inv(H)
    num = sum(float(np.sum((B - Hinv[r * 3:r * 3 + 3, c * 3:c * 3 + 3]) ** 2)) for (r, c), B in blocks.items())
    den = sum(float(np.sum(Hinv[r * 3:r * 3 + 3, c * 3:c * 3 + 3] ** 2)) for r, c in pat)
    assert np.sqrt(num / den) <= 1e-9, np.sqrt(num / den)


def test_push_pop_and_save_hessian(g2o_amd_mod, tmp_path):
    prob = _traj_cases("se2_gauge")
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    opt.initialize_optimization()
    c0 = opt.chi2()
    lib = g2o_amd_mod.lib()
    assert lib.g2ohip_push(opt.h) == 0
    opt.optimize(2)
    assert opt.chi2() < c0
    assert lib.g2ohip_pop(opt.h) == 0
    assert opt.chi2() == c0
    opt.build_system()
    assert opt.save_hessian(str(tmp_path / "H.txt"))


# ---------------------------------------------------------------- 7: landmark shards
def _cam_prior_records(cam_est, rows, z):
    """A translation prior on a VertexSE3Expmap (e = t - z; under exp(u) * T, u = (omega, upsilon):
    J = [-[t]x | I])."""
    out = []
    for r, zz in zip(rows, z):
        t = cam_est[r, :3]
        out += [t - zz, np.hstack([-unary_ref._skew(t), np.eye(3)]).ravel()]
    return np.concatenate(out)


def _sharded_problem(mod):
    base = _ba_priors()
    cams = base.vertices[0]
    rows = np.array([5, 30])
    z = cams.est[rows, :3] + np.array([[0.01, -0.02, 0.015], [-0.02, 0.01, 0.0]])
    info = np.array([[[40.0, 5, 0], [5, 30, 2], [0, 2, 50]]] * 2)
    hj = synth.EdgeSet(mod.E_HOSTJ_UNARY(3), cams.ids[rows].copy(), None, None, info, None)
    return synth.Problem(base.name + "+camprior", base.vertices, base.edges + [hj], 6, 3), rows, z


def _sharded_optimizer(mod, prob, rows, z):
    opt = mod.SparseOptimizer(0).add_problem(prob)
    opt.set_host_edge_callback(lambda etype, wj: _cam_prior_records(opt.estimates(synth.V_SE3_EXPMAP), rows, z))
    return opt


def test_two_local_ranks(g2o_amd_mod):
    """XYZ priors on landmarks of both shards, host-J unary priors on two cameras (assembled by rank 0 once): no prior
    counted twice or dropped."""
    prob, rows, z = _sharded_problem(g2o_amd_mod)
    nranks, iters = 2, 4
    key = uuid.uuid4().hex
    opts = [_sharded_optimizer(g2o_amd_mod, prob, rows, z) for _ in range(nranks)]
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
    single = _sharded_optimizer(g2o_amd_mod, prob, rows, z)
    n1, st1 = single.optimize(iters)
    for r in range(nranks):
        n, st = res[r]
        assert n == n1
        for a, b in zip(st, st1):
            assert a.levenbergIterations == b.levenbergIterations
            assert abs(a.chi2 - b.chi2) <= RTOL * b.chi2
    pri = prob.edges[1].v0
    held = [np.isin(pri, o.local_landmark_ids()).sum() for o in opts]
    assert all(h > 0 for h in held) and sum(held) == len(pri), held
    x, _ = gather_sharded_state(prob, opts)
    xs = single.minimal_state()
    assert np.linalg.norm(x - xs) <= 1e-9 * np.linalg.norm(xs)


# ---------------------------------------------------------------- 8: online
def test_online_priors_on_existing_vertices(g2o_amd_mod):
    base = synth.se2_grid(300)
    withp = synth.with_priors(base, synth.E_SE2_PRIOR, every=9, sigma=[0.2, 0.2, 0.1], seed=91, start=1)
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(base)
    opt.optimize(3)
    est = opt.estimates(synth.V_SE2)
    opt.add_edges(withp.edges[-1])
    opt.update_initialization()
    on = _run(opt, 4)
    v = withp.vertices[0]
    fresh_p = synth.Problem("fresh", [synth.VertexSet(v.vtype, v.ids, est, v.fixed, v.marginalized)], withp.edges, 3, 0)
    fr = _run(g2o_amd_mod.SparseOptimizer(0).add_problem(fresh_p), 4)
    _same_trajectory(on, fr, 1e-9)
    assert on[1][0] > 0 and opt.num_edges() == withp.num_edges


# ---------------------------------------------------------------- 9: .g2o files
def _file_graphs():
    a = _slam2d_case()
    a = synth.with_priors(a, synth.E_SE2_XY_PRIOR, every=11, sigma=0.3, seed=95)  # SE2, XY and SE2-XY priors
    sp = synth.sphere(6, 6)
    rng = np.random.default_rng(96)
    pts = synth.VertexSet(synth.V_XYZ, (1000 + np.arange(5)).astype(np.int32), rng.uniform(-1, 1, (5, 3)),
                          np.zeros(5, np.int32), np.ones(5, np.int32))
    b = synth.Problem("sphere+pts", sp.vertices + [pts], sp.edges, 6, 3)
    b = synth.with_priors(b, synth.E_XYZ_PRIOR, every=1, sigma=0.2, seed=97)
    b1 = synth.with_priors(b, synth.E_SE3_PRIOR, every=4, sigma=SE3_SIGMA, seed=98, offset=OFFSET, start=1)
    b2 = synth.with_priors(b, synth.E_SE3_PRIOR, every=4, sigma=SE3_SIGMA, seed=99, start=2)  # identity offset
    e1, e2 = b1.edges[-1], b2.edges[-1]
    ident = np.broadcast_to(unary_ref.IDENT7, (len(e2.v0), 7))
    both = synth.EdgeSet(e1.etype, np.concatenate([e1.v0, e2.v0]), None, np.vstack([e1.meas, e2.meas]),
                         np.concatenate([e1.info, e2.info]), np.vstack([e1.params, ident]))
    return a, synth.Problem("sphere+priors", b.vertices, b.edges + [both], 6, 3)


@pytest.mark.parametrize("which", [0, 1])
def test_g2o_round_trip(g2o_amd_mod, tmp_path, which):
    """Save -> load(unary=True): edge counts and chi2 equal; the file saved again from the loaded graph has the same
    edge and parameter lines (shortest round-trip decimals: every measurement, information and offset value
    bit-exact; the vertex lines go through the state layout and are left to the loader's own tests). Plain load skips
    the prior tags."""
    prob = _file_graphs()[which]
    src = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    p1, p2 = str(tmp_path / "a.g2o"), str(tmp_path / "b.g2o")
    src.save(p1)
    text = open(p1).read()
    for tag in (("EDGE_PRIOR_SE2 ", "EDGE_PRIOR_SE2_XY ", "EDGE_PRIOR_XY ") if which == 0 else
                ("EDGE_POINTXYZ_PRIOR ", "EDGE_SE3_PRIOR ", "PARAMS_SE3OFFSET ")):
        assert tag in text, tag
    if which == 1:
        assert text.count("PARAMS_SE3OFFSET ") == 2  # one line per distinct offset
    back = g2o_amd_mod.SparseOptimizer(0)
    back.load(p1, unary=True)
    assert back.num_edges() == src.num_edges() == prob.num_edges
    assert back.num_vertices() == src.num_vertices()
    c0, c1 = src.chi2(), back.chi2()
    assert abs(c0 - c1) <= 1e-12 * c0, (c0, c1)
    back.save(p2)

    def rest(t):
        return [ln for ln in t.splitlines() if not ln.startswith("VERTEX")]

    assert rest(open(p2).read()) == rest(text)
    plain = g2o_amd_mod.SparseOptimizer(0)
    plain.load(p1)
    assert plain.num_edges() == sum(len(e.v0) for e in prob.edges if e.v1 is not None)


def test_g2o_missing_parameter_fails(g2o_amd_mod, tmp_path):
    path = tmp_path / "bad.g2o"
    info = " ".join("1" if r == c else "0" for r in range(6) for c in range(r, 6))
    path.write_text("PARAMS_SE3OFFSET 1 0 0 0 0 0 0 1\nVERTEX_SE3:QUAT 0 0 0 0 0 0 0 1\nVERTEX_SE3:QUAT 1 1 0 0 0 0 0 1\n"
                    f"EDGE_SE3:QUAT 0 1 1 0 0 0 0 0 1 {info}\nEDGE_SE3_PRIOR 1 2 1 0 0 0 0 0 1 {info}\n")
    with pytest.raises(g2o_amd_mod.G2OHipError) as ei:
        g2o_amd_mod.SparseOptimizer(0).load(str(path), unary=True)
    assert "parameter id 2" in str(ei.value)
    short = tmp_path / "short.g2o"
    short.write_text("VERTEX_SE2 0 0 0 0\nEDGE_PRIOR_SE2 0 1 2 3 1 0 0 1\n")
    with pytest.raises(g2o_amd_mod.G2OHipError) as ei:
        g2o_amd_mod.SparseOptimizer(0).load(str(short), unary=True)
    assert "EDGE_PRIOR_SE2" in str(ei.value)
    ok = g2o_amd_mod.SparseOptimizer(0)
    ok.load(str(path))  # the plain loader skips the tags: one binary edge
    assert ok.num_edges() == 1


# ---------------------------------------------------------------- 10: refusals
def _mono_trace(mod):
    opt = mod.SparseOptimizer(0).add_problem(synth.ba(12, 150, obs_per_point=5, window=8))
    n, st = opt.optimize(2)
    assert n == 2
    return [s.chi2 for s in st], opt.kernel_bytes("linearize")


def test_refusals(g2o_amd_mod, tmp_path):
    mod = g2o_amd_mod
    before = _mono_trace(mod)
    prob = synth.with_priors(synth.se2_grid(40), synth.E_SE2_PRIOR, every=5, seed=3)
    e = prob.edges[-1]
    # v1 given for a unary type; v1 missing for a binary one
    opt = mod.SparseOptimizer(0)
    opt.add_vertices(prob.vertices[0])
    with pytest.raises(mod.G2OHipError):
        opt.add_edges(synth.EdgeSet(e.etype, e.v0, e.v0, e.meas, e.info, None))
    b = prob.edges[0]
    with pytest.raises(mod.G2OHipError):
        opt.add_edges(synth.EdgeSet(b.etype, b.v0, None, b.meas, b.info, None))
    assert opt.num_edges() == 0
    # a prior on a vertex of the wrong type
    opt.add_edges(b)
    opt.add_edges(synth.EdgeSet(synth.E_XY_PRIOR, e.v0, None, e.meas[:, :2], e.info[:, :2, :2], None))
    with pytest.raises(mod.G2OHipError):
        opt.initialize_optimization()
    # the CGLS solver is BA-only
    ba = _ba_priors()
    opt = mod.SparseOptimizer(0).add_problem(ba)
    opt.set_algorithm("lm_pcg6_3_eigen")
    with pytest.raises(mod.G2OHipError) as ei:
        opt.optimize(1)
    assert "(-4)" in str(ei.value) and "unary" in str(ei.value)
    # host-J unary edges are not written (as binary host-J ones are not): the file holds the rest
    hj, _ = _hostj_unary(mod, prob)
    path = str(tmp_path / "hj.g2o")
    hj.save(path)
    back = mod.SparseOptimizer(0)
    back.load(path, unary=True)
    assert back.num_edges() == len(b.v0)
    # a monocular BA graph still takes the fused path and reproduces its chi2 trace bit for bit
    assert _mono_trace(mod) == before
    assert before[1] < 150 * 5 * (36 * 8.0)  # no per-edge slots in its linearize pass
