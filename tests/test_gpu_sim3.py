"""Sim3 pose graphs on the device (G2OHIP_V_SIM3, G2OHIP_E_SIM3, g2ohip_set_sim3_fix_scale, 7 x 7 blocks): FamilySim3
through k_linearize_sim3 / k_error and the slot reduction, both states of the shared information record, the four
branches of Sim3::log and of the exponential, oplus, the dimension-7 vertex reduction, factorisation, symv, dogleg and
marginals, host-Jacobian edges of dimension 7 and on Sim3 vertices, levels and classification, .g2o files and the
refusals.

Two references: tests/sim3_ref.py (plain numpy) for chi2, the stage level, oplus and marginals, and the same graph with
the edge set entered as G2OHIP_E_HOSTJ(7) edges whose host callback returns sim3_ref's [e | Ji | Jj] records (the twin)
for the trajectories. The twin's stage is pinned against numpy before it serves.

Tolerances are the project's own: chi2 against numpy 1e-12 relative (tests/test_sim3_host.py measures a float64 floor of
3e-15 in total and 8e-14 per edge on these cases, under the 1e-13 that keeps 1e-12), stage level 1e-9 (b, x) and 1e-11
(H), trajectories 1e-6 relative with identical iteration and trial counts, linear residual 1e-10
(tests/test_gpu_parity.py), marginals tests/test_gpu_marginals.py's 1e-9, .g2o round trip 1e-12.
"""
import os

import numpy as np
import pytest

import sim3_ref as S
from g2o_amd import synth

pytestmark = pytest.mark.gpu

RTOL = 1e-6
EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble
V, E, HJ = S.V_SIM3, S.E_SIM3, S.HOSTJ
ERR_ARG, ERR_UNSUPPORTED = -1, -4
_CACHE = {}  # problems and reference runs, computed once, shared, left unchanged


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _est_of(opt, prob):
    return {v.vtype: opt.estimates(v.vtype) for v in prob.vertices}


def _device(mod, prob, robust=None, fix_scale=False):
    opt = mod.SparseOptimizer(0).add_problem(prob)
    if robust:
        opt.set_robust_kernel(E, *robust)
    if fix_scale:
        opt.set_sim3_fix_scale(True)
    return opt


def _twin(mod, prob, robust=None, fix_scale=False, levels=None):
    """The graph with the EdgeSim3 set entered as an E_HOSTJ(7) set between the same vertices, sim3_ref's records in
    the callback."""
    g = S.Graph(prob, fix_scale)
    opt = mod.SparseOptimizer(0).add_problem(S.hostj_problem(prob))
    opt.set_host_edge_callback(lambda etype, with_jac: g.payload(_est_of(opt, prob)))
    if robust:
        opt.set_robust_kernel(HJ, *robust)
    if fix_scale:
        opt.set_sim3_fix_scale(True)
    if levels is not None:
        opt.set_edge_levels(HJ, levels)
    return opt


def _rk(robust):
    return {E: robust} if robust else None


def _stage_against(tag, s, r):
    assert s["ok"] == 1 and (s["n"], s["np"]) == (r["n"], r["np"]), (tag, s["n"], s["np"], r["n"], r["np"])
    for k in ("b", "x", "bschur"):
        err = np.linalg.norm(s[k] - r[k]) / np.linalg.norm(r[k])
        print(f"{tag} {k}: {err:.2e}")
        assert err <= 1e-9, (tag, k, err)
    err = np.linalg.norm(s["Hschur"] - r["Hschur"]) / np.linalg.norm(r["Hschur"])
    print(f"{tag} H: {err:.2e}")
    assert err <= 1e-11, (tag, err)


def _stage_both(mod, tag, prob, robust=None, fix_scale=False):
    """The device and the twin, each against numpy at the handle's own estimates (quaternions as normalised on entry)."""
    for who, opt in (("device", _device(mod, prob, robust, fix_scale)), ("twin", _twin(mod, prob, robust, fix_scale))):
        est = _est_of(opt, prob)
        r = S.numpy_stage(prob, None, _rk(robust), est, fix_scale)
        _stage_against(f"{who} {tag}", opt.stage(r["lam"]), r)
        ref = S.Graph(prob, fix_scale).chi2(est=est, robust=_rk(robust))
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


def _graph():
    return _cached("graph", synth.sim3_pose_graph)


def _twin_run(mod, algo, robust=None, iters=4):
    return _cached(("twinrun", algo, bool(robust), iters), lambda: _run(_twin(mod, _graph(), robust), iters, algo))


# ---------------------------------------------------------------- 1: single-edge pins
def test_single_edge_pins(g2o_amd_mod):
    prob = S.one_edge()
    opt = _device(g2o_amd_mod, prob)
    est = _est_of(opt, prob)
    g = S.Graph(prob)
    ref = g.chi2(est=est)
    chi = opt.chi2()
    print(f"chi2 device {chi:.17g} numpy {ref:.17g} rel {abs(chi - ref) / ref:.2e}")
    assert ref > 0 and abs(chi - ref) <= 1e-12 * ref
    delta = 0.5 * np.sqrt(ref)  # sqrt(e2) > delta: Huber's linear branch, chi2 = rho
    opt.set_robust_kernel(E, "Huber", delta)
    rho = 2 * np.sqrt(ref) * delta - delta * delta
    assert abs(opt.chi2() - rho) <= 1e-12 * rho
    assert abs(g.chi2(est=est, robust={E: ("Huber", delta)}) - rho) <= 1e-12 * rho
    # the sign of the error: the single edge's b = -J^T Omega e
    opt2 = _device(g2o_amd_mod, prob)
    r = S.numpy_stage(prob, None, est=est)
    s = opt2.stage(r["lam"])
    assert np.linalg.norm(s["b"] - r["b"]) <= 1e-9 * np.linalg.norm(r["b"])
    assert np.linalg.norm(s["b"] + r["b"]) > np.linalg.norm(r["b"])
    assert opt2.block_dims() == [7, 0, 2, 0]
    # the estimate goes in and comes out as 8 doubles, q normalised with w >= 0; the minimal state is log()
    assert np.allclose(opt.estimates(V), S.normalized(prob.vertices[0].est), rtol=0, atol=4 * EPS)
    assert np.allclose(opt.minimal_state(), S.minimal(est[V]).ravel(), rtol=0, atol=1e-14)


# ---------------------------------------------------------------- 2: stage level at the kernel's edges
@pytest.mark.parametrize("ne", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("uniform", [False, True])
def test_stage_kernel_edges(g2o_amd_mod, uniform, ne):
    """A partial wave, a full wave (both 32-lane passes of the off-diagonal staging), a wave plus one edge, one edge past
    a 256-thread block; per-edge information records and one shared record (EdgeData::ue bit 0). The chain's errors cycle
    through the branches of log, every 8th vertex is fixed."""
    _stage_both(g2o_amd_mod, f"ne={ne} uniform={uniform}", S.edge_case(ne, uniform))


def test_stage_huber_and_fix_scale(g2o_amd_mod):
    prob = S.edge_case(65)
    est = {V: S.normalized(prob.vertices[0].est)}
    delta = float(np.sqrt(np.median(S.Graph(prob).edge_chi2(est))))  # half of the edges on Huber's linear branch
    _stage_both(g2o_amd_mod, "Huber", prob, ("Huber", delta))
    # _fix_scale: row and column 6 of every block hold lambda alone, b[6] = 0; LM's lambda keeps the solve definite
    _stage_both(g2o_amd_mod, "fix_scale", prob, fix_scale=True)
    opt = _device(g2o_amd_mod, prob, fix_scale=True)
    s = opt.stage(1.0)
    H = s["Hschur"] - np.eye(s["np"])
    assert not H[6::7].any() and not H[:, 6::7].any() and not s["b"][6::7].any() and H.any()


def test_shared_offdiagonal_blocks_and_transposed_edges(g2o_amd_mod):
    """Two edges between one vertex pair (per-edge slots summed by k_offblock_reduce at block size 49) and edges whose
    first vertex has the larger hessian index (the transposed orientation of the block)."""
    base = S.edge_case(12)
    es = base.edges[0]
    v0 = np.concatenate([es.v0, es.v1[:5], es.v0[3:6]])
    v1 = np.concatenate([es.v1, es.v0[:5], es.v1[3:6]])
    rng = np.random.default_rng(7500)
    meas = np.concatenate([es.meas, np.array([S._rand_sim3(rng, (0.9, 1.1)) for _ in range(8)])])
    info = np.concatenate([es.info, S._spd(rng, 7, 8)])
    prob = synth.Problem("sim3dup", base.vertices, [S._es(E, v0, v1, meas, info)], 7, 0)
    _stage_both(g2o_amd_mod, "duplicates", prob)


# ---------------------------------------------------------------- 3: branch inputs
@pytest.mark.parametrize("k", range(len(S.LOG_BRANCHES)))
def test_branch_inputs(g2o_amd_mod, k):
    """The log-branch cases of tests/test_sim3_host.py as one-edge graphs."""
    case = S.log_cases()[k]
    prob = S.one_edge(case)
    opt = _device(g2o_amd_mod, prob)
    est = _est_of(opt, prob)
    ref = S.Graph(prob).chi2(est=est)
    chi = opt.chi2()
    print(f"{case[0]}: chi2 {chi:.17g} numpy {ref:.17g} rel {abs(chi - ref) / ref:.2e}")
    assert abs(chi - ref) <= 1e-12 * ref
    r = S.numpy_stage(prob, None, est=est)
    _stage_against(case[0], opt.stage(r["lam"]), r)


# ---------------------------------------------------------------- 4: oplus
@pytest.mark.parametrize("fix_scale", [False, True])
def test_oplus_in_every_exp_branch(g2o_amd_mod, fix_scale):
    """SparseOptimizer::update with increments in each branch of the exponential, against sim3_ref in longdouble; one
    fixed vertex, which must not move. Tolerance per entry: max(64 eps, 8 x the float64-against-longdouble floor of the
    numpy restatement on the same inputs) x max(1, |value|)."""
    cases = S.exp_cases()
    n = len(cases)
    rng = np.random.default_rng(7600)
    est = np.array([S._rand_sim3(rng) for _ in range(n + 1)])
    fx = np.zeros(n + 1, np.int32)
    fx[-1] = 1
    ids = np.arange(n + 1)
    prob = synth.Problem("sim3oplus", [S._vs(V, ids, est, fx)],
                         [S._es(E, ids[:-1], ids[1:], est[:n], S._spd(rng, 7, n))], 7, 0)
    opt = _device(g2o_amd_mod, prob, fix_scale=fix_scale)
    opt.initialize_optimization()
    opt.build_structure()
    assert opt.vector_size() == 7 * n  # the free vertices in id order
    before = opt.estimates(V)
    u = np.array([c[1] for c in cases])
    opt.update(u.ravel())
    got = opt.estimates(V)
    want = S.oplus(before[:n], u, fix_scale, LD)
    f64 = S.oplus(before[:n], u, fix_scale)
    floor = float(np.max(np.abs(f64.astype(LD) - want) / np.maximum(1, np.abs(want))))
    err = np.abs(got[:n].astype(LD) - want) / np.maximum(1, np.abs(want))
    print(f"fix_scale={fix_scale}: worst {float(err.max()):.2e}, numpy float64 floor {floor:.2e}")
    assert float(err.max()) <= max(64 * EPS, 8 * floor)
    assert np.array_equal(got[n], before[n])
    if fix_scale:
        assert np.array_equal(got[:n, 7], before[:n, 7])  # update[6] is zeroed: no scale moves
    else:
        assert np.all(got[:n, 7] != before[:n, 7])
    # nothing is normalised after the product: the small-theta branches leave |q| != 1 by O(theta^4) at most
    assert np.max(np.abs(np.linalg.norm(got[:, 3:7], axis=1) - 1)) < 1e-12
    opt.push()
    opt.update(u.ravel())
    opt.pop()
    assert np.array_equal(opt.estimates(V), got)


# ---------------------------------------------------------------- 5: trajectories against the twin
def test_twin_stage_pin(g2o_amd_mod):
    _stage_both(g2o_amd_mod, "sim3_pose_graph", _graph())


@pytest.mark.parametrize("algo", ["lm_hip_var", "lm_hip_fix7_3", "gn_hip_var", "dl_hip_var"])
def test_trajectory_against_twin(g2o_amd_mod, algo):
    prob = _graph()
    dev = _run(_device(g2o_amd_mod, prob), 4, algo)
    print(f"{algo}: chi2 {dev[1]} trials {dev[2]}")
    _same_trajectory(dev, _twin_run(g2o_amd_mod, algo))
    assert dev[0] == 4 and dev[1][-1] < dev[1][0]


def test_trajectory_huber(g2o_amd_mod):
    prob = _graph()
    est = {V: S.normalized(prob.vertices[0].est)}
    robust = ("Huber", float(np.sqrt(np.median(S.Graph(prob).edge_chi2(est)))))
    dev = _run(_device(g2o_amd_mod, prob, robust), 4, "lm_hip_var")
    print(f"Huber: chi2 {dev[1]} trials {dev[2]}")
    _same_trajectory(dev, _twin_run(g2o_amd_mod, "lm_hip_var", robust))
    plain = _twin_run(g2o_amd_mod, "lm_hip_var")
    assert abs(dev[1][0] - plain[1][0]) > 1e-3 * plain[1][0]  # the kernel is at work: another trajectory


def test_trajectory_fix_scale(g2o_amd_mod):
    """LM under _fix_scale: the scales stay, the rest converges as the twin's does; Gauss-Newton on the same graph is
    not positive definite (H(6, 6) = 0), as in the reference."""
    prob = _graph()
    opt = _device(g2o_amd_mod, prob, fix_scale=True)
    s0 = opt.estimates(V)[:, 7]
    dev = _run(opt, 4, "lm_hip_fix7_3")
    _same_trajectory(dev, _run(_twin(g2o_amd_mod, prob, fix_scale=True), 4, "lm_hip_fix7_3"))
    assert np.array_equal(opt.estimates(V)[:, 7], s0) and dev[1][-1] < dev[1][0]
    gn = _device(g2o_amd_mod, prob, fix_scale=True)
    gn.set_algorithm("gn_hip_var")
    gn.initialize_optimization()
    gn.build_structure()
    gn.build_system()
    assert gn.solve() is False


# ---------------------------------------------------------------- 6: a larger graph through the factorisation
def test_300_pose_graph_linear_residual(g2o_amd_mod):
    """n = 2093: several supernodes, and block edges at multiples of 7, off the factor's 32-column panel grid."""
    prob = _cached("graph300", lambda: synth.sim3_pose_graph(num_poses=300, loops=200))
    opt = _device(g2o_amd_mod, prob)
    opt.set_algorithm("lm_hip_fix7_3")
    opt.initialize_optimization()
    opt.build_structure()
    opt.build_system()
    fi = opt.factor_info()
    print(f"n {fi['n']:.0f} supernodes {fi['supernodes']:.0f} levels {fi['levels']:.0f} max front {fi['max_front']:.0f}")
    assert fi["n"] == 299 * 7 and fi["supernodes"] > 1
    lam = 1e-5 * opt.diag_absmax()
    opt.set_lambda(lam)
    assert opt.solve()
    res = opt.linear_residual()
    print(f"linear residual {res:.2e}")
    assert res <= 1e-10
    # Hpp v on the device (k_block_symv<7>) against the dense system
    est = _est_of(opt, prob)
    H = S.numpy_stage(prob, lam, est=est)["H"]
    v = np.random.default_rng(7700).standard_normal(H.shape[0])
    got = opt.multiply_hessian(v)
    want = (H + lam * np.eye(len(v))) @ v
    assert np.linalg.norm(got - want) <= 1e-11 * np.linalg.norm(want)
    chi0 = S.Graph(prob).chi2(est=est)
    n, st = opt.optimize(3)
    print(f"chi2 {chi0:.6g} -> {[s.chi2 for s in st]}")
    assert n == 3 and st[0].chi2 < 0.5 * chi0 and all(b.chi2 <= a.chi2 for a, b in zip(st, st[1:]))


# ---------------------------------------------------------------- 7: per-edge chi2, levels, classification
def test_levels_chi2_classify(g2o_amd_mod):
    prob = _graph()
    opt = _device(g2o_amd_mod, prob)
    opt.initialize_optimization()
    ref = S.Graph(prob).edge_chi2(_est_of(opt, prob))
    lv = np.zeros(len(ref), np.int32)
    lv[::7] = 2  # some edges set aside first: the per-edge chi2 covers the inactive ones too
    opt.set_edge_levels(E, lv)
    chi = opt.edge_chi2(E)
    print(f"per-edge chi2 worst {np.max(np.abs(chi - ref) / ref):.2e}")
    assert len(chi) == len(ref) and np.max(np.abs(chi - ref) / ref) <= 1e-12
    srt = np.sort(ref)
    top = srt[len(srt) // 2:]  # a threshold in the upper half: some, not all, edges are outliers
    k = int(np.argmax(np.diff(top)))
    gap = (top[k + 1] - top[k]) / top[k]
    thr = 0.5 * (top[k] + top[k + 1])
    print(f"threshold {thr:.6g} in a gap of {gap:.2e} relative")
    assert gap > 1e-9
    bad = ref > thr
    counts = opt.classify_edges(E, thr)
    assert counts == dict(over_chi2=int(bad.sum()), depth_failed=0, bad=int(bad.sum())) and 0 < bad.sum() < len(bad)
    assert np.array_equal(opt.edge_levels(E), bad.astype(np.int32))
    for call in (lambda: opt.classify_edges(E, thr, check_depth=True), lambda: opt.edge_chi2(E, depth=True)):
        with pytest.raises(g2o_amd_mod.G2OHipError) as ei:  # EdgeSim3 has no isDepthPositive
            call()
        assert f"({ERR_ARG})" in str(ei.value)
    opt.initialize_optimization(0)
    tw = _twin(g2o_amd_mod, prob, levels=bad.astype(np.int32))
    tw.initialize_optimization(0)
    dev, twr = _run(opt, 3, "lm_hip_var"), _run(tw, 3, "lm_hip_var")
    _same_trajectory(dev, twr)
    assert dev[1][0] < float(np.sum(ref))  # the outliers are out of the system


# ---------------------------------------------------------------- 8: marginals
def test_marginals(g2o_amd_mod):
    """K = 63 right-hand sides per solve (nine block columns of 7)."""
    prob = _graph()
    opt = _device(g2o_amd_mod, prob)
    opt.set_algorithm("lm_hip_var")
    opt.initialize_optimization()
    opt.build_structure()
    opt.build_system()
    pd, _, npose, _ = opt.block_dims()
    H = S.numpy_stage(prob, 0.0, est=_est_of(opt, prob))["H"]
    assert pd == 7 and H.shape == (npose * pd, npose * pd)
    Hinv = np.linalg.inv(H)
    pat = [(k, k) for k in range(0, npose, 3)] + [(3, 7), (2, npose - 1), (npose - 1, npose - 1)]
    assert len({c for _, c in pat}) > 9  # more than one batch of block columns
    blocks = opt.compute_marginals(pat)
    assert blocks is not None and len(blocks) == len(set(pat))
    num = den = 0.0
    for (r, c), B in blocks.items():
        Rf = Hinv[r * pd:(r + 1) * pd, c * pd:(c + 1) * pd]
        num += float(np.sum((B - Rf) ** 2))
        den += float(np.sum(Rf ** 2))
    print(f"marginals {np.sqrt(num / den):.2e}")
    assert np.sqrt(num / den) <= 1e-9


# ---------------------------------------------------------------- 9: host-Jacobian edges on Sim3 vertices
@pytest.mark.parametrize("inverse", [False, True])
def test_hostj_projection_edges(g2o_amd_mod, inverse):
    """EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ as G2OHIP_E_HOSTJ(2) from fixed points (dimension 3) to one free
    Sim3 vertex (dimension 7): OptimizeSim3's shape, at stage level against numpy and through LM."""
    prob, records = S.projection_problem(inverse=inverse)
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    est = _est_of(opt, prob)
    rec = records(est[V][0])
    opt.set_host_jacobians(34, rec)
    opt.initialize_optimization()
    r = S.numpy_stage(prob, None, est=est, binary={34: rec})
    _stage_against(f"projection inverse={inverse}", opt.stage(r["lam"]), r)
    assert opt.block_dims() == [7, 0, 1, 0]
    opt.set_host_edge_callback(lambda etype, with_jac: records(opt.estimates(V)[0]))
    chi0 = opt.chi2()
    ref0 = S.Graph(prob).chi2(est=est, binary={34: rec})
    assert abs(chi0 - ref0) <= 1e-12 * ref0
    n, st = opt.optimize(5)
    print(f"inverse={inverse}: chi2 {chi0} -> {[s.chi2 for s in st]}")
    assert n == 5 and st[-1].chi2 < 0.9 * chi0 and all(b.chi2 <= a.chi2 for a, b in zip(st, st[1:]))


def test_hostj_unary_on_a_sim3_vertex(g2o_amd_mod):
    """G2OHIP_E_HOSTJ_UNARY(7) on Sim3 vertices beside the device's EdgeSim3: a prior e = log(Z S^-1)."""
    prob = S.edge_case(9)
    vs = prob.vertices[0]
    rng = np.random.default_rng(7800)
    free = vs.ids[vs.fixed == 0]
    z = S.normalized(vs.est)[vs.fixed == 0]
    info = S._spd(rng, 7, len(free))
    full = synth.Problem("sim3prior", prob.vertices, prob.edges + [S._es(48 + 7, free, None, np.zeros((len(free), 1)), info)], 7, 0)
    full.edges[1].meas = None
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(full)
    est = _est_of(opt, full)
    # e = log(I * Z * S^-1) with Z the start moved a little: the edge function with C = identity, v0 = Z, v1 = S
    ident = np.broadcast_to([0, 0, 0, 0, 0, 0, 1.0, 1.0], z.shape)
    zm = S.oplus(z, 0.01 * rng.standard_normal((len(free), 7)))
    e, _, J = S.edge(zm, est[V][vs.fixed == 0], ident)
    rec = np.concatenate([e, J.reshape(len(free), -1)], 1).ravel()
    opt.set_host_jacobians(55, rec)
    opt.initialize_optimization()
    g = S.Graph(prob)
    H, b = g.dense_system(est=est)
    for k, i in enumerate(free):
        o = g.off[int(i)]
        H[o:o + 7, o:o + 7] += J[k].T @ info[k] @ J[k]
        b[o:o + 7] -= J[k].T @ info[k] @ e[k]
    lam = 1e-5 * float(np.max(np.diag(H)))
    s = opt.stage(lam)
    r = dict(b=b, x=np.linalg.solve(H + lam * np.eye(len(b)), b), Hschur=H + lam * np.eye(len(b)), bschur=b, n=len(b), np=len(b))
    _stage_against("unary host-J", s, r)


# ---------------------------------------------------------------- 10: .g2o files
def test_g2o_save_load(g2o_amd_mod, tmp_path):
    """On an arc of the ring (sim3_ref.arc_problem): the lines hold logs of cam2world transforms, which lose digits
    near a half turn; the arc stays 0.7 rad clear of it."""
    prob = S.arc_problem()
    nv, ne = len(prob.vertices[0].ids), len(prob.edges[0].v0)
    a = _device(g2o_amd_mod, prob)
    a.optimize(1)  # the state that is written is the device's
    path = str(tmp_path / "sim3.g2o")
    a.save(path)
    text = open(path).read()
    assert text.count("VERTEX_SIM3:EXPMAP ") == nv == 14 and text.count("EDGE_SIM3:EXPMAP ") == ne > 20
    assert "FIX 26\n" in text
    first = next(l for l in text.splitlines() if l.startswith("VERTEX_SIM3"))
    assert len(first.split()) == 13 and first.split()[-4:] == ["1", "1", "0", "0"]
    b = g2o_amd_mod.SparseOptimizer(0)
    b.load(path, sim3=True)
    assert b.num_vertices() == nv and b.num_edges() == ne
    ea, eb = a.estimates(V), b.estimates(V)
    # oplus normalises nothing, so an optimised quaternion may have w < 0; the reader's Sim3(...).inverse() brings it
    # back to w >= 0: the same rotation, compared with the sign the reader chose
    assert np.all(eb[:, 6] >= 0)
    ea[:, 3:7] *= np.where(ea[:, 6:7] < 0, -1.0, 1.0)
    err = np.max(np.abs(ea - eb)) / np.max(np.abs(ea))
    print(f"state after save -> load: {err:.2e}")
    assert err <= 1e-12
    ca, cb = a.chi2(), b.chi2()
    print(f"chi2 {ca:.17g} {cb:.17g}")
    assert abs(ca - cb) <= 1e-12 * ca
    # the reference's own lines (sim3_ref.g2o_text) load to the same graph
    ref_path = str(tmp_path / "ref.g2o")
    with open(ref_path, "w") as f:
        f.write(S.g2o_text(prob, (420.0, 415.0, 320.0, 240.0)))
    c = g2o_amd_mod.SparseOptimizer(0)
    c.load(ref_path, sim3=True)
    fresh = _device(g2o_amd_mod, prob)
    assert np.max(np.abs(c.estimates(V) - fresh.estimates(V))) <= 1e-12 * np.max(np.abs(fresh.estimates(V)))
    assert abs(c.chi2() - fresh.chi2()) <= 1e-12 * fresh.chi2()
    out2 = str(tmp_path / "again.g2o")
    c.save(out2)  # the intrinsics of the lines stay on the host and are written back
    assert next(l for l in open(out2) if l.startswith("VERTEX_SIM3")).split()[-4:] == ["420", "415", "320", "240"]
    # without the flag both tags are skipped; a vertex line of another length fails the load and names the tag
    d = g2o_amd_mod.SparseOptimizer(0)
    d.load(ref_path)
    assert d.num_vertices() == 0 and d.num_edges() == 0
    seven = str(tmp_path / "seven.g2o")
    with open(seven, "w") as f:
        f.write("VERTEX_SIM3:EXPMAP 0 0.1 0.2 0.3 1 2 3 0.05\nVERTEX_SIM3:EXPMAP 1 0 0 0 0 0 0 0\n")
    e7 = g2o_amd_mod.SparseOptimizer(0)
    e7.load(seven, sim3=True)
    want = S.inv(S.exp(np.array([0.1, 0.2, 0.3, 1, 2, 3, 0.05])))
    assert np.max(np.abs(e7.estimates(V)[0] - want[0])) <= 1e-14
    bad = str(tmp_path / "bad.g2o")
    with open(bad, "w") as f:
        f.write("VERTEX_SIM3:EXPMAP 0 0 0 0 0 0 0 0 1 1\n")
    with pytest.raises(g2o_amd_mod.G2OHipError) as ei:
        g2o_amd_mod.SparseOptimizer(0).load(bad, sim3=True)
    assert f"({ERR_ARG})" in str(ei.value) and "VERTEX_SIM3:EXPMAP" in str(ei.value)


# ---------------------------------------------------------------- 11: refusals
def _with_point(prob, marg):
    """The graph with one free V_XYZ point beside the Sim3 poses, seen through a host-J projection edge."""
    pt = S._vs(synth.V_XYZ, [1000], [[0.1, 0.2, 4.0]], marg=marg)
    edge = S._es(34, [1000], [1], np.zeros((1, 1)), np.eye(2)[None])
    edge.meas = None
    return synth.Problem("sim3+point", list(prob.vertices) + [pt], list(prob.edges) + [edge], 7, 3 if marg else 0)


def test_refusals(g2o_amd_mod):
    mod = g2o_amd_mod
    prob = S.edge_case(9)

    def refused(opt, call, code, *words):
        with pytest.raises(mod.G2OHipError) as ei:
            call()
        msg = str(ei.value)
        assert (code is None or f"({code})" in msg) and mod.last_error() and all(w in msg for w in words), msg

    # a free marginalised point: the 7/3 Schur kernels do not exist
    opt = mod.SparseOptimizer(0).add_problem(_with_point(prob, 1))
    refused(opt, opt.initialize_optimization, ERR_UNSUPPORTED, "7/3 Schur kernels do not exist")
    refused(opt, opt.build_structure, ERR_UNSUPPORTED, "7/3")
    # a free non-marginalised point: one pose block size
    opt = mod.SparseOptimizer(0).add_problem(_with_point(prob, 0))
    refused(opt, opt.initialize_optimization, ERR_UNSUPPORTED, "one pose block size")
    # the iterative solvers
    for algo in ("lm_pcg", "gn_pcg", "lm_pcg6_3", "lm_pcg6_3_eigen"):
        opt = _device(mod, prob)
        opt.set_algorithm(algo)
        refused(opt, opt.build_structure, ERR_UNSUPPORTED, "blocks of 7")
        refused(opt, lambda: opt.optimize(1), ERR_UNSUPPORTED, "blocks of 7")
    opt = _device(mod, prob)
    refused(opt, lambda: opt.set_algorithm("lm_pcg7_3"), ERR_UNSUPPORTED, "7_3")
    refused(opt, lambda: opt.set_algorithm("dl_pcg7_3"), ERR_ARG)
    for name in ("lm_hip_fix7_3", "gn_hip_fix7_3", "dl_hip_fix7_3"):
        opt.set_algorithm(name)
    # arguments
    es = prob.edges[0]
    with_params = synth.EdgeSet(E, es.v0, es.v1, es.meas, es.info, np.zeros((len(es.v0), 4)))
    opt = mod.SparseOptimizer(0)
    opt.add_vertices(prob.vertices[0])
    refused(opt, lambda: opt.add_edges(with_params), ERR_ARG)
    short = synth.EdgeSet(E, es.v0, es.v1, es.meas[:, :7], es.info)
    refused(opt, lambda: opt.add_edges(short), None, "8 measurement values")  # (the wrapper's own stride checks)
    bad_v = synth.VertexSet(V, prob.vertices[0].ids + 500, prob.vertices[0].est[:, :7], prob.vertices[0].fixed,
                            prob.vertices[0].marginalized)
    refused(opt, lambda: opt.add_vertices(bad_v), None, "8 estimate values")
    assert mod.lib().g2ohip_set_sim3_fix_scale(opt.h, 2) == ERR_ARG
    # an EdgeSim3 on a vertex of another type
    cams = S._vs(synth.V_SE3_EXPMAP, [0, 1], [[0, 0, 0, 0, 0, 0, 1.0]] * 2)
    wrong = synth.Problem("wrong", [cams], [S._es(E, [0], [1], es.meas[:1], es.info[:1])], 6, 0)
    opt = mod.SparseOptimizer(0).add_problem(wrong)
    refused(opt, opt.initialize_optimization, ERR_UNSUPPORTED, "edge type 27")
    # per-edge chi2 of the host-J twin stays with the host
    tw = _twin(mod, prob)
    tw.initialize_optimization()
    refused(tw, lambda: tw.edge_chi2(HJ), ERR_UNSUPPORTED)
