"""types_icp on the device (G2OHIP_E_V_V_GICP, G2OHIP_E_XYZ_VSC): FamilyGICP in both modes through k_error,
k_linearize and the pair-major assembly (k_linearize_pairs, k_pair_reduce), the information hook (plane-to-plane:
Omega follows the state), FamilyVSC on the slot and 6/3 Schur paths, levels and classification, marginals,
update_initialization, structure-only, landmark shards, .g2o files and the refusals.

Two references: tests/icp_ref.py (plain numpy) for chi2 and the stage level, and the same graph with each new edge set
entered as G2OHIP_E_HOSTJ(3) edges whose host callback returns icp_ref's records (the twin; a plane-to-plane set's
records whitened with Omega = L L^T at the current state) for the trajectories. The pair-major path is compared with
numpy and with the forced slot path (set_pair_major(False)) of the same graph.

Tolerances are the project's own (tests/test_gpu_offset.py): chi2 against numpy 1e-12 relative (tests/test_icp_host.py
measures a float64 floor of 1.9e-14 on these cases, under the 1e-13 that keeps 1e-12), stage level 1e-9 (b, bschur, x)
and 1e-11 (H), trajectories 1e-6 relative with identical trial counts, lm_pcg 1e-5, marginals 1e-9, structure-only
1e-6 with equal counts, shards 1e-9 on the state and 1e-6 on chi2. Every graph has at most 20 poses and 6,000 edges.
"""
import threading
import uuid

import numpy as np
import pytest

import icp_ref as I
import structure_only_ref
from g2o_amd import synth
from icp_ref import GICP, HOSTJ3, VSC

pytestmark = pytest.mark.gpu

RTOL = 1e-6
PCG_RTOL = 1e-5
ERR_ARG, ERR_UNSUPPORTED = -1, -4
POSE = synth.V_SE3_QUAT
_CACHE = {}  # problems and reference runs, computed once, shared, left unchanged


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _est_of(opt, prob):
    return {v.vtype: opt.estimates(v.vtype) for v in prob.vertices}


def _device(mod, prob, robust=None, pair_major=True):
    opt = mod.SparseOptimizer(0).add_problem(prob)
    if not pair_major:
        opt.set_pair_major(False)
    for et, (kind, delta) in (robust or {}).items():
        opt.set_robust_kernel(et, kind, delta)
    return opt


def _twin(mod, prob, robust=None, levels=None):
    """The graph with its GICP / VSC sets entered as one E_HOSTJ(3) set, icp_ref's records in the callback."""
    g = I.Graph(prob)
    opt = mod.SparseOptimizer(0).add_problem(I.hostj_problem(prob))
    opt.set_host_edge_callback(lambda etype, with_jac: g.payload(_est_of(opt, prob)))
    if robust:
        (kind, delta), = set(robust.values())
        opt.set_robust_kernel(HOSTJ3, kind, delta)
    if levels is not None:
        opt.set_edge_levels(HOSTJ3, levels)
    return opt


def _stage_against(tag, s, r):
    assert s["ok"] == 1 and (s["n"], s["np"]) == (r["n"], r["np"]), (tag, s["n"], s["np"], r["n"], r["np"])
    for k in ("b", "x", "bschur"):
        err = np.linalg.norm(s[k] - r[k]) / np.linalg.norm(r[k])
        print(f"{tag} {k}: {err:.2e}")
        assert err <= 1e-9, (tag, k, err)
    err = np.linalg.norm(s["Hschur"] - r["Hschur"]) / np.linalg.norm(r["Hschur"])
    print(f"{tag} H: {err:.2e}")
    assert err <= 1e-11, (tag, err)


def _stage_numpy(tag, opt, prob, robust=None, levels=None, pair_major=None):
    """The handle against numpy at its own estimates: chi2 and the stage level."""
    est = _est_of(opt, prob)
    r = I.numpy_stage(prob, None, robust, est, levels)
    s = opt.stage(r["lam"])
    if pair_major is not None:
        assert opt.pair_major_info()["pair_major"] == pair_major, (tag, opt.pair_major_info())
    _stage_against(tag, s, r)
    ref = I.Graph(prob, levels).chi2(est=est, robust=robust)
    chi = opt.chi2()
    print(f"{tag} chi2 {chi:.17g} numpy {ref:.17g} rel {abs(chi - ref) / ref:.2e}")
    assert abs(chi - ref) <= 1e-12 * ref, (tag, chi, ref)
    return s


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


def _scans(pl_pl=False):
    """Multiplicities 1, 64, 200, pairs entered both ways round, scans 0 and 1 fixed: pair (0, 1) has both ends
    fixed, pairs (0, 2), (1, 2), (1, 3), (4, 0), (5, 0), (5, 1) one."""
    return _cached(("scans", pl_pl), lambda: synth.gicp_scans(6, 2, (1, 64, 200), pl_pl=pl_pl, fixed=(0, 1)))


def _scans_noisy():
    """The same with a position noise of 0.3: no edge's error is small beside its points' coordinates, so the per-edge
    chi2 has a float64 floor under 1e-13 (tests/test_icp_host.py::test_edge_chi2_float64_floor; 3.2e-13 at 0.01)."""
    return _cached("scans_noisy", lambda: synth.gicp_scans(6, 2, (1, 64, 200), fixed=(0, 1), euc_noise=0.3))


def _ring(pl_pl=False):
    """Eight scans, one fixed, 150 correspondences per pair: the trajectories' graph."""
    return _cached(("ring", pl_pl), lambda: synth.gicp_scans(8, 2, 150, pl_pl=pl_pl))


def _sba():
    return _cached("sba", lambda: synth.gicp_sba(n_matches=200, n_points=100, num_cams=3))


# ---------------------------------------------------------------- 1: single-edge pins
@pytest.mark.parametrize("case", ["gicp", "gicp_plpl", "vsc_cam", "vsc_point"])
def test_single_edge_pins(g2o_amd_mod, case):
    etype = GICP if case.startswith("gicp") else VSC
    prob = (I.one_edge(GICP, case == "gicp_plpl") if etype == GICP else I.one_edge(VSC, free=case[4:]))
    opt = _device(g2o_amd_mod, prob)
    est = _est_of(opt, prob)
    g = I.Graph(prob)
    ref = g.chi2(est=est)
    chi = opt.chi2()
    print(f"{case}: chi2 device {chi:.17g} numpy {ref:.17g} rel {abs(chi - ref) / ref:.2e}")
    assert ref > 0 and abs(chi - ref) <= 1e-12 * ref
    delta = 0.5 * np.sqrt(ref)  # sqrt(e2) > delta: Huber's linear branch, chi2 = rho
    opt.set_robust_kernel(etype, "Huber", delta)
    rho = 2 * np.sqrt(ref) * delta - delta * delta
    assert abs(opt.chi2() - rho) <= 1e-12 * rho
    assert abs(g.chi2(est=est, robust={etype: ("Huber", delta)}) - rho) <= 1e-12 * rho
    # the stage: b = -J^T Omega e and H = J^T Omega J of the single edge (its sign too)
    opt2 = _device(g2o_amd_mod, prob)
    r = I.numpy_stage(prob, None, est=est)
    s = opt2.stage(r["lam"])
    assert np.linalg.norm(s["b"] - r["b"]) <= 1e-9 * np.linalg.norm(r["b"])
    assert np.linalg.norm(s["b"] + r["b"]) > np.linalg.norm(r["b"])
    assert np.linalg.norm(s["Hschur"] - r["Hschur"]) <= 1e-11 * np.linalg.norm(r["Hschur"])
    assert opt2.pair_major_info()["pair_major"] == (etype == GICP)


# ---------------------------------------------------------------- 2: chunk edges
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 4097])
def test_pair_chunk_edges(g2o_amd_mod, n):
    """One pair with a partial chunk, a full one, a chunk plus one edge, three chunks, and 65 chunks (more than one per
    wave of k_pair_reduce, more than one workgroup of k_linearize_pairs): pair-major and forced slot path, each
    against numpy, and against each other."""
    prob = _cached(("pair", n), lambda: synth.gicp_pair(n))
    pm, sl = _device(g2o_amd_mod, prob), _device(g2o_amd_mod, prob, pair_major=False)
    s1 = _stage_numpy(f"pair-major n={n}", pm, prob, pair_major=True)
    s2 = _stage_numpy(f"slot n={n}", sl, prob, pair_major=False)
    info = pm.pair_major_info()
    assert info["pairs"] == 1 and info["chunks"] == (n + 63) // 64, info
    _stage_against(f"pair-major against slot n={n}", s1, dict(s2, n=s2["n"], np=s2["np"]))


# ---------------------------------------------------------------- 3: orientation and fixed ends
@pytest.mark.parametrize("pl_pl", [False, True])
def test_orientation_and_fixed_ends(g2o_amd_mod, pl_pl):
    prob = _scans(pl_pl)
    es = prob.edges[0]
    both = {(int(u), int(v)) for u, v in zip(es.v0, es.v1)}
    assert any((v, u) in both for u, v in both)  # a vertex pair entered as (i, j) and as (j, i)
    pm = _device(g2o_amd_mod, prob)
    s1 = _stage_numpy(f"scans pl_pl={pl_pl} pair-major", pm, prob, pair_major=True)
    # 12 vertex pairs: (0, 1) is inactive; a fixed end counts as "no block", so the pairs (fixed, h) of one free
    # vertex h fall into one run: free vertices 2, 3, 4, 5 have such runs, and (2,3) (2,4) (3,4) (3,5) (4,5) are free pairs
    assert pm.pair_major_info()["pairs"] == 9, pm.pair_major_info()
    sl = _device(g2o_amd_mod, prob, pair_major=False)
    s2 = _stage_numpy(f"scans pl_pl={pl_pl} slot", sl, prob, pair_major=False)
    _stage_against("pair-major against slot", s1, dict(s2, n=s2["n"], np=s2["np"]))


def test_pair_major_with_priors(g2o_amd_mod):
    """Unary priors beside the GICP edges keep their own kernel and slots; the graph stays pair-major."""
    prob = _cached("scans_priors", lambda: synth.with_priors(_scans(), synth.E_SE3_PRIOR, every=2, sigma=0.1))
    assert {es.etype for es in prob.edges} == {GICP, synth.E_SE3_PRIOR}
    _stage_numpy("priors pair-major", _device(g2o_amd_mod, prob), prob, pair_major=True)
    _stage_numpy("priors slot", _device(g2o_amd_mod, prob, pair_major=False), prob, pair_major=False)


def test_mixed_with_edge_se3_takes_the_slot_path(g2o_amd_mod):
    """Another binary edge type in the graph: the slot path, as before."""
    base = _scans()
    poses = base.vertices[0]
    a, b = np.arange(2, 5, dtype=np.int32), np.arange(3, 6, dtype=np.int32)
    z = np.tile([0.5, 0.1, 0.0, 0, 0, 0, 1.0], (3, 1))
    odo = synth.EdgeSet(synth.E_SE3_QUAT, a, b, z, np.broadcast_to(np.eye(6), (3, 6, 6)).copy())
    prob = synth.Problem("mixed", [poses], [base.edges[0], odo], 6, 0)
    opt = _device(g2o_amd_mod, prob)
    opt.set_algorithm("lm_hip_var")
    n, st = opt.optimize(2)
    assert n == 2 and np.isfinite(st[-1].chi2) and not opt.pair_major_info()["pair_major"]


# ---------------------------------------------------------------- 4: bitwise reproducibility
@pytest.mark.parametrize("pl_pl", [False, True])
def test_bitwise_reproducibility(g2o_amd_mod, pl_pl):
    prob = _scans(pl_pl)
    out = []
    for _ in range(2):
        opt = _device(g2o_amd_mod, prob)
        s = opt.stage(1e-3)
        assert opt.pair_major_info()["pair_major"]
        opt.set_algorithm("lm_hip_var")
        opt.optimize(5)
        out.append((s["Hschur"], s["b"], opt.minimal_state()))
    for x, y in zip(*out):
        assert np.array_equal(x, y)


# ---------------------------------------------------------------- 5: plane-to-plane, Omega follows the state
def test_plane_to_plane_follows_the_state(g2o_amd_mod):
    """After optimize(3) chi2 and the stage are numpy's at the handle's new estimates. The three iterations start from
    lambda = 1e4 (a sixth of max diag(H)), so the state moves most of the way without converging: at a converged state
    b = -sum J^T Omega e is a cancelling sum (numpy, three undamped steps on this graph: sum |terms| / |b| = 1.4e7, so
    float64 carries b to 1e-9 at best; with this damping the ratio is 17) and a relative bound on b checks nothing."""
    prob = _ring(True)
    opt = _device(g2o_amd_mod, prob)
    opt.set_algorithm("lm_hip_var")
    chi0 = opt.chi2()
    opt.optimize(3, lambda_init=1e4)
    est = _est_of(opt, prob)
    assert np.linalg.norm(est[POSE] - prob.vertices[0].est) > 1e-3  # the poses moved
    g = I.Graph(prob)
    om0, om1 = g.terms(prob.edges[0])[3], g.terms(prob.edges[0], est)[3]
    assert np.max(np.abs(om1 - om0)) > 1e-6 * np.max(np.abs(om0))  # and so did the information
    _stage_numpy("pl_pl after optimize(3)", opt, prob, pair_major=True)
    assert opt.chi2() < chi0
    # the information frozen at the start gives another chi2 at the new state: the device did not keep it
    e = g.terms(prob.edges[0], est, jac=False)[0]
    frozen = float(np.sum(np.einsum("ni,nij,nj->n", e, om0, e)))
    assert abs(frozen - opt.chi2()) > 1e-9 * opt.chi2()


@pytest.mark.parametrize("algo", ["lm_hip_var", "gn_hip_var", "dl_hip_var", "lm_hip_fix6_6"])
@pytest.mark.parametrize("pl_pl", [False, True])
def test_trajectory_against_twin(g2o_amd_mod, pl_pl, algo):
    prob = _ring(pl_pl)
    dev = _run(_device(g2o_amd_mod, prob), 4, algo)
    print(f"{algo} pl_pl={pl_pl}: chi2 {dev[1]} trials {dev[2]}")
    tw = _cached(("twinrun", pl_pl, algo), lambda: _run(_twin(g2o_amd_mod, prob), 4, algo))
    _same_trajectory(dev, tw)
    assert dev[1][-1] < dev[1][0]


@pytest.mark.parametrize("pl_pl", [False, True])
def test_slot_path_trajectory_against_twin(g2o_amd_mod, pl_pl):
    prob = _ring(pl_pl)
    dev = _run(_device(g2o_amd_mod, prob, pair_major=False), 4, "lm_hip_var")
    _same_trajectory(dev, _cached(("twinrun", pl_pl, "lm_hip_var"), lambda: _run(_twin(g2o_amd_mod, prob), 4, "lm_hip_var")))


# ---------------------------------------------------------------- 6: robust kernels
KERNELS = ["Huber", "PseudoHuber", "Cauchy", "GemanMcClure", "Welsch", "Fair", "Tukey", "Saturated", "DCS"]


@pytest.mark.parametrize("kind", KERNELS)
def test_robust_chi2_pins(g2o_amd_mod, kind):
    """All nine kernels on point-to-plane: the robustified chi2 and the rho'-weighted system against numpy."""
    prob = _scans()
    e2 = I.Graph(prob).edge_chi2(GICP)
    delta = float(np.sqrt(np.median(e2)))  # half of the edges past the kernel's knee
    _stage_numpy(f"{kind}", _device(g2o_amd_mod, prob, {GICP: (kind, delta)}), prob, {GICP: (kind, delta)}, pair_major=True)


@pytest.mark.parametrize("kind", ["Huber", "Cauchy"])
@pytest.mark.parametrize("pl_pl", [False, True])
def test_robust_trajectory(g2o_amd_mod, pl_pl, kind):
    prob = _ring(pl_pl)
    delta = float(np.sqrt(np.median(I.Graph(prob).edge_chi2(GICP))))
    robust = {GICP: (kind, delta)}
    dev = _run(_device(g2o_amd_mod, prob, robust), 4, "lm_hip_var")
    print(f"{kind} pl_pl={pl_pl}: chi2 {dev[1]} trials {dev[2]}")
    _same_trajectory(dev, _run(_twin(g2o_amd_mod, prob, robust), 4, "lm_hip_var"))
    plain = _cached(("twinrun", pl_pl, "lm_hip_var"), lambda: _run(_twin(g2o_amd_mod, prob), 4, "lm_hip_var"))
    assert abs(dev[1][0] - plain[1][0]) > 1e-3 * plain[1][0]  # the kernel is at work: another trajectory


# ---------------------------------------------------------------- 7: levels and the outlier loop
def test_levels_and_outlier_loop(g2o_amd_mod):
    """set_edge_levels takes every edge of one pair and part of another off level 0; the pair-major table follows.
    Then classify_edges and a re-initialization: the stage on the surviving edges."""
    prob = _scans_noisy()
    es = prob.edges[0]
    lo, hi = np.minimum(es.v0, es.v1), np.maximum(es.v0, es.v1)
    lv = np.zeros(len(es.v0), np.int32)
    lv[(lo == 2) & (hi == 4)] = 1  # a whole pair
    part = np.nonzero((lo == 3) & (hi == 5))[0]
    lv[part[::2]] = 1              # every second edge of another
    assert 0 < lv.sum() < len(lv) and len(part) >= 64
    opt = _device(g2o_amd_mod, prob)
    opt.stage(1e-3)
    pairs0 = opt.pair_major_info()["pairs"]
    opt.set_edge_levels(GICP, lv)
    opt.initialize_optimization(0)
    _stage_numpy("levels", opt, prob, levels={GICP: lv}, pair_major=True)
    assert opt.pair_major_info()["pairs"] == pairs0 - 1
    # per-edge chi2 covers the inactive edges too; classification at a threshold inside a gap
    ref = I.Graph(prob).edge_chi2(GICP, _est_of(opt, prob))
    chi = opt.edge_chi2(GICP)
    assert len(chi) == len(ref) and np.max(np.abs(chi - ref) / ref) <= 1e-12
    top = np.sort(ref)[len(ref) // 2:]
    k = int(np.argmax(np.diff(top)))
    thr = 0.5 * (top[k] + top[k + 1])
    assert (top[k + 1] - top[k]) / top[k] > 1e-9
    bad = ref > thr
    counts = opt.classify_edges(GICP, thr)
    assert counts == dict(over_chi2=int(bad.sum()), depth_failed=0, bad=int(bad.sum())) and 0 < bad.sum() < len(bad)
    assert np.array_equal(opt.edge_levels(GICP), bad.astype(np.int32))
    with pytest.raises(g2o_amd_mod.G2OHipError) as ei:
        opt.classify_edges(GICP, thr, check_depth=True)
    assert f"({ERR_ARG})" in str(ei.value)
    opt.initialize_optimization(0)
    _stage_numpy("after classify", opt, prob, levels={GICP: bad.astype(np.int32)}, pair_major=True)
    dev = _run(opt, 3, "lm_hip_var")
    tw = _twin(g2o_amd_mod, prob, levels=bad.astype(np.int32))
    tw.initialize_optimization(0)
    _same_trajectory(dev, _run(tw, 3, "lm_hip_var"))


# ---------------------------------------------------------------- 8: solver modes
def test_update_initialization(g2o_amd_mod):
    """A new scan and its edges join through update_initialization; the pair-major table is rebuilt."""
    prob = _ring()
    es, poses = prob.edges[0], prob.vertices[0]
    last = int(poses.ids[-1])
    new = (es.v0 == last) | (es.v1 == last)
    sub = lambda m: synth.EdgeSet(GICP, es.v0[m], es.v1[m], es.meas[m], es.info[m], None)  # noqa: E731
    vs = lambda m: synth.VertexSet(POSE, poses.ids[m], poses.est[m], poses.fixed[m], poses.marginalized[m])  # noqa: E731
    old_v = poses.ids != last
    opt = _device(g2o_amd_mod, synth.Problem("first", [vs(old_v)], [sub(~new)], 6, 0))
    opt.set_algorithm("lm_hip_var")
    opt.optimize(2)
    p0 = opt.pair_major_info()
    opt.add_vertices(vs(~old_v))
    opt.add_edges(sub(new))
    opt.update_initialization()
    assert opt.num_edges() == len(es.v0)
    # the handle's edge order: the first edges, then the new ones
    order = np.concatenate([np.nonzero(~new)[0], np.nonzero(new)[0]])
    whole = synth.Problem("whole", [poses], [synth.EdgeSet(GICP, es.v0[order], es.v1[order], es.meas[order], es.info[order], None)], 6, 0)
    _stage_numpy("online", opt, whole, pair_major=True)
    p1 = opt.pair_major_info()
    assert p1["pairs"] > p0["pairs"] and p1["chunks"] > p0["chunks"], (p0, p1)


def test_marginals_and_multiply_hessian(g2o_amd_mod):
    prob = _ring()
    opt = _device(g2o_amd_mod, prob)
    opt.set_algorithm("lm_hip_var")
    opt.initialize_optimization()
    opt.build_structure()
    opt.build_system()
    assert opt.pair_major_info()["pair_major"]
    pd, _, npose, _ = opt.block_dims()
    H = I.numpy_stage(prob, 0.0, est=_est_of(opt, prob))["H"]
    assert H.shape == (npose * pd, npose * pd)
    v = np.random.default_rng(3).standard_normal(npose * pd)
    hv = opt.multiply_hessian(v)
    assert np.linalg.norm(hv - H @ v) <= 1e-11 * np.linalg.norm(H @ v)
    Hinv = np.linalg.inv(H)
    pat = [(0, 0), (3, 3), (3, 5), (npose - 1, npose - 1), (2, npose - 1)]
    blocks = opt.compute_marginals(pat)
    assert blocks is not None and len(blocks) == len(pat)
    num = den = 0.0
    for (r, c), B in blocks.items():
        Rf = Hinv[r * pd:(r + 1) * pd, c * pd:(c + 1) * pd]
        num += float(np.sum((B - Rf) ** 2))
        den += float(np.sum(Rf ** 2))
    print(f"marginals {np.sqrt(num / den):.2e}")
    assert np.sqrt(num / den) <= 1e-9


@pytest.mark.parametrize("pl_pl", [False, True])
def test_lm_pcg(g2o_amd_mod, pl_pl):
    prob = _ring(pl_pl)
    dev = _run(_device(g2o_amd_mod, prob), 4, "lm_pcg")
    _same_trajectory(dev, _run(_twin(g2o_amd_mod, prob), 4, "lm_pcg"), PCG_RTOL)


def test_refusals(g2o_amd_mod):
    mod = g2o_amd_mod
    for prob, algo in ((_ring(), "lm_hip_var"), (_sba(), "lm_hip_fix6_3")):
        dev = _device(mod, prob)
        dev.set_algorithm("lm_pcg6_3_eigen")
        with pytest.raises(mod.G2OHipError) as ei:
            dev.optimize(1)
        assert f"({ERR_UNSUPPORTED})" in str(ei.value) and "types_icp" in mod.last_error()
        dev.set_algorithm(algo)  # the graph is still usable
        n, st = dev.optimize(1)
        assert n == 1 and np.isfinite(st[0].chi2)
    one = I.one_edge(GICP)
    es = one.edges[0]

    def fresh(p):
        o = mod.SparseOptimizer(0)
        for vs in p.vertices:
            o.add_vertices(vs)
        return o
    # strides through the wrapper: measurement 12, covariances 12, VSC parameters 5
    for bad in (synth.EdgeSet(GICP, es.v0, es.v1, es.meas[:, :6], es.info, None),
                synth.EdgeSet(GICP, es.v0, es.v1, es.meas, es.info, np.zeros((1, 6)))):
        o = fresh(one)
        with pytest.raises(mod.G2OHipError) as ei:
            o.add_edges(bad)
        assert "12" in str(ei.value) and o.num_edges() == 0
    # no information: plane-to-plane only
    o = fresh(one)
    with pytest.raises(mod.G2OHipError) as ei:
        o.add_edges(synth.EdgeSet(GICP, es.v0, es.v1, es.meas, None, None))
    assert f"({ERR_ARG})" in str(ei.value) and o.num_edges() == 0
    # plane-to-plane holds for the whole set: edges with covariances do not join a point-to-plane set
    pl = I.one_edge(GICP, True).edges[0]
    o = fresh(one)
    o.add_edges(es)
    with pytest.raises(mod.G2OHipError) as ei:
        o.add_edges(synth.EdgeSet(GICP, es.v0, es.v1, es.meas, None, pl.params))
    assert f"({ERR_ARG})" in str(ei.value) and o.num_edges() == 1
    # VSC: NULL parameters, the wrong stride
    pv = I.one_edge(VSC)
    ev = pv.edges[0]
    o = fresh(pv)
    with pytest.raises(mod.G2OHipError) as ei:
        o.add_edges(synth.EdgeSet(VSC, ev.v0, ev.v1, ev.meas, ev.info, None))
    assert f"({ERR_ARG})" in str(ei.value) and o.num_edges() == 0
    with pytest.raises(mod.G2OHipError) as ei:
        o.add_edges(synth.EdgeSet(VSC, ev.v0, ev.v1, ev.meas, ev.info, np.zeros((1, 4))))
    assert "5" in str(ei.value) and o.num_edges() == 0
    # a VSC edge has no isDepthPositive
    d = _device(mod, _sba())
    d.initialize_optimization()
    with pytest.raises(mod.G2OHipError) as ei:
        d.edge_chi2(VSC, depth=True)
    assert f"({ERR_ARG})" in str(ei.value)
    # the switch takes 0 or 1
    assert mod.lib().g2ohip_set_pair_major(d.h, 2) == ERR_ARG


# ---------------------------------------------------------------- 9: gicp_sba (Edge_XYZ_VSC, the slot path, 6/3 Schur)
def test_gicp_sba_stage(g2o_amd_mod):
    prob = _sba()
    assert len(np.unique(prob.edges[1].params, axis=0)) == 1  # one shared record fx fy cx cy baseline
    opt = _device(g2o_amd_mod, prob)
    _stage_numpy("gicp_sba", opt, prob, pair_major=False)
    assert opt.stage(1e-3)["nl"] == 300  # 100 marginalised points
    # per-edge distinct camera records and informations
    rng = np.random.default_rng(9)
    ev = prob.edges[1]
    K = ev.params * (1.0 + 1e-3 * rng.standard_normal(ev.params.shape))
    es2 = synth.EdgeSet(VSC, ev.v0, ev.v1, ev.meas, I._spd3(rng, len(ev.v0)), K)
    p2 = synth.Problem("sba_distinct", prob.vertices, [prob.edges[0], es2], 6, 3)
    _stage_numpy("gicp_sba distinct records", _device(g2o_amd_mod, p2), p2, pair_major=False)
    delta = float(np.sqrt(np.median(I.Graph(prob).edge_chi2(VSC))))
    rb = {VSC: ("Huber", delta)}
    _stage_numpy("gicp_sba Huber", _device(g2o_amd_mod, prob, rb), prob, rb)


@pytest.mark.parametrize("algo", ["lm_hip_fix6_3", "lm_hip_var", "dl_hip_fix6_3"])
def test_gicp_sba_trajectory_against_twin(g2o_amd_mod, algo):
    prob = _sba()
    dev = _run(_device(g2o_amd_mod, prob), 4, algo)
    print(f"{algo}: chi2 {dev[1]} trials {dev[2]}")
    _same_trajectory(dev, _run(_twin(g2o_amd_mod, prob), 4, algo))
    assert dev[1][-1] < dev[1][0]


def test_gicp_sba_levels_chi2_classify(g2o_amd_mod):
    prob = _sba()
    opt = _device(g2o_amd_mod, prob)
    opt.initialize_optimization()
    ref = I.Graph(prob).edge_chi2(VSC, _est_of(opt, prob))
    chi = opt.edge_chi2(VSC)
    assert len(chi) == len(ref) and np.max(np.abs(chi - ref) / ref) <= 1e-12
    top = np.sort(ref)[len(ref) // 2:]
    k = int(np.argmax(np.diff(top)))
    thr = 0.5 * (top[k] + top[k + 1])
    bad = ref > thr
    counts = opt.classify_edges(VSC, thr)
    assert counts == dict(over_chi2=int(bad.sum()), depth_failed=0, bad=int(bad.sum())) and 0 < bad.sum() < len(bad)
    opt.initialize_optimization(0)
    _stage_numpy("sba after classify", opt, prob, levels={VSC: bad.astype(np.int32)})


def test_gicp_sba_structure_only_3(g2o_amd_mod):
    prob = _cached("sba_perturbed", lambda: structure_only_ref.perturbed(_sba(), 0.3))
    s = I.Structure(prob)
    ref_est, results = s.calc(10)
    opt = _device(g2o_amd_mod, prob)
    cams_before = opt.estimates(POSE)
    counts = opt.structure_only(iterations=10)
    print(f"device {counts} reference {structure_only_ref.counts(results)}")
    assert counts == structure_only_ref.counts(results) and counts["accepted"] > 0
    got, ref = opt.estimates(synth.V_XYZ), ref_est[synth.V_XYZ]
    worst = np.max(np.linalg.norm(got - ref, axis=1) / np.linalg.norm(ref, axis=1))
    print(f"worst landmark {worst:.2e}")
    assert worst <= RTOL
    assert np.array_equal(opt.estimates(POSE), cams_before)
    chi, chi_ref = opt.chi2(), s.graph_chi2(ref_est)
    assert abs(chi - chi_ref) <= RTOL * chi_ref
    # the algorithm name: optimize(1) is calc(points, 1)
    o2 = _device(g2o_amd_mod, prob)
    o2.set_algorithm("structure_only_3")
    n, st = o2.optimize(1)
    chi1 = s.graph_chi2(s.calc(1)[0])
    assert n == 1 and abs(st[0].chi2 - chi1) <= RTOL * chi1


def test_gicp_sba_two_local_ranks(g2o_amd_mod):
    prob = _sba()
    nranks, iters = 2, 4
    key = uuid.uuid4().hex
    opts = [_device(g2o_amd_mod, prob) for _ in range(nranks)]
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
    single = _device(g2o_amd_mod, prob)
    single.set_algorithm("lm_hip_fix6_3")
    n1, st1 = single.optimize(iters)
    for r in range(nranks):
        n, st = res[r]
        assert n == n1
        for a, b in zip(st, st1):
            assert a.levenbergIterations == b.levenbergIterations
            assert abs(a.chi2 - b.chi2) <= RTOL * b.chi2
    held = [len(o.local_landmark_ids()) for o in opts]
    assert all(h > 0 for h in held) and sum(held) == 100, held
    N, lm_ids = prob.vertices[0].ids.size, prob.vertices[1].ids
    states = [o.minimal_state() for o in opts]
    assert np.array_equal(states[1][:6 * N], states[0][:6 * N])
    x = states[0].copy()
    for r, o in enumerate(opts):
        k = np.searchsorted(lm_ids, o.local_landmark_ids())
        rows = (6 * N + 3 * k[:, None] + np.arange(3)[None, :]).ravel()
        x[rows] = states[r][rows]
    xs = single.minimal_state()
    assert np.linalg.norm(x - xs) <= 1e-9 * np.linalg.norm(xs)


# ---------------------------------------------------------------- 10: .g2o files
def test_g2o_round_trip(g2o_amd_mod, tmp_path):
    """EDGE_V_V_GICP: the file carries the 12 values; the loader rebuilds the information from normal0 as
    Edge_V_V_GICP::read does (prec0(0.01), which is what the generator set). Load, optimize, save, reload: same chi2."""
    prob = _ring()
    ne = len(prob.edges[0].v0)
    src = _device(g2o_amd_mod, prob)
    p1 = str(tmp_path / "a.g2o")
    src.save(p1)
    lines = open(p1).read().splitlines()
    tags = [ln.split()[0] for ln in lines]
    assert tags.count("EDGE_V_V_GICP") == ne
    assert len(next(ln for ln in lines if ln.startswith("EDGE_V_V_GICP")).split()) == 3 + 12
    back = g2o_amd_mod.SparseOptimizer(0)
    back.load(p1, icp=True)
    assert back.num_edges() == ne and back.num_vertices() == src.num_vertices()
    assert abs(back.chi2() - src.chi2()) <= 1e-12 * src.chi2()
    back.set_algorithm("lm_hip_var")
    back.optimize(3)
    assert back.pair_major_info()["pair_major"]
    p2 = str(tmp_path / "b.g2o")
    back.save(p2)
    assert [ln.split()[0] for ln in open(p2).read().splitlines()] == tags
    again = g2o_amd_mod.SparseOptimizer(0)
    again.load(p2, icp=True)
    assert abs(again.chi2() - back.chi2()) <= 1e-12 * back.chi2() and back.chi2() < src.chi2()
    plain = g2o_amd_mod.SparseOptimizer(0)
    plain.load(p1)  # without the flag the tag is skipped
    assert plain.num_edges() == 0 and plain.num_vertices() == src.num_vertices()
    # a hand-written line against numpy
    text = ("VERTEX_SE3:QUAT 0 0 0 0 0 0 0 1\nVERTEX_SE3:QUAT 1 0.1 0 1 0 0.6 0 0.8\nFIX 0\n"
            "EDGE_V_V_GICP 0 1 0.5 0.2 10 0.6 0 0.8 0.4 0.1 9.1 0.6 0 0.8\n")
    p3 = tmp_path / "hand.g2o"
    p3.write_text(text)
    hand = g2o_amd_mod.SparseOptimizer(0)
    hand.load(str(p3), icp=True)
    x = hand.estimates(POSE)
    m = np.array([[0.5, 0.2, 10, 0.6, 0, 0.8, 0.4, 0.1, 9.1, 0.6, 0, 0.8]])
    e = I.gicp_edge(x[:1], x[1:], m, jac=False)[0]
    ref = float(e @ g2o_amd_mod.gicp_prec([0.6, 0, 0.8], 0.01) @ e)
    assert abs(hand.chi2() - ref) <= 1e-12 * ref


def test_g2o_degenerate_normal_and_bad_lines(g2o_amd_mod, tmp_path):
    V = "VERTEX_SE3:QUAT 0 0 0 0 0 0 0 1\nVERTEX_SE3:QUAT 1 0 0 1 0 0 0 1\nVERTEX_XYZ 2 0 0 5\n"
    good = "EDGE_V_V_GICP 0 1 0.5 0.2 10 0 0 1 0.4 0.1 9 0 0 1\n"
    cases = [("degenerate normal", V + good + "EDGE_V_V_GICP 0 1 0.5 0.2 10 0 1 0 0.4 0.1 9 0 1 0\n", ("line 5", "(0,1,0)")),
             ("degenerate normal, down", V + "EDGE_V_V_GICP 0 1 0.5 0.2 10 0 -1 0 0.4 0.1 9 0 0 1\n", ("line 4",)),
             ("short line", V + "EDGE_V_V_GICP 0 1 0.5 0.2 10 0 0 1 0.4 0.1 9 0 0\n", ("EDGE_V_V_GICP",)),
             ("endpoint of the wrong type", V + "EDGE_V_V_GICP 0 2 0.5 0.2 10 0 0 1 0.4 0.1 9 0 0 1\n", ("vertex 2",)),
             ("missing endpoint", V + "EDGE_V_V_GICP 7 1 0.5 0.2 10 0 0 1 0.4 0.1 9 0 0 1\n", ("vertex 7",))]
    for name, text, names in cases:
        p = tmp_path / "bad.g2o"
        p.write_text(text)
        opt = g2o_amd_mod.SparseOptimizer(0)
        with pytest.raises(g2o_amd_mod.G2OHipError) as ei:
            opt.load(str(p), icp=True)
        assert f"({ERR_ARG})" in str(ei.value), name
        for w in names:
            assert w in g2o_amd_mod.last_error(), (name, w, g2o_amd_mod.last_error())
        assert opt.num_edges() <= 1  # nothing of the refused line is stored


def test_save_refuses_vsc(g2o_amd_mod, tmp_path):
    opt = _device(g2o_amd_mod, _sba())
    p = tmp_path / "no.g2o"
    with pytest.raises(g2o_amd_mod.G2OHipError) as ei:
        opt.save(str(p))
    assert f"({ERR_UNSUPPORTED})" in str(ei.value) and "Edge_XYZ_VSC" in g2o_amd_mod.last_error()
    assert not p.exists()
