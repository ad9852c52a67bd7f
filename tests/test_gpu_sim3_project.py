"""EdgeSim3ProjectXYZ and EdgeInverseSim3ProjectXYZ on the device (G2OHIP_E_SIM3_PROJECT_XYZ, ..._INVERSE_XYZ,
g2ohip_set_sim3_cameras, G2OHIP_LOAD_SIM3_PROJECT): FamilySim3Project through k_linearize_sim3_project / k_error /
k_classify and the dimension-7 slot reduction, both states of the shared intrinsics and information records, the
fix_scale column, robust kernels, levels and classification, marginals, update_initialization, mixing with EdgeSim3 and
host-Jacobian sets, .g2o files and the refusals.

Two references: tests/sim3_project_ref.py (plain numpy, pinned by tests/test_sim3_project_host.py) for chi2, the stage
level and marginals, and the same graph with the projection sets entered as G2OHIP_E_HOSTJ(2) edges whose host callback
returns sim3_project_ref's analytic [e | Ji | Jj] records (the twin) for the trajectories. The twin's stage is pinned
against numpy before it serves.

Tolerances are tests/test_gpu_sim3.py's own: chi2 against numpy 1e-12 relative, in total and per edge
(test_sim3_project_host.py keeps the float64 floor of the total under 1e-13 on every case, and of each edge on the
graphs and states where g2ohip_edge_chi2 is compared: the generators put every observation 3 to 6 px off), stage
level 1e-9 (b, x) and 1e-11 (H), trajectories 1e-6 relative with identical iteration and trial counts, marginals
tests/test_gpu_marginals.py's 1e-9, .g2o round trip 1e-12.
"""
import numpy as np
import pytest

import sim3_project_ref as P
import sim3_ref as S
from g2o_amd import synth
from test_gpu_sim3 import _run, _same_trajectory, _stage_against

pytestmark = pytest.mark.gpu

V, VP = S.V_SIM3, synth.V_XYZ
FWD, INV, HJ = P.E_FWD, P.E_INV, P.HJ2
ERR_ARG, ERR_UNSUPPORTED = -1, -4
HUBER = P.HUBER
_CACHE = {}  # cases and reference runs, computed once, shared, left unchanged


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _est_of(opt, prob):
    return {v.vtype: opt.estimates(v.vtype) for v in prob.vertices}


def _types(prob):
    return [es.etype for es in prob.edges if es.etype in P.TYPES]


def _set_cams(opt, cams):
    ids = sorted(cams)
    if ids:
        opt.set_sim3_cameras(ids, [cams[i][0] for i in ids], [cams[i][1] for i in ids])


def _device(mod, prob, cams, robust=None, fix_scale=False):
    opt = mod.SparseOptimizer(0).add_problem(prob)
    _set_cams(opt, cams)
    for t in _types(prob) if robust else ():
        opt.set_robust_kernel(t, *robust)
    if fix_scale:
        opt.set_sim3_fix_scale(True)
    return opt


def _twin(mod, prob, cams, robust=None, fix_scale=False):
    """The graph with the projection sets entered as one E_HOSTJ(2) set, sim3_project_ref's records in the callback."""
    g = P.Graph(prob, fix_scale, cams)
    opt = mod.SparseOptimizer(0).add_problem(P.twin_problem(prob))
    opt.set_host_edge_callback(lambda etype, with_jac: g.payload(_est_of(opt, prob)))
    if robust:
        opt.set_robust_kernel(HJ, *robust)
    if fix_scale:
        opt.set_sim3_fix_scale(True)
    return opt


def _rk(prob, robust):
    return {t: robust for t in _types(prob)} if robust else None


def _chi2_against(tag, opt, prob, cams, robust=None, fix_scale=False):
    ref = P.Graph(prob, fix_scale, cams).chi2(est=_est_of(opt, prob), robust=_rk(prob, robust))
    chi = opt.chi2()
    print(f"{tag} chi2 device {chi:.17g} numpy {ref:.17g} rel {abs(chi - ref) / ref:.2e}")
    assert ref > 0 and abs(chi - ref) <= 1e-12 * ref, (tag, chi, ref)


def _edge_chi2_against(tag, chi, ref):
    """Per-edge chi2 against numpy at the project's 1e-12 relative, on the graphs and states of
    sim3_project_ref.edge_chi2_states, whose per-edge float64 floor tests/test_sim3_project_host.py keeps under 1e-13."""
    worst = float(np.max(np.abs(chi - ref) / ref))
    print(f"{tag}: per-edge chi2 worst {worst:.2e}")
    assert len(chi) == len(ref) and worst <= 1e-12, (tag, worst)


def _stage_device(mod, tag, prob, cams, robust=None, fix_scale=False, twin=False):
    """The device (and with twin its host-J twin), each against numpy at the handle's own estimates."""
    who = [("device", _device(mod, prob, cams, robust, fix_scale))]
    if twin:
        who.append(("twin", _twin(mod, prob, cams, robust, fix_scale)))
    for name, opt in who:
        r = P.numpy_stage(prob, cams, None, _rk(prob, robust), _est_of(opt, prob), fix_scale)
        _stage_against(f"{name} {tag}", opt.stage(r["lam"]), r)
        if name == "device":
            _chi2_against(tag, opt, prob, cams, robust, fix_scale)
    return who[0][1]


def _opt_case(outliers=0):
    return _cached(("optsim3", outliers), lambda: P.optimize_sim3_case(outliers=outliers))


def _twin_run(mod, algo, robust=None, iters=4, outliers=0):
    prob, cams, _ = _opt_case(outliers)
    return _cached(("twinrun", algo, bool(robust), iters, outliers), lambda: _run(_twin(mod, prob, cams, robust), iters, algo))


# ---------------------------------------------------------------- 1: single-edge pins
@pytest.mark.parametrize("inverse", [False, True])
def test_single_edge_pins(g2o_amd_mod, inverse):
    prob, cams = P.one_edge(inverse)
    t = INV if inverse else FWD
    opt = _device(g2o_amd_mod, prob, cams)
    est = _est_of(opt, prob)
    g = P.Graph(prob, cams=cams)
    es = prob.edges[0]
    e = P.error(est[VP], est[V], es.meas, cams[9][int(inverse)], inverse)[0]
    ref = float(e @ es.info[0] @ e)
    _chi2_against(f"inverse={inverse}", opt, prob, cams)
    assert abs(opt.chi2() - ref) <= 1e-12 * ref
    opt.initialize_optimization()
    assert abs(opt.edge_chi2(t)[0] - ref) <= 1e-12 * ref
    # the error itself, sign included: the information e_k e_k^T picks one component's square, b = -Jj^T Omega e the sign
    for k in range(2):
        one = synth.Problem("pin", prob.vertices, [S._es(t, es.v0, es.v1, es.meas, np.outer(np.eye(2)[k], np.eye(2)[k])[None])], 7, 0)
        o = _device(g2o_amd_mod, one, cams)
        assert abs(o.chi2() - e[k] ** 2) <= 1e-12 * e[k] ** 2
    delta = 0.5 * np.sqrt(ref)  # sqrt(e2) > delta: Huber's linear branch, chi2 = rho
    opt.set_robust_kernel(t, "Huber", delta)
    rho = 2 * np.sqrt(ref) * delta - delta * delta
    assert abs(opt.chi2() - rho) <= 1e-12 * rho
    assert abs(g.chi2(est=est, robust={t: ("Huber", delta)}) - rho) <= 1e-12 * rho
    # the free Sim3 vertex's 7 x 7 block and b
    opt2 = _device(g2o_amd_mod, prob, cams)
    r = P.numpy_stage(prob, cams, None, est=est)
    s = opt2.stage(r["lam"])
    _stage_against(f"one edge inverse={inverse}", s, r)
    assert np.linalg.norm(s["b"] + r["b"]) > np.linalg.norm(r["b"])
    assert opt2.block_dims() == [7, 0, 1, 0]


# ---------------------------------------------------------------- 2: stage level at the kernel's edges
@pytest.mark.parametrize("ne", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("two_cams", [False, True])
@pytest.mark.parametrize("inverse", [False, True])
def test_stage_kernel_edges(g2o_amd_mod, inverse, two_cams, ne):
    """A partial wave, a full wave, a wave plus one edge, one edge past a 256-thread block; one shared intrinsics and
    information record (EdgeData::ue bits 0 and 1) or per-edge records with two vertices of other intrinsics. Every
    fourth edge ends in the fixed Sim3 vertex: its lane writes nothing."""
    prob, cams = P.kernel_case(ne, inverse, two_cams)
    opt = _stage_device(g2o_amd_mod, f"ne={ne} inverse={inverse} two_cams={two_cams}", prob, cams)
    # the all-edges view at these sizes: the fixed vertex's edges included, so the sum is the graph's chi2
    chi = opt.edge_chi2(INV if inverse else FWD)
    total = opt.chi2()
    assert len(chi) == ne and abs(float(np.sum(chi)) - total) <= 1e-12 * total


# ---------------------------------------------------------------- 3: OptimizeSim3's shape
def test_optimize_sim3_stage_and_twin_pin(g2o_amd_mod):
    prob, cams, _ = _opt_case()
    opt = _stage_device(g2o_amd_mod, "OptimizeSim3", prob, cams, twin=True)
    assert opt.block_dims() == [7, 0, 1, 0]


@pytest.mark.parametrize("algo", ["lm_hip_fix7_3", "gn_hip_fix7_3", "dl_hip_fix7_3", "lm_hip_var", "gn_hip_var", "dl_hip_var"])
def test_optimize_sim3_against_twin(g2o_amd_mod, algo):
    prob, cams, _ = _opt_case()
    dev = _run(_device(g2o_amd_mod, prob, cams), 4, algo)
    print(f"{algo}: chi2 {dev[1]} trials {dev[2]}")
    _same_trajectory(dev, _twin_run(g2o_amd_mod, algo))
    assert dev[0] == 4 and dev[1][-1] < dev[1][0]


# ---------------------------------------------------------------- 4: Huber, fix_scale
def test_huber(g2o_amd_mod):
    """On the case with six corrupted observations: they sit on Huber's linear branch, the rest on the quadratic one."""
    prob, cams, corrupted = _opt_case(6)
    est = {v.vtype: (S.normalized(v.est) if v.vtype == V else v.est) for v in prob.vertices}
    g = P.Graph(prob, cams=cams)
    chi = np.concatenate([g.project_chi2(t, est) for t in P.TYPES])
    assert np.all(chi[corrupted] > 5.991) and np.mean(chi < 5.991) > 0.5  # both branches are taken at the start
    _stage_device(g2o_amd_mod, "Huber", prob, cams, HUBER, twin=True)
    dev = _run(_device(g2o_amd_mod, prob, cams, HUBER), 4, "lm_hip_fix7_3")
    print(f"Huber: chi2 {dev[1]} trials {dev[2]}")
    _same_trajectory(dev, _twin_run(g2o_amd_mod, "lm_hip_fix7_3", HUBER, outliers=6))
    plain = _twin_run(g2o_amd_mod, "lm_hip_fix7_3", outliers=6)
    assert abs(dev[1][0] - plain[1][0]) > 1e-3 * plain[1][0]  # the kernel is at work: another trajectory


def test_huber_fix_scale(g2o_amd_mod):
    """_fix_scale zeroes column 6 of the inverse edges' Jj (the forward edges' is zero in any state): H(6, 6) holds
    lambda alone and b[6] = 0; LM's lambda keeps the solve definite."""
    prob, cams, _ = _opt_case(6)
    _stage_device(g2o_amd_mod, "Huber fix_scale", prob, cams, HUBER, fix_scale=True, twin=True)
    s = _device(g2o_amd_mod, prob, cams, HUBER, fix_scale=True).stage(1.0)
    H = s["Hschur"] - np.eye(7)
    assert not H[6].any() and not H[:, 6].any() and s["b"][6] == 0 and H.any()
    free = _device(g2o_amd_mod, prob, cams, HUBER).stage(1.0)
    assert free["Hschur"][6, 6] > 2.0 and free["b"][6] != 0
    opt = _device(g2o_amd_mod, prob, cams, HUBER, fix_scale=True)
    s0 = opt.estimates(V)[0, 7]
    dev = _run(opt, 4, "lm_hip_fix7_3")
    _same_trajectory(dev, _run(_twin(g2o_amd_mod, prob, cams, HUBER, fix_scale=True), 4, "lm_hip_fix7_3"))
    assert opt.estimates(V)[0, 7] == s0 and dev[1][-1] < dev[1][0]


def test_every_robust_kernel(g2o_amd_mod):
    prob, cams, _ = _opt_case()
    for kind in ("PseudoHuber", "Cauchy", "GemanMcClure", "Welsch", "Fair", "Tukey", "Saturated", "DCS"):
        _stage_device(g2o_amd_mod, kind, prob, cams, (kind, 4.0))


# ---------------------------------------------------------------- 5: the outlier loop on the handle
def test_outlier_loop(g2o_amd_mod):
    """OptimizeSim3's loop: optimise under Huber, set the edges over chi2 = 9.21 aside by classify_edges, initialise
    level 0 again and optimise what is left. The twin takes its levels from the numpy reference's decisions."""
    mod = g2o_amd_mod
    prob, cams, corrupted = _opt_case(6)
    n = len(prob.edges[0].v0)
    opt = _device(mod, prob, cams, HUBER)
    first = _run(opt, 5, "lm_hip_fix7_3")
    est = _est_of(opt, prob)
    g = P.Graph(prob, cams=cams)
    bad = {}
    for t in P.TYPES:
        ref = g.project_chi2(t, est)
        chi = opt.edge_chi2(t)
        print(f"type {t}: nearest to 9.21 {np.min(np.abs(ref - 9.21)) / 9.21:.2e}")
        _edge_chi2_against(f"type {t}", chi, ref)
        assert len(chi) == n
        assert np.min(np.abs(ref - 9.21)) > 1e-6 * 9.21  # no decision hangs on rounding
        bad[t] = ref > 9.21
        counts = opt.classify_edges(t, 9.21)
        assert counts == dict(over_chi2=int(bad[t].sum()), depth_failed=0, bad=int(bad[t].sum()))
        assert np.array_equal(opt.edge_levels(t), bad[t].astype(np.int32))
    found = np.concatenate([bad[FWD], bad[INV]])
    assert np.all(found[corrupted]) and found.sum() < n  # the corrupted ones and at most a few more, not the set
    opt.initialize_optimization(0)
    kept = P.without(prob, bad)
    _chi2_against("inliers", opt, kept, cams, HUBER)
    second = _run(opt, 5)
    tw = _twin(mod, prob, cams, HUBER)
    tfirst = _run(tw, 5, "lm_hip_fix7_3")
    _same_trajectory(first, tfirst)
    tw.set_edge_levels(HJ, found.astype(np.int32))
    tw.initialize_optimization(0)
    tsecond = _run(tw, 5)
    _same_trajectory(second, tsecond)
    assert abs(second[1][-1] - tsecond[1][-1]) <= 1e-6 * tsecond[1][-1] and second[1][-1] < first[1][-1]


# ---------------------------------------------------------------- 6: mixed with EdgeSim3 and host-J sets
def test_mixed_graph(g2o_amd_mod):
    """EdgeSim3 between the vertices, projection edges of both types onto four of them (one fixed, with the default
    intrinsics 1 1 0 0); in the twin the projections are a host-J set beside the device's EdgeSim3 set."""
    prob, cams = _cached("mixed", P.mixed_case)
    _stage_device(g2o_amd_mod, "mixed", prob, cams, twin=True)
    dev = _run(_device(g2o_amd_mod, prob, cams), 4, "lm_hip_fix7_3")
    print(f"mixed: chi2 {dev[1]} trials {dev[2]}")
    _same_trajectory(dev, _run(_twin(g2o_amd_mod, prob, cams), 4, "lm_hip_fix7_3"))
    assert dev[1][-1] < dev[1][0]


# ---------------------------------------------------------------- 7: intrinsics
def test_set_sim3_cameras_after_optimize(g2o_amd_mod):
    """A change of intrinsics after the edges are on the device reaches chi2, the per-edge chi2 and the system."""
    prob, cams, _ = _opt_case()
    opt = _device(g2o_amd_mod, prob, cams)
    opt.set_algorithm("lm_hip_fix7_3")
    opt.optimize(2)
    _chi2_against("before", opt, prob, cams)
    before = opt.chi2()
    opt.edge_chi2(FWD)  # the all-edges view exists: it must follow too
    new = {48: P.NEW_CAMS}
    opt.set_sim3_cameras([48], cam1=new[48][0])
    half = {48: (new[48][0], cams[48][1])}
    _chi2_against("camera 1", opt, prob, half)
    opt.set_sim3_cameras([48], cam2=new[48][1])
    _chi2_against("both", opt, prob, new)
    assert abs(opt.chi2() - before) > 1e-3 * before
    g = P.Graph(prob, cams=new)
    est = _est_of(opt, prob)
    for t in P.TYPES:
        _edge_chi2_against(f"new intrinsics type {t}", opt.edge_chi2(t), g.project_chi2(t, est))
    r = P.numpy_stage(prob, new, None, est=est)
    _stage_against("new intrinsics", opt.stage(r["lam"]), r)
    chi_new = opt.chi2()
    n, st = opt.optimize(2)
    assert n == 2 and st[-1].chi2 < chi_new


# ---------------------------------------------------------------- 8: marginals, update_initialization
def test_marginals(g2o_amd_mod):
    prob, cams, _ = _opt_case()
    opt = _device(g2o_amd_mod, prob, cams)
    opt.set_algorithm("lm_hip_fix7_3")
    opt.initialize_optimization()
    opt.build_structure()
    opt.build_system()
    H = P.numpy_stage(prob, cams, 0.0, est=_est_of(opt, prob))["H"]
    blocks = opt.compute_marginals([(0, 0)])
    assert blocks is not None and list(blocks) == [(0, 0)]
    Rf = np.linalg.inv(H)
    err = np.linalg.norm(blocks[(0, 0)] - Rf) / np.linalg.norm(Rf)
    print(f"marginals {err:.2e}")
    assert err <= 1e-9


def test_update_initialization(g2o_amd_mod):
    """The inverse set arrives after a first optimisation of the forward one."""
    prob, cams, _ = _opt_case()
    first = synth.Problem("fwd", prob.vertices, prob.edges[:1], 7, 0)
    opt = _device(g2o_amd_mod, first, cams)
    opt.set_algorithm("lm_hip_fix7_3")
    opt.optimize(1)
    opt.add_edges(prob.edges[1])
    opt.update_initialization()
    _chi2_against("joined", opt, prob, cams)
    r = P.numpy_stage(prob, cams, None, est=_est_of(opt, prob))
    _stage_against("joined", opt.stage(r["lam"]), r)


# ---------------------------------------------------------------- 9: .g2o files
def test_g2o_round_trip(g2o_amd_mod, tmp_path):
    mod = g2o_amd_mod
    prob, cams, _ = _opt_case()
    a = _device(mod, prob, cams)
    a.set_algorithm("lm_hip_fix7_3")
    a.optimize(1)  # the state that is written is the device's
    path = str(tmp_path / "proj.g2o")
    a.save(path)
    text = open(path).read()
    assert all(text.count(P.TAGS[t] + " ") == 24 for t in P.TYPES) and text.count("FIX ") == 48
    back = P.parse_edge_lines(text)
    for es in prob.edges:  # the reference's way: u v and the upper triangle, shortest round-trip decimals
        assert np.array_equal(back[es.etype][2], es.meas) and np.array_equal(np.triu(back[es.etype][3]), np.triu(es.info))
    b = mod.SparseOptimizer(0)
    b.load(path, marginalize_xyz=False, sim3=True, sim3_project=True)
    b.set_sim3_cameras([48], cam2=cams[48][1])  # no line carries camera 2; camera 1 came with the vertex line
    assert b.num_vertices() == 49 and b.num_edges() == 48
    ea, eb = a.estimates(V), b.estimates(V)
    ea[:, 3:7] *= np.where(ea[:, 6:7] < 0, -1.0, 1.0)  # (the reader's inverse brings w >= 0: the same rotation)
    err = np.max(np.abs(ea - eb)) / np.max(np.abs(ea))
    print(f"state after save -> load: {err:.2e}")
    assert err <= 1e-12 and np.array_equal(a.estimates(VP), b.estimates(VP))
    ca, cb = a.chi2(), b.chi2()
    print(f"chi2 {ca:.17g} {cb:.17g}")
    assert abs(ca - cb) <= 1e-12 * ca
    # a file in the reference's text loads to the same graph
    ref_path = str(tmp_path / "ref.g2o")
    with open(ref_path, "w") as f:
        f.write(P.g2o_text(prob, cams))
    c = mod.SparseOptimizer(0)
    c.load(ref_path, marginalize_xyz=False, sim3=True, sim3_project=True)
    c.set_sim3_cameras([48], cam2=cams[48][1])
    fresh = _device(mod, prob, cams)
    assert np.max(np.abs(c.estimates(V) - fresh.estimates(V))) <= 1e-12 * np.max(np.abs(fresh.estimates(V)))
    assert abs(c.chi2() - fresh.chi2()) <= 1e-12 * fresh.chi2()
    for t in P.TYPES:
        assert np.array_equal(c.edge_levels(t), np.zeros(24, np.int32))
    # without camera 2 the inverse edges see the default 1 1 0 0
    d = mod.SparseOptimizer(0)
    d.load(ref_path, marginalize_xyz=False, sim3=True, sim3_project=True)
    _chi2_against("default camera 2", d, prob, {48: (cams[48][0], P.DEFAULT_CAM)})
    # without sim3_project the edges are absent and nothing fails: what sim3=True alone does is unchanged
    e = mod.SparseOptimizer(0)
    e.load(ref_path, marginalize_xyz=False, sim3=True)
    assert e.num_vertices() == 49 and e.num_edges() == 0
    # marginalised points: the graph loads, initialisation refuses it
    m = mod.SparseOptimizer(0)
    with open(str(tmp_path / "free.g2o"), "w") as f:
        f.write("\n".join(l for l in P.g2o_text(prob, cams).splitlines() if l != "FIX 3") + "\n")
    m.load(str(tmp_path / "free.g2o"), marginalize_xyz=True, sim3=True, sim3_project=True)
    with pytest.raises(mod.G2OHipError) as ei:
        m.initialize_optimization()
    assert f"({ERR_UNSUPPORTED})" in str(ei.value) and "7/3 Schur kernels do not exist" in str(ei.value)
    # bad lines fail the load and name the tag
    head = "VERTEX_XYZ 0 0.1 0.2 4\nVERTEX_XYZ 1 0.3 0.1 5\nVERTEX_SIM3:EXPMAP 2 0 0 0 0 0 0 0 400 400 320 240\n"
    for tag in P.TAGS.values():
        for body in (f"{tag} 0 2 1.5 2.5 1 0\n",           # short: one information value missing
                     f"{tag} 2 0 1.5 2.5 1 0 1\n",         # v0 is no VERTEX_XYZ
                     f"{tag} 0 1 1.5 2.5 1 0 1\n",         # v1 is no VERTEX_SIM3:EXPMAP
                     f"{tag} 0 7 1.5 2.5 1 0 1\n"):        # v1 is missing
            bad = str(tmp_path / "bad.g2o")
            with open(bad, "w") as f:
                f.write(head + body)
            with pytest.raises(mod.G2OHipError) as ei:
                mod.SparseOptimizer(0).load(bad, marginalize_xyz=False, sim3=True, sim3_project=True)
            assert f"({ERR_ARG})" in str(ei.value) and tag in str(ei.value), (body, str(ei.value))
            ok = mod.SparseOptimizer(0)
            ok.load(bad, marginalize_xyz=False, sim3=True)  # skipped without the flag
            assert ok.num_edges() == 0


# ---------------------------------------------------------------- 10: refusals and arguments
def test_refusals_and_arguments(g2o_amd_mod):
    mod = g2o_amd_mod
    prob, cams, _ = _opt_case()

    def refused(call, code, *words):
        with pytest.raises(mod.G2OHipError) as ei:
            call()
        msg = str(ei.value)
        assert (code is None or f"({code})" in msg) and all(w in msg for w in words), msg

    def with_point(marg):
        fx = np.ones(48, np.int32)
        fx[5] = 0
        pts = prob.vertices[0]
        mg = np.zeros(48, np.int32)
        mg[5] = marg
        return synth.Problem("free point", [synth.VertexSet(VP, pts.ids, pts.est, fx, mg), prob.vertices[1]], prob.edges,
                             7, 3 if marg else 0)

    # a free marginalised point under a type-28 edge: today's 7/3 message; a free non-marginalised one: one pose block size
    opt = _device(mod, with_point(1), cams)
    refused(opt.initialize_optimization, ERR_UNSUPPORTED, "7/3 Schur kernels do not exist")
    opt = _device(mod, with_point(0), cams)
    refused(opt.initialize_optimization, ERR_UNSUPPORTED, "one pose block size")
    # the iterative solvers take no blocks of 7
    opt = _device(mod, prob, cams)
    opt.set_algorithm("lm_pcg6_3_eigen")
    refused(opt.build_structure, ERR_UNSUPPORTED, "blocks of 7")
    for t, es in zip(P.TYPES, prob.edges):
        # params must be NULL
        opt = mod.SparseOptimizer(0)
        for vs in prob.vertices:
            opt.add_vertices(vs)
        refused(lambda: opt.add_edges(synth.EdgeSet(t, es.v0, es.v1, es.meas, es.info, np.zeros((24, 4)))), ERR_ARG)
        refused(lambda: opt.add_edges(synth.EdgeSet(t, es.v0, es.v1, es.meas[:, :1], es.info)), None,
                "2 measurement values")  # (the wrapper's own stride checks)
        refused(lambda: opt.add_edges(synth.EdgeSet(t, es.v0, es.v1 + 1, es.meas, es.info)), ERR_ARG)  # an unknown vertex
        assert opt.num_edges() == 0
        # wrong endpoint types: the error the other types give, at initialisation
        for v0, v1 in ((es.v1, es.v1), (es.v0, es.v0)):  # a Sim3 vertex in the point's place, a point in the Sim3's
            wrong = synth.Problem("wrong", prob.vertices, [S._es(t, v0[:1], v1[:1], es.meas[:1], es.info[:1])], 7, 0)
            o = mod.SparseOptimizer(0).add_problem(wrong)
            refused(o.initialize_optimization, ERR_UNSUPPORTED, f"edge type {t} on vertex {v0[0]} of vertex type")
        # no isDepthPositive in the reference
        opt = _device(mod, prob, cams)
        opt.initialize_optimization()
        refused(lambda: opt.edge_chi2(t, depth=True), ERR_ARG, "isDepthPositive")
        refused(lambda: opt.classify_edges(t, 9.21, check_depth=True), ERR_ARG, "isDepthPositive")
    # set_sim3_cameras: an id that is no Sim3 vertex changes nothing
    opt = _device(mod, prob, cams)
    before = opt.chi2()
    other = [(1.0, 2.0, 3.0, 4.0)] * 2
    refused(lambda: opt.set_sim3_cameras([48, 7], other, other), ERR_ARG)   # 7 is a point
    refused(lambda: opt.set_sim3_cameras([48, 999], other, other), ERR_ARG)  # 999 is unknown
    assert opt.chi2() == before
    opt.set_sim3_cameras([48])  # neither camera given: nothing to do
    assert opt.chi2() == before
    assert mod.lib().g2ohip_set_sim3_cameras(opt.h, 1, None, None, None) == ERR_ARG
