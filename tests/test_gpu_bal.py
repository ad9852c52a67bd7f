"""BAL problems on the device (G2OHIP_V_CAM_BAL, G2OHIP_E_OBSERVATION_BAL, 9 x 9 camera blocks, the 9/3 Schur
complement, g2ohip_load_bal / g2ohip_save_bal): FamilyBAL through k_linearize's two-pass camera slot and k_error, the
dimension-9 vertex reduction in every lane class, k_schur_diag / k_schur_rows / k_backsub at (9, 3) with the padded G
stride, LM, Gauss-Newton and dogleg trajectories, levels and classification, marginals, files and the refusals.

One reference: tests/bal_ref.py (plain numpy, pinned on the host by tests/test_bal_host.py). No host-Jacobian twin
exists for a vertex of dimension 9, so the trajectories are compared with numpy's own LM / Gauss-Newton / dogleg loops
(bal_ref.lm, bal_ref.gn, dogleg_ref) over the dense system.

Tolerances are tests/test_gpu_sim3.py's: chi2 against numpy 1e-12 relative (test_bal_host.py measures a float64 floor of
8e-15 in total and 6e-14 per edge on every graph and state where it is compared), stage level 1e-11 (H) and 1e-9 (b, x; 64 x the measured float64
floor of x on the one graph where it is above 1e-11, bal1p: bal_ref.X_FLOOR), trajectories 1e-6 relative with identical
iteration and trial counts, linear residual 1e-9, marginals 1e-9, files bitwise.
"""
import uuid

import numpy as np
import pytest

import bal_ref as B
import dogleg_ref
from g2o_amd import synth

pytestmark = pytest.mark.gpu

RTOL = 1e-6
V, P, E = B.V_CAM, B.V_XYZ, B.E
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
    if robust:
        opt.set_robust_kernel(E, *robust)
    return opt


def _stage_against(tag, s, r, xtol=1e-9):
    assert s["ok"] == 1 and (s["n"], s["np"]) == (r["n"], r["np"]), (tag, s["n"], s["np"], r["n"], r["np"])
    for k, tol in (("b", 1e-9), ("x", xtol), ("bschur", 1e-9)):
        err = np.linalg.norm(s[k] - r[k]) / np.linalg.norm(r[k])
        print(f"{tag} {k}: {err:.2e}")
        assert err <= tol, (tag, k, err)
    err = np.linalg.norm(s["Hschur"] - r["Hschur"]) / np.linalg.norm(r["Hschur"])
    print(f"{tag} H: {err:.2e}")
    assert err <= 1e-11, (tag, err)


def _stage(mod, prob, robust=None):
    """The device against numpy at the handle's own estimates: chi2, b, x, Hschur, bschur."""
    opt = _device(mod, prob, robust)
    est = _est_of(opt, prob)
    r = B.numpy_stage(prob, None, robust, est)
    _stage_against(prob.name, opt.stage(r["lam"]), r, B.x_tolerance(prob))
    ref = B.Graph(prob).chi2(est=est, robust={E: robust} if robust else None)
    chi = opt.chi2()
    assert abs(chi - ref) <= 1e-12 * ref, (prob.name, chi, ref)
    return opt, r


def _run(opt, iters, algo):
    opt.set_algorithm(algo)
    n, st = opt.optimize(iters)
    return n, [s.chi2 for s in st], [s.levenbergIterations for s in st], opt.minimal_state()


# ---------------------------------------------------------------- 1: single-edge pins
@pytest.mark.parametrize("free_camera", [True, False])
def test_single_edge_pins(g2o_amd_mod, free_camera):
    """One free camera and one fixed point; then one fixed camera and one free marginalised point (BlockSolver needs a
    free non-marginalised vertex, so a second, free camera sees the point too: bal_ref.one_edge)."""
    prob = B.one_edge(free_camera)
    opt = _device(g2o_amd_mod, prob)
    est = _est_of(opt, prob)
    g = B.Graph(prob)
    ref = g.chi2(est=est)
    chi = opt.chi2()
    print(f"chi2 device {chi:.17g} numpy {ref:.17g} rel {abs(chi - ref) / ref:.2e}")
    assert ref > 0 and abs(chi - ref) <= 1e-12 * ref
    opt.initialize_optimization()
    per = opt.edge_chi2(E)
    assert np.max(np.abs(per - g.edge_chi2(est)) / g.edge_chi2(est)) <= 1e-12
    # each error component with its sign: under the information e_k e_k^T the chi2 is e[k]^2, and b = -J^T e_k e[k]
    es = prob.edges[0]
    n = len(es.v0)
    cams, pts = est[V][np.searchsorted(prob.vertices[0].ids, es.v0)], est[P][np.searchsorted(prob.vertices[1].ids, es.v1)]
    e = B.error(cams, pts, es.meas)
    for k in range(2):
        info = np.zeros((n, 2, 2))
        info[:, k, k] = 1.0
        pk = synth.Problem(prob.name + f"/e{k}", prob.vertices, [B._es(E, es.v0, es.v1, es.meas, info)], 9, prob.landmark_dim)
        ok = _device(g2o_amd_mod, pk)
        ok.initialize_optimization()
        got = ok.edge_chi2(E)
        assert np.max(np.abs(got - e[:, k] ** 2) / e[:, k] ** 2) <= 1e-12, (k, got, e[:, k] ** 2)
        r = B.numpy_stage(pk, 1.0, est=est)
        s = ok.stage(1.0)
        assert np.linalg.norm(s["b"] - r["b"]) <= 1e-9 * np.linalg.norm(r["b"])
        assert np.linalg.norm(s["b"] + r["b"]) > np.linalg.norm(r["b"])  # the sign
    # Huber's linear branch: sqrt(e2) > delta on every edge, chi2 = rho
    c = g.edge_chi2(est)
    delta = B.pin_huber(prob)[1]
    assert delta < float(np.sqrt(c.min()))
    opt.set_robust_kernel(E, "Huber", delta)
    rho = float(np.sum(2 * np.sqrt(c) * delta - delta * delta))
    assert abs(opt.chi2() - rho) <= 1e-12 * rho
    assert abs(g.chi2(est=est, robust={E: ("Huber", delta)}) - rho) <= 1e-12 * rho
    # the 9 x 9 block (beside the point's 3 x 3 through the Schur complement) and b against numpy
    opt2, r = _stage(g2o_amd_mod, prob)
    assert opt2.block_dims() == ([9, 0, 1, 0] if free_camera else [9, 3, 1, 1])
    assert r["Hschur"].shape == (9, 9)
    _stage(g2o_amd_mod, prob, ("Huber", delta))
    # the estimate goes in and comes out as 9 doubles, untouched; the minimal state is the same values in id order
    assert np.array_equal(opt.estimates(V), prob.vertices[0].est)
    assert np.array_equal(opt.minimal_state(), np.concatenate([prob.vertices[0].est.ravel(), prob.vertices[1].est.ravel()]))


def test_theta_zero_camera(g2o_amd_mod):
    """A camera whose rotation vector is exactly zero takes the reference's Taylor branch: P = X + w x X,
    dP/dw = -[X]x."""
    prob = B.one_edge(True, 0.0)
    assert not prob.vertices[0].est[0, :3].any()
    opt, r = _stage(g2o_amd_mod, prob)
    assert np.linalg.norm(r["b"][:3]) > 0  # the rotation columns of the Taylor branch are at work
    # one LM step moves the rotation off zero, into the other branch (the single observation is then met: its residual
    # is near zero, where no chi2 is compared)
    chi0 = opt.chi2()
    n, chi, trials, x = _run(opt, 1, "lm_hip_fix9_3")
    assert n == 1 and trials == [1] and opt.estimates(V)[0, :3].any() and chi[0] < 1e-3 * chi0


# ---------------------------------------------------------------- 2: linearize at the kernel's edges
@pytest.mark.parametrize("ne", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("uniform", [True, False])
def test_stage_kernel_edges(g2o_amd_mod, uniform, ne):
    """A partial wave, a full wave (both 32-lane passes of the camera slot), a wave plus one edge, one edge past a
    256-thread block; one shared information record (EdgeData::ue bit 0) and per-edge records; one camera and one point
    fixed among the endpoints (nothing is written for them)."""
    _stage(g2o_amd_mod, B.kernel_case(ne, uniform))


def test_stage_huber(g2o_amd_mod):
    prob = B.kernel_case(65, False)
    _stage(g2o_amd_mod, prob, B.median_huber(prob))  # half of the edges on the linear branch


# ---------------------------------------------------------------- 3: vertex reduce at dimension 9
@pytest.mark.parametrize("which", ["lt6", "6to15", "16to127", "ge128"])
def test_vertex_reduce_lane_classes(g2o_amd_mod, which):
    """Average camera degree under 6 (one lane per vertex), 6 - 15 (4), 16 - 127 (8) and >= 128 (k_vertex_reduce<9, 64>:
    the wide kernel's half-wave cannot hold the 54-double slot)."""
    prob = B.degree_case(which)
    deg = len(prob.edges[0].v0) / len(prob.vertices[0].ids)
    lo, hi = {"lt6": (0, 6), "6to15": (6, 16), "16to127": (16, 128), "ge128": (128, 1e9)}[which]
    assert lo <= deg < hi
    _stage(g2o_amd_mod, prob)


# ---------------------------------------------------------------- 4: the 9/3 Schur complement
@pytest.mark.parametrize("which", ["1", "64", "65", "257", "neighbours", "260"])
def test_schur_9_3(g2o_amd_mod, which):
    """Camera rows of 1, 64, 65 and 257 observations (k_schur_diag's wave loop: a partial wave, a full one, one block
    more, a second pass of the workgroup), one camera with 69 off-diagonal neighbours (more than SCHUR_SL = 64: two row
    tasks), a row whose 520 staged blocks exceed one 128-block batch."""
    prob = B.schur_case(which)
    opt, r = _stage(g2o_amd_mod, prob)
    nc, npt = len(prob.vertices[0].ids), len(prob.vertices[1].ids)
    assert opt.block_dims() == [9, 3, nc, npt]
    opt.set_algorithm("lm_hip_fix9_3")
    opt.initialize_optimization()
    opt.build_structure()
    opt.build_system()
    opt.set_lambda(r["lam"])
    assert opt.solve()
    res = opt.linear_residual()
    print(f"{prob.name}: linear residual {res:.2e}")
    assert res <= 1e-9
    assert np.linalg.norm(opt.x() - r["x"]) <= B.x_tolerance(prob) * np.linalg.norm(r["x"])


# ---------------------------------------------------------------- 5: trajectories
def _reference_run(algo, fixed, robust=None, iters=5):
    def make():
        d = B.Dense(B.trajectory_case(fixed), robust=robust)
        if algo == "lm":
            out = B.lm(d, iters)
            return [c for c, _, _ in out], [t for _, t, _ in out], d.minimal_state()
        if algo == "gn":
            out = B.gn(d, iters)
            return out, [0] * len(out), d.minimal_state()
        n, its = dogleg_ref.optimize(d, iters)
        return its, [i.tries for i in its], d.minimal_state()
    return _cached(("ref", algo, fixed, bool(robust), iters), make)


def _same_as_reference(dev, ref, trials=True):
    n, chi, tr, x = dev
    rchi, rtr, rx = ref
    assert n == len(rchi) and (not trials or tr == rtr), (n, tr, rtr)
    for a, b in zip(chi, rchi):
        assert abs(a - b) <= RTOL * abs(b), (a, b)
    assert np.linalg.norm(x - rx) <= RTOL * np.linalg.norm(rx), np.linalg.norm(x - rx) / np.linalg.norm(rx)


@pytest.mark.parametrize("algo,fixed", [("lm_hip_fix9_3", ()), ("lm_hip_var", ()), ("lm_hip_fix9_3", (0,)), ("lm_hip_var", (0,)),
                                        ("gn_hip_fix9_3", (0, 1))])
def test_trajectory(g2o_amd_mod, algo, fixed):
    """No vertex fixed, as bal_example runs, and camera 0 fixed, under LM; Gauss-Newton with the camera pair fixed that
    holds the gauge (it solves without damping; its levenbergIterations are 0, as the reference's)."""
    prob = B.trajectory_case(fixed)
    dev = _run(_device(g2o_amd_mod, prob), 5, algo)
    print(f"{algo} fixed {fixed}: chi2 {dev[1]} trials {dev[2]}")
    _same_as_reference(dev, _reference_run(algo[:2], fixed))
    assert dev[0] == 5 and dev[1][-1] < dev[1][0]


def test_trajectory_dogleg(g2o_amd_mod):
    """dl_hip_fix9_3 with the camera pair fixed, one g2ohip_optimize_step at a time: chi2, the trial count, the last
    step's kind and delta after every iteration against dogleg_ref (the second iteration takes 12 trials)."""
    fixed = (0, 1)
    its, tries, rx = _reference_run("dl", fixed)
    opt = _device(g2o_amd_mod, B.trajectory_case(fixed))
    opt.set_algorithm("dl_hip_fix9_3")
    assert len(its) == 5 and max(tries) > 1
    for k, it in enumerate(its):
        r, st = opt.optimize_step(k)
        s = opt.dogleg_state()
        print(f"it {k}: chi2 {st.chi2:.12g} state {s} | reference chi2 {it.chi2:.12g} tries {it.tries} step {it.last_step} "
              f"delta {it.delta:.9g}")
        assert r == 0 and it.result == dogleg_ref.OK
        assert abs(st.chi2 - it.chi2) <= RTOL * it.chi2, (k, st.chi2, it.chi2)
        assert s["tries"] == it.tries and s["step"] == it.last_step, (k, s, it.tries, it.last_step)
        assert abs(s["delta"] - it.delta) <= RTOL * it.delta, (k, s["delta"], it.delta)
        assert s["was_pd"] == it.was_pd and st.levenbergIterations == 0
    x = opt.minimal_state()
    assert np.linalg.norm(x - rx) <= RTOL * np.linalg.norm(rx), np.linalg.norm(x - rx) / np.linalg.norm(rx)
    assert its[-1].chi2 < its[0].chi2_before


def test_trajectory_huber(g2o_amd_mod):
    prob = B.trajectory_case(())
    dev = _run(_device(g2o_amd_mod, prob, B.HUBER), 5, "lm_hip_fix9_3")
    print(f"Huber: chi2 {dev[1]} trials {dev[2]}")
    _same_as_reference(dev, _reference_run("lm", (), B.HUBER))
    plain = _reference_run("lm", ())
    assert abs(dev[1][0] - plain[0][0]) > 1e-3 * plain[0][0]  # the kernel is at work: another trajectory


def test_two_runs_bitwise(g2o_amd_mod):
    prob = B.trajectory_case(())
    a, b = (_run(_device(g2o_amd_mod, prob), 4, "lm_hip_fix9_3") for _ in range(2))
    assert a[1] == b[1] and a[2] == b[2] and np.array_equal(a[3], b[3])


# ---------------------------------------------------------------- 6: levels and classification
def test_levels_chi2_classify(g2o_amd_mod):
    prob, bad = B.outlier_case()
    opt = _device(g2o_amd_mod, prob)
    opt.initialize_optimization()
    ref = B.Graph(prob).edge_chi2(_est_of(opt, prob))
    chi = opt.edge_chi2(E)
    print(f"per-edge chi2 worst {np.max(np.abs(chi - ref) / ref):.2e}")
    assert len(chi) == 40 and np.max(np.abs(chi - ref) / ref) <= 1e-12
    counts = opt.classify_edges(E, 300.0)  # between the inliers' 9 .. 36 and the moved observations' > 1000
    assert counts == dict(over_chi2=4, depth_failed=0, bad=4)
    assert np.array_equal(opt.edge_levels(E), bad.astype(np.int32))
    opt.initialize_optimization(0)
    kept = B.without(prob, bad)
    assert abs(opt.chi2() - float(np.sum(ref[~bad]))) <= 1e-12 * float(np.sum(ref[~bad]))
    dev = _run(opt, 3, "lm_hip_fix9_3")
    d = B.Dense(kept)
    out = B.lm(d, 3)
    _same_as_reference(dev, ([c for c, _, _ in out], [t for _, t, _ in out], d.minimal_state()))
    # the set-aside edges are still evaluated, at the optimised state (the active ones are fitted by then: their chi2
    # falls under 0.1, where the float64 floor is no longer under 1e-13, tests/test_bal_host.py)
    after = B.Graph(prob).edge_chi2(_est_of(opt, prob))
    got = opt.edge_chi2(E)
    assert len(got) == 40 and np.max(np.abs(got[bad] - after[bad]) / after[bad]) <= 1e-12 and got[bad].min() > 300.0


# ---------------------------------------------------------------- 7: marginals
def test_marginals(g2o_amd_mod):
    prob = B.trajectory_case((0,))
    opt = _device(g2o_amd_mod, prob)
    opt.set_algorithm("lm_hip_fix9_3")
    opt.initialize_optimization()
    opt.build_structure()
    opt.build_system()
    pd, _, npose, _ = opt.block_dims()
    r = B.numpy_stage(prob, 0.0, est=_est_of(opt, prob))
    Hpp = r["H"][:r["np"], :r["np"]]
    assert pd == 9 and Hpp.shape == (npose * 9, npose * 9)
    Hinv = np.linalg.inv(Hpp)
    blocks = opt.compute_marginals([(0, 0), (3, 3), (1, 3)])
    assert blocks is not None and len(blocks) == 3
    num = den = 0.0
    for (rr, c), Bk in blocks.items():
        Rf = Hinv[rr * 9:(rr + 1) * 9, c * 9:(c + 1) * 9]
        num += float(np.sum((Bk - Rf) ** 2))
        den += float(np.sum(Rf ** 2))
    print(f"marginals {np.sqrt(num / den):.2e}")
    assert np.sqrt(num / den) <= 1e-9


# ---------------------------------------------------------------- 8: files
def test_bal_files(g2o_amd_mod, tmp_path):
    mod = g2o_amd_mod
    prob = B.trajectory_case(())
    (es,) = prob.edges
    nc, npt = 6, 40
    path = str(tmp_path / "problem.txt")
    with open(path, "w") as f:
        f.write(B.bal_text(prob, sep="\t\r\n "))  # whitespace of any kind between the tokens
    a = mod.SparseOptimizer(0)
    a.load_bal(path)
    assert a.num_vertices() == nc + npt and a.num_edges() == len(es.v0)
    assert np.array_equal(a.estimates(V), prob.vertices[0].est) and np.array_equal(a.estimates(P), prob.vertices[1].est)
    L = mod.lib()
    ids = np.zeros(npt, np.int32)
    assert L.g2ohip_get_estimates(a.h, P, None, mod._p(ids)) == npt and np.array_equal(ids, nc + np.arange(npt))
    ids = np.zeros(nc, np.int32)
    assert L.g2ohip_get_estimates(a.h, V, None, mod._p(ids)) == nc and np.array_equal(ids, np.arange(nc))
    fresh = _device(mod, prob)
    assert a.chi2() == fresh.chi2()
    a.set_algorithm("lm_hip_fix9_3")
    a.initialize_optimization()
    a.build_structure()
    assert a.block_dims() == [9, 3, nc, npt]
    free = mod.SparseOptimizer(0)
    free.load_bal(path, marginalize=False)  # points of dimension 3 beside cameras of 9
    with pytest.raises(mod.G2OHipError) as ei:
        free.initialize_optimization()
    assert f"({ERR_UNSUPPORTED})" in str(ei.value) and "one pose block size" in str(ei.value)
    # save -> load is bitwise, from the device's state
    a.optimize(1)
    out = str(tmp_path / "out.txt")
    a.save_bal(out)
    b = mod.SparseOptimizer(0)
    b.load_bal(out)
    assert np.array_equal(a.estimates(V), b.estimates(V)) and np.array_equal(a.estimates(P), b.estimates(P))
    assert a.chi2() == b.chi2()
    cams, pts, ci, pi, obs = B.parse_bal(open(out).read())
    assert np.array_equal(cams, a.estimates(V)) and np.array_equal(ci, es.v0) and np.array_equal(obs, es.meas)
    out2 = str(tmp_path / "out2.txt")
    b.save_bal(out2)
    assert open(out).read() == open(out2).read()
    # what the format cannot carry is refused and nothing is written
    for change in ("info", "ids"):
        p2 = B.trajectory_case(())
        if change == "info":
            p2.edges[0].info[3] = [[2.0, 0.0], [0.0, 1.0]]
        else:
            p2.vertices[1].ids[:] = p2.vertices[1].ids + 1
            p2.edges[0].v1[:] = p2.edges[0].v1 + 1
        c = _device(mod, p2)
        nowhere = str(tmp_path / f"none_{change}.txt")
        with pytest.raises(mod.G2OHipError) as ei:
            c.save_bal(nowhere)
        assert f"({ERR_UNSUPPORTED})" in str(ei.value) and not (tmp_path / f"none_{change}.txt").exists()


@pytest.mark.parametrize("what", ["truncated", "index", "token", "header", "nan"])
def test_bad_bal_files(g2o_amd_mod, tmp_path, what):
    """A short file, an index out of range, a non-numeric token, counts the file cannot hold (nothing is allocated from
    them) and a value that is no finite decimal number: ERR_ARG, the record named, the graph unchanged."""
    mod = g2o_amd_mod
    prob = B.scene(3, 5, 3, 9700)
    words = B.bal_text(prob).split()
    if what == "truncated":
        words, name = words[:-2], "point 4"
    elif what == "index":
        words[3 + 4 * 7], name = "3", "observation 7"  # cameras are 0 .. 2
    elif what == "header":
        words[2], name = "2000000000", "header"
    elif what == "nan":
        words[-4], name = "nan", "point 3"
    else:
        words[3 + 4 * 15 + 9 + 6], name = "4x1.5", "camera 1"
    path = str(tmp_path / f"{what}.txt")
    with open(path, "w") as f:
        f.write("\n".join(words) + "\n")
    base = B.one_edge(True)  # ids 3 and 7: a graph that is there already
    opt = _device(mod, base)
    with pytest.raises(mod.G2OHipError) as ei:
        opt.load_bal(path)
    msg = str(ei.value)
    assert f"({ERR_ARG})" in msg and name in msg and mod.last_error(), msg
    assert opt.num_vertices() == 2 and opt.num_edges() == 1
    assert np.array_equal(opt.estimates(V), base.vertices[0].est)


# ---------------------------------------------------------------- 9: refusals
def test_refusals(g2o_amd_mod):
    mod = g2o_amd_mod
    prob = B.scene(3, 8, 3, 9800)

    def refused(call, code, *words):
        with pytest.raises(mod.G2OHipError) as ei:
            call()
        msg = str(ei.value)
        assert f"({code})" in msg and mod.last_error() and all(w in msg for w in words), msg

    # the iterative solvers: pose blocks of 3 or 6 only
    for algo in ("lm_pcg", "lm_pcg6_3", "lm_pcg6_3_eigen"):
        opt = _device(mod, prob)
        opt.set_algorithm(algo)
        refused(opt.build_structure, ERR_UNSUPPORTED, "blocks of 9", "lm_hip_fix9_3")
        refused(lambda: opt.optimize(1), ERR_UNSUPPORTED, "blocks of 9")
    opt = _device(mod, prob)
    for name in ("lm_hip_fix9_3", "gn_hip_fix9_3", "dl_hip_fix9_3", "lm_hip_var"):
        opt.set_algorithm(name)
    # a sharded graph: refused at the structure build, before any collective
    key = uuid.uuid4().hex
    opts = [_device(mod, prob) for _ in range(2)]
    for r, o in enumerate(opts):
        o.set_algorithm("lm_hip_fix9_3")
        o.set_comm_local(key, r, 2)
    for o in opts:
        refused(o.build_structure, ERR_UNSUPPORTED, "2 ranks", "blocks of 9")
    # structure-only on a point that carries a BAL edge
    opt = _device(mod, prob)
    opt.set_algorithm("structure_only_3")
    refused(lambda: opt.structure_only(iterations=1), ERR_UNSUPPORTED, "structure-only", "edge type 30 on a marginalised vertex")
    # the .g2o format cannot carry the types
    opt = _device(mod, prob)
    refused(lambda: opt.save("/nonexistent-directory/never-written.g2o"), ERR_UNSUPPORTED, "EdgeObservationBAL", "g2ohip_save_bal")
    # arguments
    es = prob.edges[0]
    opt = mod.SparseOptimizer(0)
    for vs in prob.vertices:
        opt.add_vertices(vs)
    refused(lambda: opt.add_edges(synth.EdgeSet(E, es.v0, es.v1, es.meas, es.info, np.zeros((len(es.v0), 4)))), ERR_ARG,
            "edge type 30", "params must be NULL")
    opt.add_edges(es)
    opt.initialize_optimization()
    refused(lambda: opt.classify_edges(E, 10.0, check_depth=True), ERR_ARG, "isDepthPositive")
    refused(lambda: opt.edge_chi2(E, depth=True), ERR_ARG, "isDepthPositive")
    # a point in the camera's place and the reverse
    pts = prob.vertices[1]
    swapped = synth.Problem("swapped", prob.vertices, [B._es(E, es.v1[:2], es.v0[:2], es.meas[:2], es.info[:2])], 9, 3)
    opt = _device(mod, swapped)
    refused(opt.initialize_optimization, ERR_UNSUPPORTED, "edge type 30", f"vertex type {P}")
    two_cams = synth.Problem("cams", prob.vertices, [B._es(E, [0, 1], [1, 2], es.meas[:2], es.info[:2])], 9, 3)
    opt = _device(mod, two_cams)
    refused(opt.initialize_optimization, ERR_UNSUPPORTED, "edge type 30", f"vertex type {V}")
    # a free non-marginalised point beside the cameras
    loose = B.scene(3, 8, 3, 9800, marginalize=False)
    opt = _device(mod, loose)
    refused(opt.initialize_optimization, ERR_UNSUPPORTED, "one pose block size")
    # host-Jacobian edges stop at dimension 7
    hj = synth.EdgeSet(32 + 2, es.v0[:2], es.v1[:2], None, es.info[:2], None)
    opt = _device(mod, synth.Problem("hj", prob.vertices, [hj], 9, 3))
    refused(opt.initialize_optimization, ERR_UNSUPPORTED, "2, 3, 6 or 7")
