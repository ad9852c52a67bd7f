"""Device-resident Powell dogleg (dl_hip_*, Engine::dl_solve) on the GPU.

* trajectory parity against the reference loop (tests/dogleg_ref.py over the CPU oracle) on the inputs whose decisions
  tests/test_dogleg_host.py shows to be far from their thresholds: every step type, rejected trials, the Hpp-only gain
  on Schur graphs, the not-PD damping loop and its Fail;
* the device loop against the same dogleg driven from the host through the Solver entry points (buildSystem,
  multiplyHessian, solve, x, b, update, push / pop, chi2) on edge families the oracle does not know;
* a host-Jacobian graph, whose trial errors come through the callback;
* determinism, the sharded refusal, the algorithm names, and LM after dogleg on one handle.
Tolerances: chi2 and state 1e-6 relative against the oracle (the project's CHI2_RTOL / STATE_RTOL), 1e-9 between the
two loops over the same device linear algebra; step types and try counts equal.
"""
import math
import threading
import uuid

import numpy as np
import pytest

import dogleg_ref
import unary_ref
from dogleg_ref import STEP_DL, STEP_GN, STEP_SD
from g2o_amd import synth

pytestmark = pytest.mark.gpu

CHI2_RTOL = 1e-6
STATE_RTOL = 1e-6
LOOP_RTOL = 1e-9
RHO_MARGIN, NORM_MARGIN, CHI_DROP = 1e-3, 1e-6, 1e-6  # tests/test_dogleg_host.py
ERR_UNSUPPORTED = -4
_CACHE = {}  # problems, computed once, shared, left unchanged


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _device_run(opt, iterations):
    """SparseOptimizer::optimize's loop one g2ohip_optimize_step at a time, the dogleg state read after each:
    (return value, [(chi2, state dict, stats)])."""
    out, cj, r = [], 0, 0
    for i in range(iterations):
        r, st = opt.optimize_step(i)
        out.append((st.chi2, opt.dogleg_state(), st))
        cj += 1
        if r != 0:
            break
    return (0 if r == 2 else cj), out


def _close(a, b, tol):
    return abs(a - b) <= tol * abs(b)


# ---------------------------------------------------------------- trajectory parity against the reference loop
_PARITY = [(c.key, algo) for c in dogleg_ref.TABLE for algo in (["dl_hip_var", c.fixed_algo] if c.pd else ["dl_hip_var"])]


@pytest.mark.parametrize("key,algo", _PARITY)
def test_trajectory_against_reference(g2o_amd_mod, oracle, key, algo):
    case = dogleg_ref.CASES[key]
    n_ref, its, x_ref = dogleg_ref.reference(key, oracle)
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(case.make())
    opt.set_algorithm(algo)
    opt.set_dogleg_params(initial_delta=case.initial_delta)
    n, dev = _device_run(opt, case.iterations)
    for k, (chi, s, st) in enumerate(dev):
        print(f"{key} {algo} it {k}: chi2 {chi:.9g} state {s} | reference chi2 {its[k].chi2:.9g} tries {its[k].tries} "
              f"delta {its[k].delta:.9g} step {its[k].last_step} lambda {its[k].lam:g}")
    assert n == n_ref and len(dev) == len(its), (n, n_ref, len(dev), len(its))
    for k, ((chi, s, st), it) in enumerate(zip(dev, its)):
        assert _close(chi, it.chi2, CHI2_RTOL), (k, chi, it.chi2)
        assert s["tries"] == it.tries, (k, s, it.tries)
        if it.result != dogleg_ref.FAIL:
            assert s["step"] == it.last_step, (k, s, it.last_step)
        assert _close(s["delta"], it.delta, 1e-6), (k, s["delta"], it.delta)
        assert s["lam"] == it.lam and s["was_pd"] == it.was_pd, (k, s, it.lam, it.was_pd)
        # G2OBatchStatistics: the reference's dogleg never sets levenbergIterations; lambda only while not PD
        assert st.levenbergIterations == 0
        assert st.lambda_ == (0.0 if it.was_pd else it.lam), (k, st.lambda_)
    x = opt.minimal_state()
    assert np.linalg.norm(x - x_ref) <= STATE_RTOL * np.linalg.norm(x_ref), \
        np.linalg.norm(x - x_ref) / np.linalg.norm(x_ref)


def test_fail_returns_zero(g2o_amd_mod, oracle):
    """lambda passes maxLambda at iteration 0: g2ohip_optimize returns 0 as for Gauss-Newton's Fail, state untouched."""
    case = dogleg_ref.CASES["C1_indef-0.5"]
    prob = case.make()
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    opt.set_algorithm("dl_hip_var")
    x0 = opt.minimal_state()
    n, st = opt.optimize(4)
    assert n == 0
    s = opt.dogleg_state()
    assert s["lam"] == 1e3 and not s["was_pd"] and s["tries"] == 1
    assert np.array_equal(opt.minimal_state(), x0)


def test_algorithm_names(g2o_amd_mod):
    """(here and not in the host tests: g2ohip_set_algorithm takes a graph handle, which takes a device)"""
    opt = g2o_amd_mod.SparseOptimizer(0)
    for suffix in ("var", "fix6_3", "fix3_2", "fix3_3", "fix6_6"):
        opt.set_algorithm("dl_hip_" + suffix)
    for name in ("dl_pcg", "dl_pcg6_3", "dl_pcg3_2", "dl_pcg6_3_eigen", "dl_var", "dl_hip_", "dl_"):
        with pytest.raises(g2o_amd_mod.G2OHipError, match="unknown optimization algorithm"):
            opt.set_algorithm(name)


def test_default_parameters(g2o_amd_mod):
    """set_dogleg_params(0, 0, 0, 0) selects the defaults: the run of a handle that never called it, and of one that
    had other values before."""
    prob = _cached("S2", lambda: synth.by_name("S2", "small"))
    runs = []
    for mode in range(3):
        opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
        opt.set_algorithm("dl_hip_fix3_2")
        if mode == 2:
            opt.set_dogleg_params(3.0, 2, 1e-3, 4.0)
        if mode >= 1:
            opt.set_dogleg_params(0, 0, 0, 0)
        n, dev = _device_run(opt, 3)
        runs.append((n, [(c, s) for c, s, _ in dev], opt.minimal_state()))
    assert runs[0][1][0][1]["tries"] == 10  # the default delta 1e4: nine rejected GN trials first
    for r in runs[1:]:
        assert r[0] == runs[0][0] and r[1] == runs[0][1]
        assert np.array_equal(r[2], runs[0][2])


def test_max_trials_terminates(g2o_amd_mod):
    """maxTrialsAfterFailure below the rejections the first iteration needs: Terminate after that iteration, the state
    popped back, delta halved once per rejected trial."""
    prob = _cached("S2", lambda: synth.by_name("S2", "small"))
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    opt.set_algorithm("dl_hip_var")
    opt.set_dogleg_params(max_trials=4)
    x0, chi0 = opt.minimal_state(), opt.chi2()
    n, st = opt.optimize(5)
    s = opt.dogleg_state()
    assert n == 1 and s["tries"] == 4 and s["step"] == STEP_GN and s["delta"] == 1e4 / 16
    assert st[0].chi2 == chi0 and np.array_equal(opt.minimal_state(), x0)


# ---------------------------------------------------------------- the same dogleg driven from the host
def _host_dogleg(mod, opt, iterations, initial_delta, max_trials=100):
    """optimization_algorithm_dogleg.cpp:57-208 on the host over the Solver entry points of the device (every vector
    crosses to the host, every product is one g2ohip_solver_multiply_hessian). PD systems only.
    Returns [(chi2, tries, delta, [(step, rho)], rho margin, norm margin, chi2 before)]."""
    L, h = mod.lib(), opt.h
    opt.initialize_optimization()
    opt.build_structure()
    npose = opt.block_dims()[0] * opt.block_dims()[2]
    delta, out = float(initial_delta), []
    for _ in range(iterations):
        chi = opt.chi2()
        opt.build_system()
        opt.restore_diagonal()
        b = opt.b()
        aux = opt.multiply_hessian(b[:npose])
        alpha = float(b @ b) / float(aux @ b[:npose])
        hsd = alpha * b
        hsd_norm = float(np.linalg.norm(hsd))
        assert opt.solve()
        hgn = opt.x()
        hgn_norm = float(np.linalg.norm(hgn))
        trials, tries, good, new_chi, rho_m, norm_m = [], 0, False, chi, math.inf, math.inf
        while True:
            tries += 1
            norm_m = min(norm_m, abs(hgn_norm - delta) / delta)
            if hgn_norm < delta:
                hdl, step = hgn, STEP_GN
            else:
                norm_m = min(norm_m, abs(hsd_norm - delta) / delta)
                if hsd_norm > delta:
                    hdl, step = delta / hsd_norm * hsd, STEP_SD
                else:
                    bma = hgn - hsd
                    c, bma_sq, hsd_sq = float(hsd @ bma), float(bma @ bma), float(hsd @ hsd)
                    disc = math.sqrt(c * c + bma_sq * (delta * delta - hsd_sq))
                    beta = (-c + disc) / bma_sq if c <= 0.0 else (delta * delta - hsd_sq) / (c + disc)
                    hdl, step = hsd + beta * bma, STEP_DL
            aux = opt.multiply_hessian(hdl[:npose])
            gain = -1.0 * float(aux @ hdl[:npose]) + 2.0 * float(b @ hdl)
            assert L.g2ohip_push(h) == 0
            hdl = np.ascontiguousarray(hdl)
            assert L.g2ohip_update(h, hdl.ctypes.data) == 0
            t_chi = opt.chi2()
            if abs(gain) < 1e-12:
                gain = 1e-12
            rho = (chi - t_chi) / gain
            if rho > 0:
                assert L.g2ohip_discard_top(h) == 0
                good, new_chi = True, t_chi
            else:
                assert L.g2ohip_pop(h) == 0
            if rho > 0.75:
                delta = max(delta, 3.0 * float(np.linalg.norm(hdl)))
            elif rho < 0.25:
                delta *= 0.5
            trials.append((step, rho))
            rho_m = min(rho_m, abs(rho), abs(rho - 0.25), abs(rho - 0.75))
            if good or tries >= max_trials:
                break
        out.append((new_chi, tries, delta, trials, rho_m, norm_m, chi))
        if not good:
            break
    return out


def _robust_ba():  # 2 px of noise under Huber(2.447): a good part of the observations is past the kernel's delta
    return synth.ba(24, 600, obs_per_point=6, window=12, pixel_noise=2.0)


_LOOP_CASES = {
    # name: (problem, initial delta, iterations, robust kernel (edge type, kind, delta) or None)
    "ba_stereo": (lambda: synth.ba_stereo(24, 600, obs_per_point=6, window=12), 0.05, 4, None),
    "slam3d_landmarks": (lambda: synth.slam3d_landmarks(20, 200), 0.2, 4, None),
    "expmap_pose_graph": (lambda: synth.expmap_pose_graph(60, 12), 0.2, 4, None),
    "ba_huber": (_robust_ba, 0.05, 4, (synth.E_SE3_PROJECT_XYZ, "Huber", 2.447)),
}


@pytest.mark.parametrize("name", list(_LOOP_CASES))
def test_device_loop_against_host_loop(g2o_amd_mod, name):
    make, delta0, iters, robust = _LOOP_CASES[name]
    prob = _cached(name, make)

    def new():
        o = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
        if robust:
            o.set_robust_kernel(*robust)
        return o

    host = new()
    ref = _host_dogleg(g2o_amd_mod, host, iters, delta0)
    for k, (chi, tries, delta, trials, rho_m, norm_m, chi0) in enumerate(ref):
        print(f"{name} host loop it {k}: chi2 {chi0:.9g} -> {chi:.9g} tries {tries} delta {delta:.6g} "
              f"trials {[(s, float(f'{r:.4g}')) for s, r in trials]} rho margin {rho_m:.3g} norm margin {norm_m:.3g}")
        assert rho_m >= RHO_MARGIN and norm_m >= NORM_MARGIN, (k, rho_m, norm_m)
        assert chi0 - chi > CHI_DROP * chi0, (k, chi0, chi)
    assert len(ref) == iters
    assert any(s != STEP_GN for r in ref for s, _ in r[3]), "the initial delta must give a non-GN step"
    dev = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    if robust:
        dev.set_robust_kernel(*robust)
    dev.set_algorithm("dl_hip_var")
    dev.set_dogleg_params(initial_delta=delta0)
    n, run = _device_run(dev, iters)
    assert n == iters
    for k, ((chi, s, st), r) in enumerate(zip(run, ref)):
        print(f"{name} device it {k}: chi2 {chi:.12g} {s}")
        assert s["tries"] == r[1] and s["step"] == r[3][-1][0], (k, s, r[1], r[3])
        assert _close(chi, r[0], LOOP_RTOL), (k, chi, r[0])
        assert _close(s["delta"], r[2], LOOP_RTOL), (k, s["delta"], r[2])
    xh, xd = host.minimal_state(), dev.minimal_state()
    assert np.linalg.norm(xd - xh) <= LOOP_RTOL * np.linalg.norm(xh), np.linalg.norm(xd - xh) / np.linalg.norm(xh)


# ---------------------------------------------------------------- host-Jacobian edges: errors through the callback
def test_host_jacobian_callback(g2o_amd_mod, oracle):
    """SE2 priors entered as host-Jacobian unary edges (the priors alone hold the gauge): every trial's
    computeActiveErrors asks the callback for their errors. Reference: the oracle's binary twin (synth.twin_of)."""
    prob = _cached("hostj", lambda: synth.with_priors(synth.se2_grid(300), synth.E_SE2_PRIOR, every=10,
                                                      sigma=[0.2, 0.2, 0.1], seed=61, drop_fixed=True))
    iters, delta0 = 4, 1.0
    og = oracle.OracleGraph(synth.twin_of(prob))
    n_ref, its = dogleg_ref.optimize(og, iters, initial_delta=delta0)
    x_ref = og.minimal_state()[:-3]  # without the twin's identity vertex
    for k, it in enumerate(its):
        print(f"hostj reference it {k}: chi2 {it.chi2:.9g} tries {it.tries} delta {it.delta:.6g} trials {it.trials}")
        assert it.rho_margin >= RHO_MARGIN and it.norm_margin >= NORM_MARGIN, (k, it.rho_margin, it.norm_margin)
        assert it.chi2_before - it.chi2 > CHI_DROP * it.chi2_before
    g = unary_ref.Graph(prob)
    ht = g2o_amd_mod.E_HOSTJ_UNARY(3)
    edges = [synth.EdgeSet(ht, e.v0, None, None, e.info, None) if e.v1 is None else e for e in prob.edges]
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(synth.Problem("hostj", prob.vertices, edges, prob.pose_dim,
                                                                   prob.landmark_dim))
    calls = {True: 0, False: 0}

    def cb(etype, with_jac):
        calls[bool(with_jac)] += 1
        return g.prior_payload(synth.E_SE2_PRIOR, {v.vtype: opt.estimates(v.vtype) for v in prob.vertices})

    opt.set_host_edge_callback(cb)
    opt.set_algorithm("dl_hip_var")
    opt.set_dogleg_params(initial_delta=delta0)
    n, run = _device_run(opt, iters)
    assert n == n_ref == iters
    for k, ((chi, s, st), it) in enumerate(zip(run, its)):
        assert _close(chi, it.chi2, CHI2_RTOL), (k, chi, it.chi2)
        assert s["tries"] == it.tries and s["step"] == it.last_step, (k, s, it.tries, it.last_step)
        assert _close(s["delta"], it.delta, 1e-6)
    x = opt.minimal_state()
    assert np.linalg.norm(x - x_ref) <= STATE_RTOL * np.linalg.norm(x_ref)
    # one error refresh per trial at least, one linearization per iteration
    assert calls[False] >= sum(it.tries for it in its) and calls[True] >= iters, calls


# ---------------------------------------------------------------- online mode
def test_online_growth_resets_trust_region(g2o_amd_mod, oracle):
    """updateInitialization, then optimize again: iteration 0 starts over from initialDelta (the first part ends with
    delta 60.8, the continuation's first iteration leaves 3 * 3), as the reference's solve() does with a fresh
    algorithm. Reference: the same growth on the oracle under dogleg_ref."""
    from test_online import grow_split
    before, add_v, add_e, _ = _cached("online", lambda: grow_split(synth.se2_grid(300)))
    delta0 = 3.0
    g = oracle.OracleGraph(before)
    n1, its1 = dogleg_ref.optimize(g, 3, initial_delta=delta0)
    for v in add_v:
        g.add_vertices(v)
    for e in add_e:
        g.add_edges(e)
    assert g.update_initialization() == 0
    n2, its2 = dogleg_ref.optimize(g, 3, initial_delta=delta0)
    for k, it in enumerate(its1 + its2):
        assert it.rho_margin >= RHO_MARGIN and it.norm_margin >= NORM_MARGIN, (k, it.rho_margin, it.norm_margin)
        assert it.chi2_before - it.chi2 > CHI_DROP * it.chi2_before
    assert its1[-1].delta > 50 and its2[0].delta == pytest.approx(9.0)
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(before)
    opt.set_algorithm("dl_hip_fix3_3")
    opt.set_dogleg_params(initial_delta=delta0)
    m1, run1 = _device_run(opt, 3)
    for v in add_v:
        opt.add_vertices(v)
    for e in add_e:
        opt.add_edges(e)
    opt.update_initialization()
    m2, run2 = _device_run(opt, 3)
    assert (m1, m2) == (n1, n2) == (3, 3)
    for k, ((chi, s, st), it) in enumerate(zip(run1 + run2, its1 + its2)):
        assert _close(chi, it.chi2, CHI2_RTOL), (k, chi, it.chi2)
        assert s["tries"] == it.tries and s["step"] == it.last_step, (k, s, it.tries, it.last_step)
        assert _close(s["delta"], it.delta, 1e-6), (k, s["delta"], it.delta)
    x, xr = opt.minimal_state(), g.minimal_state()
    assert np.linalg.norm(x - xr) <= STATE_RTOL * np.linalg.norm(xr)


# ---------------------------------------------------------------- determinism, refusals, LM afterwards
def test_bitwise_reproducible(g2o_amd_mod):
    prob = _cached("S2", lambda: synth.by_name("S2", "small"))
    runs = []
    for _ in range(2):
        opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
        opt.set_algorithm("dl_hip_fix3_2")
        n, dev = _device_run(opt, 5)
        runs.append(([(c, s) for c, s, _ in dev], opt.minimal_state()))
    assert runs[0][0] == runs[1][0]
    assert np.array_equal(runs[0][1], runs[1][1])


def test_sharded_graph_refused(g2o_amd_mod):
    """Two landmark shards in one process: the structure build refuses dl_* before any collective."""
    prob = _cached("C4", lambda: synth.by_name("C4", "small"))
    L = g2o_amd_mod.lib()
    key = uuid.uuid4().hex
    opts = [g2o_amd_mod.SparseOptimizer(0).add_problem(prob) for _ in range(2)]
    for r, o in enumerate(opts):
        o.set_algorithm("dl_hip_fix6_3")
        o.set_comm_local(key, r, 2)
    res = [None, None]

    def body(r):  # one host thread per rank: g2ohip_last_error is per thread
        code = L.g2ohip_optimize(opts[r].h, None, 2, None)
        res[r] = (code, g2o_amd_mod.last_error())

    th = [threading.Thread(target=body, args=(r,)) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(120)
    for code, msg in res:
        assert code == ERR_UNSUPPORTED, res
        assert "dogleg" in msg and "shard" in msg, msg


def test_lm_after_dogleg_untouched(g2o_amd_mod):
    """A dl_* run leaves nothing behind that an lm_* run on the same handle reads: back at the initial estimates it
    gives the trajectory of a fresh graph, bit for bit."""
    prob = _cached("C4", lambda: synth.by_name("C4", "small"))

    def lm(opt):
        opt.set_algorithm("lm_hip_fix6_3")
        n, st = opt.optimize(4)
        return n, [(s.chi2, s.lambda_, s.levenbergIterations) for s in st], opt.minimal_state()

    fresh = lm(g2o_amd_mod.SparseOptimizer(0).add_problem(prob))
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    opt.set_algorithm("dl_hip_fix6_3")
    opt.set_dogleg_params(initial_delta=0.05)
    n, _ = opt.optimize(3)
    assert n == 3
    for vs in prob.vertices:
        opt.set_estimates(vs.vtype, vs.est)
    again = lm(opt)
    assert again[0] == fresh[0] and again[1] == fresh[1]
    assert np.array_equal(again[2], fresh[2])
