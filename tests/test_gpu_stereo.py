"""Device-side EdgeStereoSE3ProjectXYZ (G2OHIP_E_STEREO_SE3_PROJECT_XYZ): the family (error with the float-rounded bf,
the reference's Jacobian forms), the fused assembly at D = 3 (landmark-major chunks, k_lm_fixup, the camera-major pass,
the Schur split with G blocks), the generic slot path (mixed mono + stereo graphs), landmark shards and the refusals.

References: tests/stereo_ref.py (plain numpy: dense normal equations, dense Schur complement) for the stage-level
checks, and the same graph entered as G2OHIP_E_HOSTJ(3) edges whose host callback is stereo_ref's payload for the LM
trajectories (the device then only assembles and solves what the host linearized).

Tolerances are the project's own: stage level 1e-9 (b, bschur, x) and 1e-11 (Hschur) as test_gpu_schur_split._stage;
initial chi2 1e-12 as test_gpu_generic.test_robust_kernel_lm; trajectories 1e-6 relative with identical trial counts
(test_gpu_generic.RTOL); fused against generic 1e-10 as test_split_equals_plain_passes; multiplyHessian 1e-8 as
test_split_hpp_consumers_after_optimize; shards against one rank 1e-9 on the state and 1e-6 on chi2 as
test_gpu_sharded.test_sharded_matches_single_and_oracle.
"""
import threading
import uuid

import numpy as np
import pytest

import stereo_ref
from g2o_amd import synth
from shard_util import gather_sharded_state

pytestmark = pytest.mark.gpu

RTOL = 1e-6
E_STEREO = synth.E_STEREO_SE3_PROJECT_XYZ
HUBER = 2.447

_PROBS = {}  # problems and reference runs, computed once, shared, left unchanged


def _cached(key, make):
    if key not in _PROBS:
        _PROBS[key] = make()
    return _PROBS[key]


def _lm_problem():
    return _cached("lm", lambda: synth.ba_stereo(40, 1500, obs_per_point=8, window=24))


def _noisy_problem():
    # test_split_trajectory_with_rejected_trials's noise (the right image as noisy as the left)
    return _cached("noisy", lambda: synth.ba_stereo(40, 1500, obs_per_point=8, window=24, cam_rot_noise=0.02,
                                                    cam_trans_noise=0.05, point_noise=0.1, pixel_noise=200.0,
                                                    disparity_noise=200.0, seed=11))


# ---------------------------------------------------------------- the host-J(3) reference run
def _hostj_problem(mod, prob):
    edges = [synth.EdgeSet(mod.E_HOSTJ(3), e.v0, e.v1, None, e.info, None) if e.etype == E_STEREO else e
             for e in prob.edges]
    return synth.Problem(prob.name + "_hostj", prob.vertices, edges, prob.pose_dim, prob.landmark_dim)


def _hostj_optimizer(mod, prob, huber=False):
    g = stereo_ref.StereoGraph(prob)
    opt = mod.SparseOptimizer(0).add_problem(_hostj_problem(mod, prob))

    def cb(etype, with_jac):
        assert etype == mod.E_HOSTJ(3)
        return g.payload(opt.estimates(synth.V_SE3_EXPMAP), opt.estimates(synth.V_XYZ))

    opt.set_host_edge_callback(cb)
    if huber:
        for e in _hostj_problem(mod, prob).edges:
            opt.set_robust_kernel(e.etype, "Huber", HUBER)
    return opt


def _device_optimizer(mod, prob, huber=False):
    opt = mod.SparseOptimizer(0).add_problem(prob)
    if huber:
        for e in prob.edges:
            opt.set_robust_kernel(e.etype, "Huber", HUBER)
    return opt


def _run(opt, iters):
    n, st = opt.optimize(iters)
    return n, [s.chi2 for s in st], [s.levenbergIterations for s in st], opt.minimal_state()


def _hostj_run(mod, key, prob, iters, huber=False):
    return _cached(("hostj", key, iters, huber), lambda: _run(_hostj_optimizer(mod, prob, huber), iters))


def _same_trajectory(a, b, tol=RTOL):
    (na, ca, ta, xa), (nb, cb, tb, xb) = a, b
    assert na == nb and ta == tb, (na, nb, ta, tb)
    for x, y in zip(ca, cb):
        assert abs(x - y) <= tol * abs(y), (x, y)
    assert np.linalg.norm(xa - xb) <= tol * np.linalg.norm(xb), np.linalg.norm(xa - xb) / np.linalg.norm(xb)


# ---------------------------------------------------------------- 1, 2: the error
def test_single_edge_pins_float_bf(g2o_amd_mod):
    """One fixed camera, one point, one edge, bf = 100.3, |e| ~ 1e-3: the double bf would move chi2 by 1e-3 relative
    (test_stereo_host.test_float_bf_is_visible_in_the_single_edge_error)."""
    prob = stereo_ref.single_edge_case()
    ref = stereo_ref.StereoGraph(prob).chi2()
    chi = g2o_amd_mod.SparseOptimizer(0).add_problem(prob).chi2()
    print(f"single stereo edge: chi2 device {chi:.17g} numpy {ref:.17g} rel {abs(chi - ref) / ref:.2e}")
    assert abs(chi - ref) <= 1e-12 * ref


def test_initial_chi2(g2o_amd_mod):
    prob = synth.ba_stereo(40, 1500)
    ref = stereo_ref.StereoGraph(prob).chi2()
    chi = g2o_amd_mod.SparseOptimizer(0).add_problem(prob).chi2()
    print(f"ba_stereo(40, 1500): chi2 device {chi:.17g} numpy {ref:.17g} rel {abs(chi - ref) / ref:.2e}")
    assert abs(chi - ref) <= 1e-12 * ref


@pytest.mark.parametrize("kind", ["Huber", "PseudoHuber", "Cauchy", "GemanMcClure", "Welsch", "Fair", "Tukey",
                                  "Saturated", "DCS"])
def test_robust_kernels_accepted(g2o_amd_mod, kind):
    """Every kernel of the factory on the stereo type: the robust chi2 of the device family equals that of the same
    errors entered as host-J(3) records (the same robustify on both sides), and Huber's equals numpy's."""
    prob = synth.ba_stereo(12, 150, obs_per_point=5, window=8, pixel_noise=3.0)
    dev = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    dev.set_robust_kernel(E_STEREO, kind, 2.0)
    g = stereo_ref.StereoGraph(prob)
    hj = g2o_amd_mod.SparseOptimizer(0).add_problem(_hostj_problem(g2o_amd_mod, prob))
    hj.set_host_jacobians(g2o_amd_mod.E_HOSTJ(3), g.payload())
    hj.set_robust_kernel(g2o_amd_mod.E_HOSTJ(3), kind, 2.0)
    a, b = dev.chi2(), hj.chi2()
    assert abs(a - b) <= 1e-12 * b, (a, b)
    assert a < g.chi2()  # the kernel bites
    if kind == "Huber":
        assert abs(a - g.chi2(huber_delta=2.0)) <= 1e-12 * a


# ---------------------------------------------------------------- 3, 4: stage against the dense numpy system
def _stage_problem():
    """ba_stereo(12, 150, 5, 8) with every 7th point fixed, per-edge intrinsics (bf included), a random non-diagonal
    SPD information per edge and 5 % gross outliers."""
    def make():
        base = synth.ba_stereo(12, 150, obs_per_point=5, window=8)
        cams, pts = base.vertices
        fixed = pts.fixed.copy()
        fixed[::7] = 1
        pv = synth.VertexSet(pts.vtype, pts.ids, pts.est, fixed, pts.marginalized)
        e = base.edges[0]
        rng = np.random.default_rng(5)
        n = len(e.v0)
        par = e.params * (1.0 + 0.02 * rng.standard_normal(e.params.shape))
        A = rng.standard_normal((n, 3, 3)) * 0.4
        info = np.eye(3)[None] + np.einsum("nij,nkj->nik", A, A)
        meas = e.meas.copy()
        out = rng.random(n) < 0.05
        meas[out] += rng.standard_normal((int(out.sum()), 3)) * 30.0
        ev = synth.EdgeSet(e.etype, e.v0, e.v1, meas, info, par)
        return synth.Problem(base.name + "_fixedpts", [cams, pv], [ev], 6, 3)
    return _cached("stage", make)


def _dense_ref(key, prob, lam, huber):
    def make():
        H, b, npose, nl = stereo_ref.StereoGraph(prob).dense_system(HUBER if huber else None)
        Hs, bs, x = stereo_ref.schur_solve(H, b, npose, lam)
        return dict(b=b, bschur=bs, x=x, Hschur=Hs, np=npose, nl=nl)
    return _cached(("dense", key, lam, huber), make)


PATHS = {"fused_split": {}, "plain_passes": {"G2OHIP_SCHUR_SPLIT": "0"}, "generic": {"G2OHIP_ASM_FUSED": "0"}}


def _stage_check(mod, monkeypatch, key, prob, lam, huber, path):
    monkeypatch.setenv("G2OHIP_STAGE_SPLIT", "1")
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)
    r = _dense_ref(key, prob, lam, huber)
    opt = _device_optimizer(mod, prob, huber)
    g = opt.stage(lam)
    assert g["ok"] == 1
    assert (g["np"], g["nl"]) == (r["np"], r["nl"])
    for k in ("b", "bschur", "x"):
        err = np.linalg.norm(g[k] - r[k]) / np.linalg.norm(r[k])
        print(f"{key} {path} {k}: {err:.2e}")
        assert err <= 1e-9, (k, err)
    err = np.linalg.norm(g["Hschur"] - r["Hschur"]) / np.linalg.norm(r["Hschur"])
    print(f"{key} {path} Hschur: {err:.2e}")
    assert err <= 1e-11, err


@pytest.mark.parametrize("path", list(PATHS))
def test_stage_fixed_points_varied_intrinsics_robust(g2o_amd_mod, monkeypatch, path):
    _stage_check(g2o_amd_mod, monkeypatch, "fixedpts", _stage_problem(), 1e-3, True, path)


@pytest.mark.parametrize("path", list(PATHS))
def test_stage_long_tracks(g2o_amd_mod, monkeypatch, path):
    """Landmarks with more than 64 observations: chunk partials and k_lm_fixup (U, c and G of a split landmark) at D = 3."""
    prob = _cached("long", lambda: synth.ba_stereo(140, 300, obs_per_point=90, window=120, seed=7))
    _stage_check(g2o_amd_mod, monkeypatch, "long", prob, 1e-2, False, path)


# ---------------------------------------------------------------- 5, 6: LM trajectories
def test_lm_trajectory_against_host_jacobians(g2o_amd_mod):
    prob = _lm_problem()
    _same_trajectory(_run(_device_optimizer(g2o_amd_mod, prob), 6), _hostj_run(g2o_amd_mod, "lm", prob, 6))


def test_lm_trajectory_with_rejected_trials(g2o_amd_mod):
    prob = _noisy_problem()
    dev = _run(_device_optimizer(g2o_amd_mod, prob), 6)
    print("noisy stereo LM: trials per iteration", dev[2])
    _same_trajectory(dev, _hostj_run(g2o_amd_mod, "noisy", prob, 6))
    assert any(t > 1 for t in dev[2]), f"no rejected trial: {dev[2]}"


@pytest.mark.parametrize("which", ["lm", "noisy"])
def test_fused_equals_generic(g2o_amd_mod, monkeypatch, which):
    prob = _lm_problem() if which == "lm" else _noisy_problem()
    runs, lin_bytes = [], []
    for flag in ("1", "0"):
        monkeypatch.setenv("G2OHIP_ASM_FUSED", flag)
        opt = _device_optimizer(g2o_amd_mod, prob)
        runs.append(_run(opt, 6))
        lin_bytes.append(opt.kernel_bytes("linearize"))
    # the stereo graph really takes the fused assembly: its linearize pass writes no per-edge slots (36 doubles an edge)
    assert lin_bytes[1] - lin_bytes[0] >= prob.num_edges * 36 * 8.0 - prob.vertices[1].ids.size * 12 * 8.0, lin_bytes
    (n1, c1, t1, x1), (n0, c0, t0, x0) = runs
    assert n1 == n0 and t1 == t0
    assert np.allclose(c1, c0, rtol=1e-10, atol=0)
    assert np.linalg.norm(x1 - x0) <= 1e-10 * np.linalg.norm(x0)


# ---------------------------------------------------------------- 7: mixed mono + stereo
def test_mixed_mono_stereo_graph(g2o_amd_mod):
    """stereo_fraction = 0.6: two edge groups sharing (landmark, camera) structure, the generic slot path; Huber on
    both types. Reference: mono on the device + the stereo edges as host-J(3)."""
    prob = _cached("mixed", lambda: synth.ba_stereo(40, 1500, obs_per_point=8, window=24, stereo_fraction=0.6))
    assert len(prob.edges) == 2
    dev = _run(_device_optimizer(g2o_amd_mod, prob, huber=True), 5)
    _same_trajectory(dev, _hostj_run(g2o_amd_mod, "mixed", prob, 5, huber=True))


# ---------------------------------------------------------------- 8: one fixed camera
def test_one_fixed_camera(g2o_amd_mod):
    """A stereo rig observes the scale: one fixed camera leaves a well-posed system (the monocular graph needs two)."""
    prob = _cached("fixed1", lambda: synth.ba_stereo(40, 1500, obs_per_point=8, window=24, fixed_cameras=1))
    opt = _device_optimizer(g2o_amd_mod, prob)
    n, st = opt.optimize(5)
    assert n == 5
    assert all(np.isfinite(s.chi2) for s in st) and st[-1].chi2 < st[0].chi2
    dev = (n, [s.chi2 for s in st], [s.levenbergIterations for s in st], opt.minimal_state())
    _same_trajectory(dev, _hostj_run(g2o_amd_mod, "fixed1", prob, 5))
    # the bound test_gpu_parity.test_factor_schedules holds the two-fixed-camera monocular C4 to, at its lambda
    opt.build_system()
    opt.set_lambda(1e-3)
    assert opt.solve()
    res = opt.linear_residual()
    print(f"one fixed camera: linear residual {res:.2e}")
    assert res <= 1e-10
    opt.restore_diagonal()


# ---------------------------------------------------------------- 9: Hpp consumers after a split assembly
def test_hpp_consumers_after_optimize(g2o_amd_mod):
    prob = _lm_problem()
    opt = _device_optimizer(g2o_amd_mod, prob)
    opt.optimize(3)
    npose = opt.block_dims()[2] * 6
    v = np.random.default_rng(0).standard_normal(npose)
    y = opt.multiply_hessian(v)
    H, _, np_, _ = stereo_ref.StereoGraph(prob).dense_system(
        cam_est=opt.estimates(synth.V_SE3_EXPMAP), pt_est=opt.estimates(synth.V_XYZ))
    assert np_ == npose
    Hpp = H[:npose, :npose]
    assert np.linalg.norm(y - Hpp @ v) <= 1e-8 * np.linalg.norm(Hpp @ v)


# ---------------------------------------------------------------- 10: landmark shards
def test_two_local_ranks(g2o_amd_mod):
    prob = _lm_problem()
    nranks, iters = 2, 5
    key = uuid.uuid4().hex
    opts = [_device_optimizer(g2o_amd_mod, prob) for _ in range(nranks)]
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
    single = _device_optimizer(g2o_amd_mod, prob)
    n1, st1 = single.optimize(iters)
    for r in range(nranks):
        n, st = res[r]
        assert n == n1
        for a, b in zip(st, st1):
            assert a.levenbergIterations == b.levenbergIterations
            assert abs(a.chi2 - b.chi2) <= RTOL * b.chi2
    x, states = gather_sharded_state(prob, opts)
    C = prob.vertices[0].ids.size
    for s in states[1:]:
        assert np.array_equal(s[:6 * C], states[0][:6 * C])
    xs = single.minimal_state()
    assert np.linalg.norm(x - xs) <= 1e-9 * np.linalg.norm(xs)


# ---------------------------------------------------------------- 11: clean refusals
def _mono_still_works(mod):
    opt = mod.SparseOptimizer(0).add_problem(synth.ba(12, 150, obs_per_point=5, window=8))
    n, st = opt.optimize(1)
    assert n == 1 and np.isfinite(st[0].chi2)


def test_refusals(g2o_amd_mod, tmp_path):
    mod = g2o_amd_mod
    prob = synth.ba_stereo(12, 150, obs_per_point=5, window=8)
    e = prob.edges[0]
    # no intrinsics
    opt = mod.SparseOptimizer(0)
    for vs in prob.vertices:
        opt.add_vertices(vs)
    with pytest.raises(mod.G2OHipError):
        opt.add_edges(synth.EdgeSet(e.etype, e.v0, e.v1, e.meas, e.info, None))
    assert opt.num_edges() == 0
    _mono_still_works(mod)
    # wrong vertex types (camera, point instead of point, camera)
    opt = mod.SparseOptimizer(0)
    for vs in prob.vertices:
        opt.add_vertices(vs)
    opt.add_edges(synth.EdgeSet(e.etype, e.v1, e.v0, e.meas, e.info, e.params))
    with pytest.raises(mod.G2OHipError):
        opt.initialize_optimization()
    _mono_still_works(mod)
    # the CGLS solver's kernels are monocular only
    opt = mod.SparseOptimizer(0).add_problem(prob)
    opt.set_algorithm("lm_pcg6_3_eigen")
    with pytest.raises(mod.G2OHipError):
        opt.optimize(1)
    _mono_still_works(mod)
    # .g2o files cannot carry the type
    opt = mod.SparseOptimizer(0).add_problem(prob)
    path = tmp_path / "stereo.g2o"
    with pytest.raises(mod.G2OHipError) as ei:
        opt.save(str(path))
    assert "Stereo" in str(ei.value) or "stereo" in str(ei.value)
    assert not path.exists()
    _mono_still_works(mod)
    # and the stereo graph itself is unharmed by the refused save
    n, st = opt.optimize(1)
    assert n == 1
