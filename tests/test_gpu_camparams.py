"""Device-side EdgeProjectXYZ2UV / EdgeProjectXYZ2UVU on a CameraParameters record (G2OHIP_E_PROJECT_XYZ2UV = 23,
_XYZ2UVU = 24): the error in all doubles (no float bf), the fused assembly (Kt records for the monocular type, G blocks
for the stereo one), the generic slot path (mixed graphs, G2OHIP_ASM_FUSED=0), landmark shards, structure-only, levels /
per-edge chi2 / classification, the refusals and the .g2o files.

References: tests/camparams_ref.py (plain numpy: errors, dense normal equations, dense Schur complement, the
reference's file formats), the same graph entered as G2OHIP_E_HOSTJ(D) edges whose host callback is camparams_ref's
payload (LM trajectories), and the twins in the fork's types (synth.camparams_twin).

Tolerances are the project's own, as listed in tests/test_gpu_stereo.py: stage level 1e-9 (b, bschur, x) and 1e-11
(Hschur); initial and per-edge chi2 1e-12; trajectories 1e-6 relative with identical trial counts; fused against generic
1e-10; multiplyHessian 1e-8; shards against one rank 1e-9 on the state and 1e-6 on chi2. The monocular twin runs the
same device arithmetic and is held to 1e-10; structure-only against the twins: points 1e-12 (mono) and 1e-9 (stereo,
f = 512, b = 0.125: bf = 64 is exact in float, the error forms differ in their rounding only).
"""
import threading
import uuid

import numpy as np
import pytest

import camparams_ref as R
from camparams_ref import KINDS, UV, UVU
from g2o_amd import synth
from shard_util import gather_sharded_state

pytestmark = pytest.mark.gpu

RTOL = 1e-6
HUBER = 2.447
ERR_ARG, ERR_UNSUPPORTED = -1, -4
ALL_RK = ["Huber", "PseudoHuber", "Cauchy", "GemanMcClure", "Welsch", "Fair", "Tukey", "Saturated", "DCS"]
NOISY = dict(cam_rot_noise=0.02, cam_trans_noise=0.05, point_noise=0.1, pixel_noise=200.0, disparity_noise=200.0,
             seed=11)  # test_gpu_stereo._noisy_problem's

_PROBS = {}  # problems and reference runs, computed once, shared, left unchanged


def _cached(key, make):
    if key not in _PROBS:
        _PROBS[key] = make()
    return _PROBS[key]


def _lm_problem(etype):
    return _cached(("lm", etype), lambda: synth.ba_camparams(40, 1500, obs_per_point=8, window=24, stereo=etype == UVU))


def _noisy_problem(etype):
    return _cached(("noisy", etype), lambda: synth.ba_camparams(40, 1500, obs_per_point=8, window=24,
                                                                stereo=etype == UVU, **NOISY))


def _exact_problem(etype):
    # f = 512, b = 0.125: bf = 64 is exact in float
    return _cached(("exact", etype), lambda: synth.ba_camparams(40, 1500, obs_per_point=8, window=24,
                                                                stereo=etype == UVU, focal=512.0, baseline=0.125))


# ---------------------------------------------------------------- the host-J reference run
def _hostj_problem(mod, prob):
    edges = [synth.EdgeSet(mod.E_HOSTJ(synth.ERR_DIM[e.etype]), e.v0, e.v1, None, e.info, None)
             if e.etype in KINDS else e for e in prob.edges]
    return synth.Problem(prob.name + "_hostj", prob.vertices, edges, prob.pose_dim, prob.landmark_dim)


def _hostj_optimizer(mod, prob, huber=False):
    g = R.Graph(prob)
    back = {mod.E_HOSTJ(synth.ERR_DIM[e.etype]): e.etype for e in prob.edges if e.etype in KINDS}
    hp = _hostj_problem(mod, prob)
    opt = mod.SparseOptimizer(0).add_problem(hp)
    opt.set_host_edge_callback(
        lambda etype, with_jac: g.payload(back[etype], opt.estimates(synth.V_SE3_EXPMAP), opt.estimates(synth.V_XYZ)))
    if huber:
        for e in hp.edges:
            opt.set_robust_kernel(e.etype, "Huber", HUBER)
    return opt


def _device_optimizer(mod, prob, huber=False):
    opt = mod.SparseOptimizer(0).add_problem(prob)
    if huber:
        for e in prob.edges:
            opt.set_robust_kernel(e.etype, "Huber", HUBER)
    return opt


def _run(opt, iters, algo=None):
    if algo:
        opt.set_algorithm(algo)
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
def test_single_edge_pin(g2o_amd_mod):
    """One fixed camera, one point, one XYZ2UVU edge, f = 1003, b = 0.1, |e| ~ 1e-3: a float-rounded f * b would move
    chi2 by 8.9e-4 relative (test_camparams_host.test_double_baseline_is_visible_in_the_single_edge_error)."""
    prob = R.single_edge_case()
    ref = R.Graph(prob).chi2()
    chi = g2o_amd_mod.SparseOptimizer(0).add_problem(prob).chi2()
    print(f"single XYZ2UVU edge: chi2 device {chi:.17g} numpy {ref:.17g} rel {abs(chi - ref) / ref:.2e}")
    assert abs(chi - ref) <= 1e-12 * ref


@pytest.mark.parametrize("etype", KINDS)
def test_initial_chi2(g2o_amd_mod, etype):
    prob = synth.ba_camparams(40, 1500, stereo=etype == UVU)
    ref = R.Graph(prob).chi2()
    chi = g2o_amd_mod.SparseOptimizer(0).add_problem(prob).chi2()
    print(f"ba_camparams(40, 1500) type {etype}: chi2 device {chi:.17g} numpy {ref:.17g} rel {abs(chi - ref) / ref:.2e}")
    assert abs(chi - ref) <= 1e-12 * ref


# ---------------------------------------------------------------- 3: robust kernels
@pytest.mark.parametrize("etype", KINDS)
def test_robust_kernels(g2o_amd_mod, etype):
    """Every kernel of the factory on each type: the robust chi2 of the device family equals that of the same errors
    entered as host-J records (the same robustify on both sides), and Huber's equals numpy's."""
    mod = g2o_amd_mod
    prob = _cached(("rk", etype), lambda: synth.ba_camparams(12, 150, obs_per_point=5, window=8, pixel_noise=3.0,
                                                             stereo=etype == UVU))
    g = R.Graph(prob)
    hj_t = mod.E_HOSTJ(synth.ERR_DIM[etype])
    dev = mod.SparseOptimizer(0).add_problem(prob)
    hj = mod.SparseOptimizer(0).add_problem(_hostj_problem(mod, prob))
    hj.set_host_jacobians(hj_t, g.payload(etype))
    plain = g.chi2()
    for kind in ALL_RK:
        dev.set_robust_kernel(etype, kind, 2.0)
        hj.set_robust_kernel(hj_t, kind, 2.0)
        a, b = dev.chi2(), hj.chi2()
        print(f"type {etype} {kind}: device {a:.17g} host-J {b:.17g}")
        assert abs(a - b) <= 1e-12 * b, (kind, a, b)
        assert a < plain, kind  # the kernel bites
        if kind == "Huber":
            assert abs(a - g.chi2(huber_delta=2.0)) <= 1e-12 * a


# ---------------------------------------------------------------- 4: stage against the dense numpy system
def _stage_problem(etype):
    """ba_camparams(12, 150, 5, 8) with every 7th point fixed, a CameraParameters record of its own per edge, a random
    non-diagonal SPD information per edge and 5 % gross outliers."""
    def make():
        base = synth.ba_camparams(12, 150, obs_per_point=5, window=8, stereo=etype == UVU)
        cams, pts = base.vertices
        fixed = pts.fixed.copy()
        fixed[::7] = 1
        pv = synth.VertexSet(pts.vtype, pts.ids, pts.est, fixed, pts.marginalized)
        e = base.edges[0]
        D = synth.ERR_DIM[etype]
        rng = np.random.default_rng(5)
        n = len(e.v0)
        par = e.params * (1.0 + 0.02 * rng.standard_normal(e.params.shape))
        A = rng.standard_normal((n, D, D)) * 0.4
        info = np.eye(D)[None] + np.einsum("nij,nkj->nik", A, A)
        meas = e.meas.copy()
        out = rng.random(n) < 0.05
        meas[out] += rng.standard_normal((int(out.sum()), D)) * 30.0
        ev = synth.EdgeSet(e.etype, e.v0, e.v1, meas, info, par)
        return synth.Problem(base.name + "_fixedpts", [cams, pv], [ev], 6, 3)
    return _cached(("stage", etype), make)


def _dense_ref(key, prob, lam, huber):
    def make():
        H, b, npose, nl = R.Graph(prob).dense_system(HUBER if huber else None)
        Hs, bs, x = R.schur_solve(H, b, npose, lam)
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
@pytest.mark.parametrize("etype", KINDS)
def test_stage_fixed_points_varied_records_robust(g2o_amd_mod, monkeypatch, etype, path):
    _stage_check(g2o_amd_mod, monkeypatch, ("fixedpts", etype), _stage_problem(etype), 1e-3, True, path)


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("etype", KINDS)
def test_stage_long_tracks(g2o_amd_mod, monkeypatch, etype, path):
    """Landmarks with more than 64 observations: chunk partials and k_lm_fixup."""
    prob = _cached(("long", etype), lambda: synth.ba_camparams(140, 300, obs_per_point=90, window=120, seed=7,
                                                               stereo=etype == UVU))
    _stage_check(g2o_amd_mod, monkeypatch, ("long", etype), prob, 1e-2, False, path)


# ---------------------------------------------------------------- 5: LM trajectories
@pytest.mark.parametrize("etype", KINDS)
def test_lm_trajectory_against_host_jacobians(g2o_amd_mod, etype):
    prob = _lm_problem(etype)
    _same_trajectory(_run(_device_optimizer(g2o_amd_mod, prob), 6), _hostj_run(g2o_amd_mod, ("lm", etype), prob, 6))


@pytest.mark.parametrize("etype", KINDS)
def test_lm_trajectory_with_rejected_trials(g2o_amd_mod, etype):
    prob = _noisy_problem(etype)
    ref = _hostj_run(g2o_amd_mod, ("noisy", etype), prob, 6)
    print(f"noisy type {etype}: reference trials per iteration {ref[2]}")
    assert any(t > 1 for t in ref[2]), f"the reference run rejected no trial: {ref[2]}"
    _same_trajectory(_run(_device_optimizer(g2o_amd_mod, prob), 6), ref)


# ---------------------------------------------------------------- 6: twins
def test_mono_equals_its_twin(g2o_amd_mod):
    prob = _lm_problem(UV)
    (n1, c1, t1, x1), (n0, c0, t0, x0) = (_run(_device_optimizer(g2o_amd_mod, p), 6)
                                          for p in (prob, synth.camparams_twin(prob)))
    assert n1 == n0 and t1 == t0, (t1, t0)
    assert np.allclose(c1, c0, rtol=1e-10, atol=0)
    assert np.linalg.norm(x1 - x0) <= 1e-10 * np.linalg.norm(x0)


def test_stereo_against_its_twin(g2o_amd_mod):
    prob = _exact_problem(UVU)
    tw = synth.camparams_twin(prob)
    assert np.all(tw.edges[0].params[:, 4] == 64.0)
    _same_trajectory(_run(_device_optimizer(g2o_amd_mod, prob), 6), _run(_device_optimizer(g2o_amd_mod, tw), 6))


# ---------------------------------------------------------------- 7: the fused path is taken
@pytest.mark.parametrize("etype", KINDS)
def test_fused_equals_generic(g2o_amd_mod, monkeypatch, etype):
    prob = _lm_problem(etype)
    runs, lin_bytes = [], []
    for flag in ("1", "0"):
        monkeypatch.setenv("G2OHIP_ASM_FUSED", flag)
        opt = _device_optimizer(g2o_amd_mod, prob)
        runs.append(_run(opt, 6))
        lin_bytes.append(opt.kernel_bytes("linearize"))
    # the graph really takes the fused assembly: its linearize pass writes no per-edge slots (36 doubles an edge)
    assert lin_bytes[1] - lin_bytes[0] >= prob.num_edges * 36 * 8.0 - prob.vertices[1].ids.size * 12 * 8.0, lin_bytes
    (n1, c1, t1, x1), (n0, c0, t0, x0) = runs
    assert n1 == n0 and t1 == t0
    assert np.allclose(c1, c0, rtol=1e-10, atol=0)
    assert np.linalg.norm(x1 - x0) <= 1e-10 * np.linalg.norm(x0)


def test_mono_takes_the_kt_record_split(g2o_amd_mod):
    opt = _device_optimizer(g2o_amd_mod, _lm_problem(UV))
    _run(opt, 2, "lm_hip_fix6_3")
    info = opt.factor_info()
    print(f"XYZ2UV under lm_hip_fix6_3: schur_tasks {info['schur_tasks']} schur_tasks_kx {info['schur_tasks_kx']}")
    assert info["schur_tasks_kx"] > 0, info
    # the stereo type has no Kt record (D = 3): G blocks
    opt = _device_optimizer(g2o_amd_mod, _lm_problem(UVU))
    _run(opt, 2, "lm_hip_fix6_3")
    info = opt.factor_info()
    assert info["schur_tasks_kx"] == 0 and info["schur_tasks"] > 0, info


# ---------------------------------------------------------------- 8: mixed graphs
def _beside_fork_mono():
    """ba(40, 1500, 8, 24) with every other observation as XYZ2UV and the rest as E_SE3_PROJECT_XYZ."""
    def make():
        base = synth.ba(40, 1500, obs_per_point=8, window=24)
        e = base.edges[0]
        sel = np.arange(len(e.v0)) % 2 == 0
        par = np.stack([e.params[sel, 0], e.params[sel, 2], e.params[sel, 3], np.full(int(sel.sum()), 0.1)], axis=1)
        a = synth.EdgeSet(UV, e.v0[sel], e.v1[sel], e.meas[sel], e.info[sel], par)
        b = synth.EdgeSet(e.etype, e.v0[~sel], e.v1[~sel], e.meas[~sel], e.info[~sel], e.params[~sel])
        return synth.Problem(base.name + "_uv+fork", base.vertices, [a, b], 6, 3)
    return _cached("beside", make)


@pytest.mark.parametrize("which", ["uvu+uv", "uv+fork"])
def test_mixed_graphs(g2o_amd_mod, which):
    """Two edge groups sharing (landmark, camera) structure: the generic slot path; Huber on both types. Reference:
    the CameraParameters edges as host-J records (the fork's monocular edges stay on the device)."""
    if which == "uvu+uv":
        prob = _cached("mixed", lambda: synth.ba_camparams(40, 1500, obs_per_point=8, window=24, stereo_fraction=0.6))
    else:
        prob = _beside_fork_mono()
    assert len(prob.edges) == 2
    dev = _run(_device_optimizer(g2o_amd_mod, prob, huber=True), 5)
    _same_trajectory(dev, _hostj_run(g2o_amd_mod, ("mixed", which), prob, 5, huber=True))


# ---------------------------------------------------------------- 9: landmark shards
@pytest.mark.parametrize("etype", KINDS)
def test_two_local_ranks(g2o_amd_mod, etype):
    prob = _lm_problem(etype)
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


# ---------------------------------------------------------------- 10: Hpp consumers after a split assembly
@pytest.mark.parametrize("etype", KINDS)
def test_multiply_hessian_after_optimize(g2o_amd_mod, etype):
    prob = _lm_problem(etype)
    opt = _device_optimizer(g2o_amd_mod, prob)
    opt.optimize(3)
    npose = opt.block_dims()[2] * 6
    v = np.random.default_rng(0).standard_normal(npose)
    y = opt.multiply_hessian(v)
    H, _, np_, _ = R.Graph(prob).dense_system(cam_est=opt.estimates(synth.V_SE3_EXPMAP),
                                              pt_est=opt.estimates(synth.V_XYZ))
    assert np_ == npose
    Hpp = H[:npose, :npose]
    assert np.linalg.norm(y - Hpp @ v) <= 1e-8 * np.linalg.norm(Hpp @ v)


# ---------------------------------------------------------------- 11: structure-only
@pytest.mark.parametrize("etype", KINDS)
def test_structure_only_against_twin(g2o_amd_mod, etype):
    """ba_demo's first step, structure_only(iterations=10), against the twin in the fork's types: the monocular twin
    runs the same arithmetic (points at 1e-12), the stereo twin (bf = 64, exact in float) differs in the rounding of
    its error (points at 1e-9). The five counts are equal."""
    prob = _cached(("so", etype), lambda: synth.ba_camparams(12, 150, obs_per_point=5, window=8, stereo=etype == UVU,
                                                             focal=512.0, baseline=0.125, point_noise=0.2))
    out = []
    for p in (prob, synth.camparams_twin(prob)):
        opt = g2o_amd_mod.SparseOptimizer(0).add_problem(p)
        cams_before = opt.estimates(synth.V_SE3_EXPMAP)
        c0 = opt.chi2()
        counts = opt.structure_only(iterations=10)
        assert np.array_equal(opt.estimates(synth.V_SE3_EXPMAP), cams_before)
        assert counts["accepted"] > 0 and opt.chi2() < c0
        out.append((counts, opt.estimates(synth.V_XYZ)))
    (ca, pa), (cb, pb) = out
    print(f"type {etype}: counts {ca} twin {cb}")
    assert ca == cb
    worst = np.max(np.linalg.norm(pa - pb, axis=1) / np.linalg.norm(pb, axis=1))
    print(f"type {etype}: worst point against the twin {worst:.2e}")
    assert worst <= (1e-12 if etype == UV else 1e-9)


@pytest.mark.parametrize("etype", KINDS)
def test_ba_demo_sequence(g2o_amd_mod, etype):
    """ba_demo's sequence: structure_only(10), then LM on the same handle; the end state's chi2 is numpy's."""
    prob = synth.ba_camparams(8, 120, obs_per_point=4, window=8, stereo=etype == UVU, point_noise=0.2)
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    c0 = opt.chi2()
    counts = opt.structure_only(iterations=10)
    c1 = opt.chi2()
    opt.set_algorithm("lm_hip_fix6_3")
    n, st = opt.optimize(3)
    assert counts["accepted"] > 0 and c1 < c0 and st[-1].chi2 < c1
    ref = R.Graph(prob).chi2(cam_est=opt.estimates(synth.V_SE3_EXPMAP), pt_est=opt.estimates(synth.V_XYZ))
    assert abs(opt.chi2() - ref) <= 1e-12 * ref


# ---------------------------------------------------------------- 12: levels, per-edge chi2, classification
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("ne", [1, 64, 65, 257])
@pytest.mark.parametrize("etype", KINDS)
def test_edge_chi2_and_classify(g2o_amd_mod, etype, ne, shared):
    prob = R.edge_case(etype, ne, shared)
    ref = R.Graph(prob).edge_chi2(etype)
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    opt.initialize_optimization()
    chi = opt.edge_chi2(etype)
    assert chi.shape == ref.shape and np.max(np.abs(chi - ref) / ref) <= 1e-12
    if ne > 1:
        srt = np.sort(ref)
        top = srt[len(srt) // 2:]  # a threshold in the upper half: some, not all, edges are outliers
        k = int(np.argmax(np.diff(top)))
        gap = (top[k + 1] - top[k]) / top[k]
        thr = 0.5 * (top[k] + top[k + 1])
        assert gap > 1e-9
    else:
        thr = 0.5 * ref[0]
    bad = ref > thr
    counts = opt.classify_edges(etype, thr)
    assert counts == dict(over_chi2=int(bad.sum()), depth_failed=0, bad=int(bad.sum())) and bad.sum() > 0
    assert np.array_equal(opt.edge_levels(etype), bad.astype(np.int32))
    # the reference types have no isDepthPositive
    with pytest.raises(g2o_amd_mod.G2OHipError) as ei:
        opt.classify_edges(etype, thr, check_depth=True)
    assert f"({ERR_ARG})" in str(ei.value)
    with pytest.raises(g2o_amd_mod.G2OHipError) as ei:
        opt.edge_chi2(etype, depth=True)
    assert f"({ERR_ARG})" in str(ei.value)


@pytest.mark.parametrize("etype", KINDS)
def test_levels_leave_the_outliers_out(g2o_amd_mod, etype):
    """Level 1 edges are out of the system at initialize_optimization(0): the run equals that of the graph without them."""
    prob = _stage_problem(etype)
    e = prob.edges[0]
    ref = R.Graph(prob).edge_chi2(etype)
    bad = ref > np.sort(ref)[int(0.9 * len(ref))]
    opt = _device_optimizer(g2o_amd_mod, prob)
    opt.set_edge_levels(etype, bad.astype(np.int32))
    opt.initialize_optimization(0)
    keep = ~bad
    sub = synth.Problem("kept", prob.vertices, [synth.EdgeSet(etype, e.v0[keep], e.v1[keep], e.meas[keep], e.info[keep],
                                                              e.params[keep])], 6, 3)
    a, b = _run(opt, 3), _run(_device_optimizer(g2o_amd_mod, sub), 3)
    _same_trajectory(a, b)
    assert a[1][0] < float(np.sum(ref))


# ---------------------------------------------------------------- 13: refusals
def _mono_still_works(mod):
    opt = mod.SparseOptimizer(0).add_problem(synth.ba_camparams(12, 150, obs_per_point=5, window=8))
    n, st = opt.optimize(1)
    assert n == 1 and np.isfinite(st[0].chi2)


@pytest.mark.parametrize("etype", KINDS)
def test_refusals(g2o_amd_mod, tmp_path, etype):
    mod = g2o_amd_mod
    prob = synth.ba_camparams(12, 150, obs_per_point=5, window=8, stereo=etype == UVU)
    e = prob.edges[0]
    # no CameraParameters
    opt = mod.SparseOptimizer(0)
    for vs in prob.vertices:
        opt.add_vertices(vs)
    with pytest.raises(mod.G2OHipError) as ei:
        opt.add_edges(synth.EdgeSet(e.etype, e.v0, e.v1, e.meas, e.info, None))
    assert f"({ERR_ARG})" in str(ei.value) and opt.num_edges() == 0
    _mono_still_works(mod)
    # the Python wrapper checks the record length (n * 4)
    with pytest.raises(mod.G2OHipError):
        opt.add_edges(synth.EdgeSet(e.etype, e.v0, e.v1, e.meas, e.info, np.zeros((len(e.v0), 5))))
    # swapped endpoints (camera, point instead of point, camera)
    opt = mod.SparseOptimizer(0)
    for vs in prob.vertices:
        opt.add_vertices(vs)
    opt.add_edges(synth.EdgeSet(e.etype, e.v1, e.v0, e.meas, e.info, e.params))
    with pytest.raises(mod.G2OHipError) as ei:
        opt.initialize_optimization()
    assert f"({ERR_UNSUPPORTED})" in str(ei.value) and f"edge type {etype}" in str(ei.value)
    _mono_still_works(mod)
    # the CGLS solver's kernels take the fork's monocular edge only
    opt = mod.SparseOptimizer(0).add_problem(prob)
    opt.set_algorithm("lm_pcg6_3_eigen")
    with pytest.raises(mod.G2OHipError) as ei:
        opt.optimize(1)
    assert f"({ERR_UNSUPPORTED})" in str(ei.value) and "CameraParameters" in mod.last_error()
    assert f"edge type {etype}" in mod.last_error() and "lm_pcg6_3" in mod.last_error()
    opt.set_algorithm("lm_hip_fix6_3")  # the graph is still usable
    n, st = opt.optimize(1)
    assert n == 1 and np.isfinite(st[0].chi2)
    _mono_still_works(mod)
    if etype == UVU:  # .g2o files cannot carry the type
        path = tmp_path / "uvu.g2o"
        with pytest.raises(mod.G2OHipError) as ei:
            opt.save(str(path))
        assert f"({ERR_UNSUPPORTED})" in str(ei.value) and "XYZ2UVU" in mod.last_error()
        assert not path.exists()
        _mono_still_works(mod)
        n, st = opt.optimize(1)  # and the graph itself is unharmed by the refused save
        assert n == 1


# ---------------------------------------------------------------- 14: .g2o files
def test_loader_reads_the_reference_format(g2o_amd_mod, tmp_path):
    """A file written by camparams_ref (two distinct records) loads with camparams=True to the same graph; without the
    flag both tags are skipped; the library's own file, read by camparams_ref, holds the same records and edges."""
    mod = g2o_amd_mod
    prob = R.two_record_problem()
    e = prob.edges[0]
    p1 = str(tmp_path / "ref.g2o")
    recs, pid = R.write_g2o(prob, p1)
    opt = mod.SparseOptimizer(0)
    opt.load(p1, camparams=True)
    assert opt.num_edges() == len(e.v0) and opt.num_vertices() == 46
    ref = R.Graph(prob).chi2()
    assert abs(opt.chi2() - ref) <= 1e-12 * ref
    assert np.array_equal(opt.estimates(synth.V_XYZ), prob.vertices[1].est)
    plain = mod.SparseOptimizer(0)
    plain.load(p1)  # without the flag the two tags are skipped
    assert plain.num_vertices() == 46 and plain.num_edges() == 0
    p2 = str(tmp_path / "dev.g2o")
    opt.save(p2)
    got_recs, got_edges = R.read_g2o(p2)
    assert got_recs == dict(enumerate(recs))  # one line per distinct record, the baseline included, first-seen ids
    assert [g[:3] for g in got_edges] == [(a, b, k) for a, b, k in zip(e.v0, e.v1, pid)]
    vals = np.array([g[3:] for g in got_edges])
    want = np.stack([e.meas[:, 0], e.meas[:, 1], e.info[:, 0, 0], e.info[:, 0, 1], e.info[:, 1, 1]], axis=1)
    assert np.array_equal(vals, want)
    text = open(p2).read()
    assert "EDGE_PROJECT_XYZ2UVU" not in text and text.count(R.TAG_PARAMS) == 2


def test_g2o_round_trip_on_the_device(g2o_amd_mod, tmp_path):
    """save -> load(camparams=True) -> optimize(3): the chi2 trajectory of the original handle."""
    prob = R.two_record_problem()
    src = _device_optimizer(g2o_amd_mod, prob)
    p1 = str(tmp_path / "a.g2o")
    src.save(p1)
    back = g2o_amd_mod.SparseOptimizer(0)
    back.load(p1, camparams=True)
    assert back.num_edges() == src.num_edges() and back.num_vertices() == src.num_vertices()
    (na, ca, ta, _), (nb, cb, tb, _) = _run(src, 3), _run(back, 3)
    print(f"round trip: chi2 {ca} against {cb}")
    assert na == nb and ta == tb
    for x, y in zip(ca, cb):
        assert abs(x - y) <= 1e-12 * abs(y), (x, y)


BASE = ("PARAMS_CAMERAPARAMETERS 0 1000 320 240 0.1\nVERTEX_SE3:EXPMAP 0 0 0 0 0 0 0 1\nVERTEX_XYZ 1 0.1 0.2 4\n")
MALFORMED = {
    "undefined id": (BASE + "EDGE_PROJECT_XYZ2UV:EXPMAP 1 0 7 330 250 1 0 1\n", ("parameter id 7", "PARAMS_CAMERAPARAMETERS")),
    "id of another kind": ("PARAMS_SE3OFFSET 3 0 0 0 0 0 0 1\n" + BASE + "EDGE_PROJECT_XYZ2UV:EXPMAP 1 0 3 330 250 1 0 1\n",
                           ("parameter id 3", "another kind")),
    "missing endpoint": (BASE + "EDGE_PROJECT_XYZ2UV:EXPMAP 5 0 0 330 250 1 0 1\n", ("EDGE_PROJECT_XYZ2UV:EXPMAP", "vertex 5")),
    "wrong-typed endpoint": (BASE + "EDGE_PROJECT_XYZ2UV:EXPMAP 0 1 0 330 250 1 0 1\n",
                             ("EDGE_PROJECT_XYZ2UV:EXPMAP", "vertex 0", "VERTEX_XYZ")),
    "short edge line": (BASE + "EDGE_PROJECT_XYZ2UV:EXPMAP 1 0 0 330 250 1 0\n", ("EDGE_PROJECT_XYZ2UV:EXPMAP",)),
    "short parameter line": ("PARAMS_CAMERAPARAMETERS 0 1000 320 240\nVERTEX_XYZ 1 0.1 0.2 4\n", ("PARAMS_CAMERAPARAMETERS",)),
}


@pytest.mark.parametrize("case", list(MALFORMED))
def test_malformed_files(g2o_amd_mod, tmp_path, case):
    mod = g2o_amd_mod
    text, words = MALFORMED[case]
    path = tmp_path / "bad.g2o"
    path.write_text(text)
    with pytest.raises(mod.G2OHipError) as ei:
        mod.SparseOptimizer(0).load(str(path), camparams=True, offset=True)
    for w in words:
        assert w in mod.last_error(), (w, mod.last_error())
    assert f"({ERR_ARG})" in str(ei.value)
    # the same file without the flag: both tags are skipped, nothing fails
    opt = mod.SparseOptimizer(0)
    opt.load(str(path), offset=True)
    assert opt.num_edges() == 0
    # and a well-formed file loads: one edge, numpy's chi2
    good = tmp_path / "good.g2o"
    good.write_text(BASE + "EDGE_PROJECT_XYZ2UV:EXPMAP 1 0 0 330 250 2 0.25 1.5\n")
    opt = mod.SparseOptimizer(0)
    opt.load(str(good), camparams=True)
    e = R.edge_error(UV, [[0, 0, 0, 0, 0, 0, 1.0]], [[0.1, 0.2, 4.0]], [[330.0, 250.0]], [[1000.0, 320.0, 240.0, 0.1]])[0]
    ref = e @ np.array([[2.0, 0.25], [0.25, 1.5]]) @ e
    assert opt.num_edges() == 1 and abs(opt.chi2() - ref) <= 1e-12 * ref
