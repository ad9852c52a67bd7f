"""Edge levels, per-edge chi2, the depth test and outlier classification on the device (g2ohip_set_edge_levels,
g2ohip_initialize_level, g2ohip_edge_chi2, g2ohip_classify_edges; classify.hip).

References: a level-filtered handle against its "twin", a handle that holds only the edges of the level (bitwise: both
upload the same group arrays and every kernel sums in a fixed order); per-edge chi2 and camera-frame depth against the
numpy restatements of edge_levels_ref.Graph (unary_ref, slam3d_ref, expmap_ref, stereo_ref); the classification
against the callers' rule on numpy's values, with the threshold in a gap of them.

Tolerances are the project's own (tests/test_gpu_expmap.py): per-edge chi2 pins 1e-12 relative, trajectories 1e-6
relative, shards against one rank 1e-9. The pinned inputs carry noise or a perturbation, so that no edge's error is a
small difference of large numbers; EdgeSE3Expmap's cases stay outside the acos band (expmap_ref.assert_outside_band).
"""
import threading
import uuid

import numpy as np
import pytest

import edge_levels_ref as R
import expmap_ref
import pose_edges_ref
import slam3d_ref
import structure_only_ref
from g2o_amd import synth
from shard_util import gather_sharded_state

pytestmark = pytest.mark.gpu

E_BA, E_SBA, E_MONO, E_STEREO = R.E_BA, R.E_STEREO_BA, R.E_MONO, R.E_STEREO
ERR_ARG, ERR_STATE, ERR_UNSUPPORTED = -1, -2, -4
_CACHE = {}  # problems and numpy references, computed once, shared, left unchanged


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _ba():
    return _cached("ba", lambda: synth.ba(num_cameras=6, num_points=40, obs_per_point=4))


def _opt(mod, prob, alg=None, levels=None, level=None):
    opt = mod.SparseOptimizer(0).add_problem(prob)
    if alg:
        opt.set_algorithm(alg)
    if levels:
        R.apply_levels(opt, levels)
    if level is not None:
        opt.initialize_optimization(level)
    return opt


def _run(opt, iters=5, lam=1e-3):
    n, st = opt.optimize(iters)
    s = opt.stage(lam)
    return dict(n=n, chi=[x.chi2 for x in st], trials=[x.levenbergIterations for x in st], state=opt.minimal_state(),
                stage={k: s[k] for k in ("b", "x", "Hschur", "bschur")}, dims=opt.block_dims())


def _identical(a, b, tag):
    assert a["n"] == b["n"] and a["trials"] == b["trials"], (tag, a["n"], b["n"], a["trials"], b["trials"])
    assert a["dims"] == b["dims"], (tag, a["dims"], b["dims"])
    assert np.array_equal(np.array(a["chi"]), np.array(b["chi"])), (tag, a["chi"], b["chi"])
    assert np.array_equal(a["state"], b["state"]), (tag, np.abs(a["state"] - b["state"]).max())
    for k in a["stage"]:
        assert np.array_equal(a["stage"][k], b["stage"][k]), (tag, k)


# ---------------------------------------------------------------- 1: a level filter equals the twin graph
def _twin_cases():
    ba = _ba()
    return {
        "ba": (ba, "lm_hip_fix6_3", R.ba_levels(ba, 11)[0]),
        "ba_priors": (synth.with_priors(ba, synth.E_XYZ_PRIOR, every=3), "lm_hip_fix6_3", None),
        "slam3d": (synth.slam3d_landmarks(num_poses=6, num_points=30), "lm_hip_fix6_3", None),
        "expmap": (synth.expmap_pose_graph(num_poses=12, loops=4), "dl_hip_var", None),
        "pose_only": (synth.pose_only(num_cameras=3, points_per_camera=20), "gn_hip_var", None),
        "slam2d": (R.slam2d_problem(), "lm_hip_var", None),
    }


@pytest.mark.parametrize("name", ["ba", "ba_priors", "slam3d", "expmap", "pose_only", "slam2d"])
def test_level_filter_equals_twin(g2o_amd_mod, name):
    """Handle A: the whole graph, a pseudo-random third of every type's edges at level 1, initialize_level(0). Handle B:
    only the level-0 edges, g2ohip_initialize. chi2 per iteration, trial counts, the state and stage() are identical;
    initialize_level(1) equals the complement twin, initialize_level(-1) an untouched copy."""
    prob, alg, levels = _cached("twin", _twin_cases)[name]
    if levels is None:
        levels = R.ba_levels(prob, 12)[0] if name == "ba_priors" else R.third_levels(prob, 13)
    for level, keep in ((0, {t: lv == 0 for t, lv in levels.items()}), (1, {t: lv == 1 for t, lv in levels.items()}),
                        (-1, {})):
        a = _run(_opt(g2o_amd_mod, prob, alg, levels, level))
        twin = _opt(g2o_amd_mod, R.subproblem(prob, keep), alg)
        twin.initialize_optimization()
        b = _run(twin)
        assert a["n"] >= 1, (name, level, a["n"])  # a run that failed (0) would compare nothing
        print(f"{name} level {level}: dims {a['dims']} chi2 {a['chi'][0]:.6g} -> {a['chi'][-1]:.6g}")
        _identical(a, b, (name, level))
    if name in ("ba", "ba_priors"):  # a landmark with every observation set aside leaves the system
        whole = _opt(g2o_amd_mod, prob, alg, None, 0)
        whole.build_structure()
        filt = _opt(g2o_amd_mod, prob, alg, levels, 0)
        filt.build_structure()
        assert filt.block_dims()[3] == whole.block_dims()[3] - 1, (filt.block_dims(), whole.block_dims())


def test_default_levels_are_todays_initialize(g2o_amd_mod):
    """Every level 0: initialize_optimization(0), g2ohip_initialize and a graph that was given explicit zeros agree."""
    prob = _ba()
    a = _run(_opt(g2o_amd_mod, prob, "lm_hip_fix6_3"))
    b = _run(_opt(g2o_amd_mod, prob, "lm_hip_fix6_3", {E_BA: np.zeros(prob.num_edges, np.int32)}, 0))
    _identical(a, b, "zeros")
    assert np.array_equal(_opt(g2o_amd_mod, prob).edge_levels(E_BA), np.zeros(prob.num_edges, np.int32))


# ---------------------------------------------------------------- 2: a changed level waits for the next initialization
def test_levels_wait_for_initialization(g2o_amd_mod):
    prob = _ba()
    l0 = R.ba_levels(prob, 11)[0]
    l1 = {E_BA: l0[E_BA].copy()}
    l1[E_BA][::5] = 1
    a = _opt(g2o_amd_mod, prob, "lm_hip_fix6_3", l0, 0)
    ref = _opt(g2o_amd_mod, prob, "lm_hip_fix6_3", l0, 0)
    R.apply_levels(a, l1)
    assert np.array_equal(a.edge_levels(E_BA), l1[E_BA])
    assert a.chi2() == ref.chi2()
    ra, sa = a.optimize_step(0)
    rr, sr = ref.optimize_step(0)
    assert (ra, sa.chi2, sa.levenbergIterations) == (rr, sr.chi2, sr.levenbergIterations)
    assert np.array_equal(a.minimal_state(), ref.minimal_state())
    # back at the start and initialised again: the twin of the new levels
    for vs in prob.vertices:
        a.set_estimates(vs.vtype, vs.est)
    a.initialize_optimization(0)
    twin = _opt(g2o_amd_mod, R.subproblem(prob, {E_BA: l1[E_BA] == 0}), "lm_hip_fix6_3")
    twin.initialize_optimization()
    assert a.chi2() == twin.chi2()
    ra, sa = a.optimize_step(0)
    rt, stw = twin.optimize_step(0)
    assert (ra, sa.chi2, sa.levenbergIterations) == (rt, stw.chi2, stw.levenbergIterations)
    assert np.array_equal(a.minimal_state(), twin.minimal_state())


# ---------------------------------------------------------------- 3: per-edge chi2 pins
def _fix(prob, vtype, rows):
    verts = []
    for vs in prob.vertices:
        fx = vs.fixed.copy()
        if vs.vtype == vtype:
            fx[rows] = 1
        verts.append(synth.VertexSet(vs.vtype, vs.ids, vs.est, fx, vs.marginalized))
    return synth.Problem(prob.name + "_fix", verts, prob.edges, prob.pose_dim, prob.landmark_dim)


def _pin_cases():
    ba = _ba()
    s2 = R.slam2d_problem()
    sph = synth.sphere(nodes_per_level=6, laps=2)
    cam = [260.0, 250.0, 160.0, 120.0]
    return {
        "ba_mono": (ba, [E_BA]),
        "ba_stereo": (synth.ba_stereo(num_cameras=6, num_points=40, obs_per_point=4), [E_SBA]),
        "se3": (pose_edges_ref.se3_chain(20)[0], [synth.E_SE3_QUAT]),
        "se2": (pose_edges_ref.se2_chain(20)[0], [synth.E_SE2]),
        # vertices 0 and 1 fixed: the first edge joins two fixed vertices
        "se2_fixed_pair": (_fix(pose_edges_ref.se2_chain(9)[0], synth.V_SE2, [0, 1]), [synth.E_SE2]),
        "se2xy": (pose_edges_ref.se2xy_fan(20), [synth.E_SE2_XY]),
        "slam3d": (synth.slam3d_landmarks(6, 30, kind=slam3d_ref.KINDS, offset=slam3d_ref.OFFSET, camera=cam, seed=76),
                   list(slam3d_ref.KINDS)),
        "expmap": (expmap_ref.expmap_case(12, 4, seed=5), [synth.E_SE3_EXPMAP]),
        "pose_only": (synth.pose_only(num_cameras=3, points_per_camera=20), [E_MONO]),
        "pose_only_stereo": (synth.pose_only(num_cameras=3, points_per_camera=20, stereo=True), [E_STEREO]),
        "prior_se2": (synth.with_priors(s2, synth.E_SE2_PRIOR, every=3), [synth.E_SE2_PRIOR]),  # vertex 0 is fixed
        "prior_se2xy": (synth.with_priors(s2, synth.E_SE2_XY_PRIOR, every=3), [synth.E_SE2_XY_PRIOR]),
        "prior_xy": (synth.with_priors(s2, synth.E_XY_PRIOR, every=5), [synth.E_XY_PRIOR]),
        "prior_se3": (synth.with_priors(sph, synth.E_SE3_PRIOR, every=3, sigma=[0.05] * 3 + [0.01] * 3,
                                        offset=slam3d_ref.OFFSET), [synth.E_SE3_PRIOR]),
        "prior_xyz": (synth.with_priors(ba, synth.E_XYZ_PRIOR, every=3), [synth.E_XYZ_PRIOR, E_BA]),
    }


def _pin(opt, prob, etype, tag):
    want = _cached(("chi2", tag, etype), lambda: R.edge_chi2(prob, etype))
    got = opt.edge_chi2(etype)
    rel = np.abs(got - want) / want
    print(f"{tag} type {etype}: {len(want)} edges, chi2 {want.min():.3g} .. {want.max():.3g}, max rel {rel.max():.2e}")
    assert got.shape == want.shape and np.all(want > 0)
    assert np.all(rel <= 1e-12), (tag, etype, int(np.argmax(rel)), rel.max())
    return got


@pytest.mark.parametrize("name", ["ba_mono", "ba_stereo", "se3", "se2", "se2_fixed_pair", "se2xy", "slam3d", "expmap",
                                  "pose_only", "pose_only_stereo", "prior_se2", "prior_se2xy", "prior_xy", "prior_se3",
                                  "prior_xyz"])
def test_edge_chi2_pins(g2o_amd_mod, name):
    """Every device family per edge against numpy; a third of the edges on level 1 (inactive), the priors on fixed
    vertices and the edge between two fixed vertices get their chi2 like any other."""
    prob, etypes = _cached("pins", _pin_cases)[name]
    if name == "expmap":
        expmap_ref.assert_outside_band(expmap_ref.Graph(prob).residual_angles())
    if name == "prior_se2":
        es = R.edge_set(prob, synth.E_SE2_PRIOR)
        assert prob.vertices[0].fixed[np.searchsorted(prob.vertices[0].ids, es.v0)].any()  # a prior on a fixed vertex
    opt = _opt(g2o_amd_mod, prob, None, R.third_levels(prob, 21), 0)
    for etype in etypes:
        _pin(opt, prob, etype, name)


@pytest.mark.parametrize("n", [1, 64, 65, 257])
@pytest.mark.parametrize("stereo", [False, True])
def test_edge_chi2_sizes(g2o_amd_mod, n, stereo):
    """n edges of one camera: one wave, the wave boundary, the block boundary."""
    prob = _cached(("po", n, stereo), lambda: synth.pose_only(num_cameras=1, points_per_camera=n, stereo=stereo))
    assert prob.num_edges == n
    _pin(_opt(g2o_amd_mod, prob, None, None, 0), prob, E_STEREO if stereo else E_MONO, f"pose_only{n}")


def _records(prob, uniform):
    (es,) = prob.edges
    info, par = es.info.copy(), es.params.copy()
    if uniform:
        info[:] = info[0]
        par[:, 3:] = par[0, 3:]
    else:
        k = np.arange(len(info))
        info = info * (1 + 0.01 * k)[:, None, None]
        par[:, 3] += 0.25 * k
    return synth.Problem(prob.name + ("_u" if uniform else "_v"), prob.vertices,
                         [synth.EdgeSet(es.etype, es.v0, es.v1, es.meas, info, par)], prob.pose_dim, prob.landmark_dim)


@pytest.mark.parametrize("uniform", [True, False])
def test_edge_chi2_record_paths(g2o_amd_mod, uniform):
    """One shared information / intrinsics record for the whole set, and records that differ per edge."""
    prob = _records(synth.pose_only(num_cameras=2, points_per_camera=40), uniform)
    _pin(_opt(g2o_amd_mod, prob, None, None, 0), prob, E_MONO, prob.name)
    ba = _records(_ba(), uniform)
    _pin(_opt(g2o_amd_mod, ba, None, None, 0), ba, E_BA, ba.name)


def test_edge_chi2_sum_and_robust_kernel(g2o_amd_mod):
    """Every level 0, no robust kernel: the per-edge values add up to chi2() (another summation order: 1e-12). With
    Huber on the type edge_chi2 stays the raw e^T Omega e, bit for bit, while chi2() is the robust one."""
    prob = _cached("pins", _pin_cases)["prior_xyz"][0]
    opt = _opt(g2o_amd_mod, prob, None, None, 0)
    raw = {t: opt.edge_chi2(t) for t in (E_BA, synth.E_XYZ_PRIOR)}
    total, chi = sum(float(v.sum()) for v in raw.values()), opt.chi2()
    print(f"sum of edge_chi2 {total:.17g} chi2() {chi:.17g}")
    assert abs(total - chi) <= 1e-12 * chi
    opt.set_robust_kernel(E_BA, "Huber", 2.0)
    assert opt.chi2() < chi
    assert np.array_equal(opt.edge_chi2(E_BA), raw[E_BA])


# ---------------------------------------------------------------- 4: the depth flag
def _behind_cases():
    out = {}
    for name, prob, etype in (("ba_mono", _ba(), E_BA),
                              ("ba_stereo", synth.ba_stereo(num_cameras=6, num_points=40, obs_per_point=4), E_SBA),
                              ("pose_only", synth.pose_only(num_cameras=3, points_per_camera=20), E_MONO),
                              ("pose_only_stereo", synth.pose_only(num_cameras=3, points_per_camera=20, stereo=True), E_STEREO)):
        es = R.edge_set(prob, etype)
        if etype in (E_BA, E_SBA):  # the first observation of five landmarks; every edge of them follows
            rows = [int(np.flatnonzero(es.v0 == i)[0]) for i in np.unique(es.v0)[[2, 9, 17, 25, 33]]]
            moved = np.isin(es.v0, es.v0[rows])
        else:
            rows = [1, 7, 19, 20, 44, 59]
            moved = np.zeros(len(es.v0), bool)
            moved[rows] = True
        out[name] = (R.behind_camera(prob, etype, rows), etype, moved)
    return out


@pytest.mark.parametrize("name", ["ba_mono", "ba_stereo", "pose_only", "pose_only_stereo"])
def test_depth_flag(g2o_amd_mod, name):
    prob, etype, moved = _cached("behind", _behind_cases)[name]
    z = R.depth_z(prob, etype)
    assert np.all(z[moved] <= -0.1) and np.all(z[~moved] >= 0.1) and moved.any() and not moved.all()
    opt = _opt(g2o_amd_mod, prob, None, None, 0)
    chi, dp = opt.edge_chi2(etype, depth=True)
    assert dp.dtype == bool and np.array_equal(dp, z > 0)
    assert np.all(np.isfinite(chi))


def test_depth_on_a_type_without_it(g2o_amd_mod):
    prob = pose_edges_ref.se3_chain(5)[0]
    opt = _opt(g2o_amd_mod, prob, None, None, 0)
    chi, dp = np.zeros(5), np.zeros(5, np.uint8)
    L = g2o_amd_mod.lib()
    assert L.g2ohip_edge_chi2(opt.h, synth.E_SE3_QUAT, chi.ctypes.data, dp.ctypes.data) == ERR_ARG
    assert L.g2ohip_classify_edges(opt.h, synth.E_SE3_QUAT, 1.0, 1, 0, 1, None) == ERR_ARG
    assert L.g2ohip_edge_chi2(opt.h, synth.E_SE3_QUAT, chi.ctypes.data, None) == 0


# ---------------------------------------------------------------- 5: classification
def _classify_check(mod, prob, etype, tag):
    chi = R.edge_chi2(prob, etype)
    z = R.depth_z(prob, etype)
    thr, gap = R.gap_threshold(chi)
    print(f"{tag}: threshold {thr:.6g} in a gap of {gap:.2e} relative")
    assert gap >= 1e-9
    for check_depth in (False, True):
        opt = _opt(mod, prob, None, None, 0)
        counts = opt.classify_edges(etype, thr, check_depth=check_depth)
        want_lv, want_counts = R.classify(chi, thr, z if check_depth else None)
        assert counts == want_counts, (tag, check_depth, counts, want_counts)
        assert np.array_equal(opt.edge_levels(etype), want_lv), (tag, check_depth)
    return chi, z, thr


@pytest.mark.parametrize("n", [1, 64, 65, 257])
def test_classify_sizes(g2o_amd_mod, n):
    """Levels and counts at one wave, the wave boundary and the block boundary of the count reduction."""
    prob = _cached(("po", n, False), lambda: synth.pose_only(num_cameras=1, points_per_camera=n))
    if n > 1:
        prob = R.behind_camera(prob, E_MONO, list(range(0, n, 7)))
    _classify_check(g2o_amd_mod, prob, E_MONO, f"pose_only{n}")


@pytest.mark.parametrize("name", ["ba_mono", "ba_stereo", "pose_only_stereo"])
def test_classify_levels_and_counts(g2o_amd_mod, name):
    prob, etype, moved = _cached("behind", _behind_cases)[name]
    chi, z, thr = _classify_check(g2o_amd_mod, prob, etype, name)
    # LEVEL_KEEP on the inlier side (local BA only ever demotes): earlier level-1 edges stay at 1, inliers included
    opt = _opt(g2o_amd_mod, prob)
    before = np.zeros(len(chi), np.int32)
    inl = np.flatnonzero(chi < thr)[:5]
    before[inl] = 1
    opt.set_edge_levels(etype, before[inl], idx=inl)
    opt.initialize_optimization(0)
    opt.classify_edges(etype, thr, inlier_level=g2o_amd_mod.LEVEL_KEEP, outlier_level=1)
    want = R.classify(chi, thr, None, before, R.LEVEL_KEEP, 1)[0]
    got = opt.edge_levels(etype)
    assert np.array_equal(got, want) and np.all(got[inl] == 1)
    # both sides kept: the counts alone, no level moves
    assert opt.classify_edges(etype, thr, check_depth=True, inlier_level=g2o_amd_mod.LEVEL_KEEP,
                              outlier_level=g2o_amd_mod.LEVEL_KEEP) == R.classify(chi, thr, z)[1]
    assert np.array_equal(opt.edge_levels(etype), want)
    # ... and on the outlier side: only promotions
    opt.classify_edges(etype, thr, inlier_level=0, outlier_level=g2o_amd_mod.LEVEL_KEEP)
    assert np.array_equal(opt.edge_levels(etype), R.classify(chi, thr, None, want, 0, R.LEVEL_KEEP)[0])


# ---------------------------------------------------------------- 6: the pose-optimisation loop
@pytest.mark.parametrize("stereo", [False, True])
def test_pose_optimisation_loop(g2o_amd_mod, stereo):
    """ORB-SLAM's PoseOptimization: four rounds of (estimates back to the start, initializeOptimization(0),
    optimize(10), classify every edge), Huber for the first two rounds. The reference runs the same loop through the
    level-less API: a fresh handle of the current inliers per round, chi2 per edge from numpy at the estimates read
    back."""
    etype, thr = (E_STEREO, 7.815) if stereo else (E_MONO, 5.991)
    prob = structure_only_ref.with_outliers(synth.pose_only(num_cameras=2, points_per_camera=60, stereo=stereo), etype,
                                            every=9, shift=40.0)
    (es,), (cams,) = prob.edges, prob.vertices
    n = len(es.v0)
    shifted = np.zeros(n, bool)
    shifted[::9] = True
    row = np.searchsorted(cams.ids, es.v0)

    dev = _opt(g2o_amd_mod, prob, "lm_hip_var")
    ref_levels = np.zeros(n, np.int32)
    ref_state = None
    for rnd in range(4):
        kind = ("Huber", np.sqrt(thr)) if rnd < 2 else ("none", 1.0)
        # the device loop
        dev.set_estimates(cams.vtype, cams.est)
        dev.set_robust_kernel(etype, *kind)
        dev.initialize_optimization(0)
        dev.optimize(10)
        counts = dev.classify_edges(etype, thr, inlier_level=0, outlier_level=1)
        # the reference loop
        ref = _opt(g2o_amd_mod, R.subproblem(prob, {etype: ref_levels == 0}), "lm_hip_var")
        ref.set_robust_kernel(etype, *kind)
        ref.initialize_optimization()
        ref.optimize(10)
        T = ref.estimates(cams.vtype)[row]
        e = expmap_ref.pose_only_error(etype, T, es.params, es.meas)
        chi = np.einsum("ni,nij,nj->n", e, es.info, e)
        margin = np.abs(chi - thr).min() / thr
        print(f"round {rnd}: {int((chi > thr).sum())} outliers, nearest chi2 {margin:.2e} of the threshold away")
        assert margin > 1e-4, "a reference chi2 at the threshold: choose another seed"
        ref_levels = (chi > thr).astype(np.int32)
        ref_state = ref.minimal_state()
        assert np.array_equal(dev.edge_levels(etype), ref_levels), rnd
        assert counts["bad"] == int(ref_levels.sum()) and counts["depth_failed"] == 0
    assert np.all(ref_levels[shifted] == 1)
    got = dev.minimal_state()
    assert np.linalg.norm(got - ref_state) <= 1e-6 * np.linalg.norm(ref_state)


# ---------------------------------------------------------------- 7: refusals and arguments
def test_arguments_and_refusals(g2o_amd_mod):
    L = g2o_amd_mod.lib()
    prob = synth.pose_only(num_cameras=2, points_per_camera=10)
    n = prob.num_edges
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)

    def set_levels(etype, idx, lv):
        ix = None if idx is None else np.ascontiguousarray(idx, np.int32)
        lv = np.ascontiguousarray(lv, np.int32)
        return L.g2ohip_set_edge_levels(opt.h, etype, len(lv), None if ix is None else ix.ctypes.data, lv.ctypes.data)

    assert set_levels(E_MONO, [0, 3], [1, 2]) == 0
    want = np.zeros(n, np.int32)
    want[[0, 3]] = [1, 2]
    for bad in ((E_MONO, [0, n], [1, 1]), (E_MONO, [-1], [1]), (E_MONO, [4, 4], [1, 1]), (E_MONO, [5], [-1]),
                (E_MONO, None, np.zeros(n - 1)), (E_STEREO, [0], [1]), (99, [0], [1])):
        assert set_levels(*bad) == ERR_ARG, bad
        assert np.array_equal(opt.edge_levels(E_MONO), want)  # nothing changed
    assert L.g2ohip_get_edge_levels(opt.h, E_STEREO, None, 0) == ERR_ARG
    chi = np.zeros(n)
    assert L.g2ohip_edge_chi2(opt.h, E_MONO, chi.ctypes.data, None) == ERR_STATE  # no initialisation yet
    assert L.g2ohip_classify_edges(opt.h, E_MONO, 1.0, 0, 0, 1, None) == ERR_STATE
    opt.initialize_optimization(0)
    assert L.g2ohip_edge_chi2(opt.h, E_STEREO, chi.ctypes.data, None) == ERR_ARG  # no edge of the type
    assert L.g2ohip_classify_edges(opt.h, E_MONO, 1.0, 0, -3, 1, None) == ERR_ARG  # a negative level
    assert np.array_equal(opt.edge_levels(E_MONO), want)
    with pytest.raises(g2o_amd_mod.G2OHipError):  # nothing on level 7: an empty graph to the optimizer
        opt.initialize_optimization(7)

    # a host-Jacobian type: the host holds those errors itself
    hp, back = expmap_ref.hostj_version(prob)
    g = expmap_ref.Graph(prob)
    hj = g2o_amd_mod.SparseOptimizer(0).add_problem(hp)
    hj.set_host_edge_callback(lambda etype, with_jac: g.payload(back[etype], {v.vtype: hj.estimates(v.vtype) for v in prob.vertices}))
    (ht,) = back
    hj.set_edge_levels(ht, [1], idx=[2])  # levels themselves work for host-J types
    hj.initialize_optimization(0)
    assert L.g2ohip_edge_chi2(hj.h, ht, chi.ctypes.data, None) == ERR_UNSUPPORTED
    assert "host" in g2o_amd_mod.last_error()
    assert L.g2ohip_classify_edges(hj.h, ht, 1.0, 0, 0, 1, None) == ERR_UNSUPPORTED

    # a sharded handle
    sh = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    sh.set_comm_local(uuid.uuid4().hex, 0, 2)
    assert L.g2ohip_edge_chi2(sh.h, E_MONO, chi.ctypes.data, None) == ERR_UNSUPPORTED
    assert "shard" in g2o_amd_mod.last_error()
    assert L.g2ohip_classify_edges(sh.h, E_MONO, 1.0, 0, 0, 1, None) == ERR_UNSUPPORTED


def test_mistyped_edge_on_another_level_is_refused(g2o_amd_mod):
    """The vertex types of every edge are checked at initialisation, the edges set aside included: the all-edges view
    and structure-only index the state arrays through them. An EdgeSE3ProjectXYZ whose second vertex is a point (its
    local index far past the six cameras), on level 1, is refused as it is on level 0."""
    prob = _ba()
    (es,), pts = prob.edges, prob.vertices[1]
    bad = synth.EdgeSet(es.etype, np.append(es.v0, pts.ids[0]), np.append(es.v1, pts.ids[39]),
                        np.vstack([es.meas, es.meas[:1]]), np.concatenate([es.info, es.info[:1]]),
                        np.vstack([es.params, es.params[:1]]))
    L = g2o_amd_mod.lib()
    n = len(bad.v0)
    for level_of_bad in (1, 0):
        opt = g2o_amd_mod.SparseOptimizer(0).add_problem(
            synth.Problem("mistyped", prob.vertices, [bad], prob.pose_dim, prob.landmark_dim))
        opt.set_edge_levels(E_BA, [level_of_bad], idx=[n - 1])
        assert L.g2ohip_initialize_level(opt.h, 0) == ERR_UNSUPPORTED, level_of_bad
        assert "vertex type" in g2o_amd_mod.last_error()
        chi = np.zeros(n)
        assert L.g2ohip_edge_chi2(opt.h, E_BA, chi.ctypes.data, None) == ERR_STATE  # nothing was initialised
        assert L.g2ohip_structure_only_calc(opt.h, 0, None, 1, 10, None) == ERR_STATE


def test_hostj_levels_equal_twin(g2o_amd_mod):
    """A host-Jacobian set takes levels like any other: the callback still covers every edge of the type."""
    prob = synth.pose_only(num_cameras=2, points_per_camera=12)
    levels = R.third_levels(prob, 5)[E_MONO]

    def hostj(p, lv):
        hp, back = expmap_ref.hostj_version(p)
        g = expmap_ref.Graph(p)
        o = g2o_amd_mod.SparseOptimizer(0).add_problem(hp)
        o.set_host_edge_callback(lambda etype, with_jac: g.payload(back[etype], {v.vtype: o.estimates(v.vtype) for v in p.vertices}))
        (ht,) = back
        if lv is not None:
            o.set_edge_levels(ht, lv)
        o.initialize_optimization(0)
        n, st = o.optimize(3)
        return n, [s.chi2 for s in st], o.minimal_state()

    a = hostj(prob, levels)
    b = hostj(R.subproblem(prob, {E_MONO: levels == 0}), None)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_update_initialization_filters_by_the_level(g2o_amd_mod):
    """Online mode on a handle with levels: the edges added later arrive at level 0 and join, one of them moved to
    level 1 first stays out, the earlier edges keep their state. The twin holds the level-0 edges only."""
    from test_online import grow_split
    before, add_v, add_e, _ = grow_split(synth.se2_grid(60))
    (es0,), (es1,) = before.edges, add_e
    lv0 = np.zeros(len(es0.v0), np.int32)
    loops = np.flatnonzero(np.abs(es0.v1 - es0.v0) != 2)  # (ids are doubled: the odometry edges join i and i + 2)
    lv0[loops[::3]] = 1
    out1 = int(np.flatnonzero(np.abs(es1.v1 - es1.v0) != 2)[1])  # a loop closure among the added edges ([0] joins the parts)
    keep1 = np.ones(len(es1.v0), bool)
    keep1[out1] = False

    def run(first, second, levels):
        o = _opt(g2o_amd_mod, first, "lm_hip_var", levels, 0)
        o.optimize(2)
        for v in add_v:
            o.add_vertices(v)
        o.add_edges(second)
        if levels:
            assert np.array_equal(o.edge_levels(synth.E_SE2)[len(lv0):], np.zeros(len(es1.v0), np.int32))
            o.set_edge_levels(synth.E_SE2, [1], idx=[len(lv0) + out1])
        o.update_initialization()
        n, st = o.optimize(3)
        return n, [x.chi2 for x in st], [x.levenbergIterations for x in st], o.minimal_state()

    a = run(before, es1, {synth.E_SE2: lv0})
    b = run(R.subproblem(before, {synth.E_SE2: lv0 == 0}), R.subproblem(
        synth.Problem("added", [], [es1], 3, 0), {synth.E_SE2: keep1}).edges[0], None)
    assert a[0] == b[0] == 3 and a[2] == b[2]
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])


# ---------------------------------------------------------------- 8: landmark shards
def test_levels_on_two_local_ranks(g2o_amd_mod):
    prob = _ba()
    levels = R.ba_levels(prob, 11)[0]
    nranks, iters = 2, 4
    key = uuid.uuid4().hex
    opts = [_opt(g2o_amd_mod, prob, "lm_hip_fix6_3", levels) for _ in range(nranks)]
    for r, o in enumerate(opts):
        o.set_comm_local(key, r, nranks)
        o.initialize_optimization(0)
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
    assert not any(t.is_alive() for t in th), "a rank did not finish"
    assert not errs, errs
    single = _opt(g2o_amd_mod, prob, "lm_hip_fix6_3", levels, 0)
    n1, st1 = single.optimize(iters)
    for r in range(nranks):
        n, st = res[r]
        assert n == n1
        for a, b in zip(st, st1):
            assert abs(a.chi2 - b.chi2) <= 1e-9 * abs(b.chi2), (a.chi2, b.chi2)
    x, _ = gather_sharded_state(prob, opts)
    x1 = single.minimal_state()
    assert np.linalg.norm(x - x1) <= 1e-9 * np.linalg.norm(x1)


# ---------------------------------------------------------------- 9: structure-only ignores levels
def test_structure_only_ignores_levels(g2o_amd_mod):
    """StructureOnlySolver::calc walks v->edges(): every edge of an active landmark whatever its level."""
    prob = structure_only_ref.perturbed(_ba(), 0.05)
    levels = R.third_levels(prob, 3)
    es = prob.edges[0]
    for i in np.unique(es.v0):  # every landmark keeps an observation on level 0: the same active landmarks
        assert np.any(levels[E_BA][es.v0 == i] == 0)
    a = _opt(g2o_amd_mod, prob, "lm_hip_fix6_3", levels, 0)
    b = _opt(g2o_amd_mod, prob, "lm_hip_fix6_3", None, 0)
    ca, cb = a.structure_only(iterations=3), b.structure_only(iterations=3)
    assert ca == cb and ca["accepted"] > 0
    assert np.array_equal(a.estimates(synth.V_XYZ), b.estimates(synth.V_XYZ))
    assert not np.array_equal(b.estimates(synth.V_XYZ), prob.vertices[1].est)
