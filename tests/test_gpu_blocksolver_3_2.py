"""BlockSolver_3_2 on the device (block_solver.h:188-201): 2D landmark SLAM, SE2 poses (VertexSE2) with XY landmarks
(VertexPointXY) marginalised by the Schur complement, EdgeSE2 odometry and EdgeSE2PointXY observations
(edge_se2_pointxy.h:41-75), the shape of g2o/examples/tutorial_slam2d. The same kernels as BlockSolver_6_3,
instantiated for 3x3 pose and 2x2 landmark blocks, against the oracle's restatement of the reference path.

Tolerances as tests/test_gpu_parity.py: state vector and chi2 within 1e-6 relative of the CSparse oracle (north_star),
stage-level outputs 1e-9 (same fp64 arithmetic in another order).
"""
import threading
import uuid

import numpy as np
import pytest

from g2o_amd import synth

pytestmark = pytest.mark.gpu

RTOL = 1e-6


def _slam2d(n=300):
    return synth.slam2d(n)


def _check_trajectory(opt, st, ref, sr):
    assert len(st) == len(sr)
    for a, b in zip(st, sr):
        assert a.levenbergIterations == b.levenbergIterations
        assert abs(a.chi2 - b.chi2) <= RTOL * abs(b.chi2), (a.chi2, b.chi2)
    xg, xr = opt.minimal_state(), ref.minimal_state()
    assert np.linalg.norm(xg - xr) <= RTOL * np.linalg.norm(xr)


@pytest.mark.parametrize("n,iters", [(300, 6), (3000, 4)])
def test_slam2d_lm_trajectory(g2o_amd_mod, oracle, n, iters):
    prob = _slam2d(n)
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    opt.set_algorithm("lm_hip_fix3_2")
    _, st = opt.optimize(iters)
    ref = oracle.OracleGraph(prob)
    _, sr = ref.optimize(iters, oracle.make_config(threads=8))
    _check_trajectory(opt, st, ref, sr)
    pd, ld, npose, nlm = opt.block_dims()
    assert (pd, ld) == (3, 2)
    assert npose == prob.vertices[0].ids.size - 1 and nlm == prob.vertices[1].ids.size


def test_slam2d_stage_reduced_system(g2o_amd_mod, oracle):
    """buildSystem + setLambda + Schur + solve at one state: b, the reduced system S / bschur and x."""
    prob = _slam2d()
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    ref = oracle.OracleGraph(prob)
    lam = 1e-3
    g = opt.stage(lam)
    r = ref.stage(lam)
    assert g["ok"] == r["ok"] == 1
    for k in ("b", "bschur", "x"):
        assert np.linalg.norm(g[k] - r[k]) <= 1e-9 * np.linalg.norm(r[k]), k
    assert np.linalg.norm(g["Hschur"] - r["Hschur"]) <= 1e-11 * np.linalg.norm(r["Hschur"])


def test_slam2d_gauss_newton(g2o_amd_mod, oracle):
    prob = _slam2d()
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    opt.set_algorithm("gn_hip_fix3_2")
    _, st = opt.optimize(4)
    ref = oracle.OracleGraph(prob)
    _, sr = ref.optimize(4, oracle.make_config(threads=8, gauss_newton=True))
    for a, b in zip(st, sr):
        assert abs(a.chi2 - b.chi2) <= RTOL * abs(b.chi2), (a.chi2, b.chi2)
    xg, xr = opt.minimal_state(), ref.minimal_state()
    assert np.linalg.norm(xg - xr) <= RTOL * np.linalg.norm(xr)


def test_slam2d_pcg3_2(g2o_amd_mod, oracle):
    """lm_pcg3_2 (solver_pcg.cpp:91-98): block-Jacobi PCG on the 3x3-block Schur complement; an iterative solve, so
    the LM converges to the direct solver's optimum rather than following its trajectory step for step."""
    prob = _slam2d()
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    opt.set_algorithm("lm_pcg3_2")
    _, st = opt.optimize(10)
    chi = [s.chi2 for s in st]
    assert all(b <= a * (1 + 1e-12) for a, b in zip(chi, chi[1:]))
    ref = oracle.OracleGraph(prob)
    _, sr = ref.optimize(10, oracle.make_config(threads=8))
    # the PCG stops at its relative residual tolerance (linear_solver_pcg.hpp:129-159): optimum within 1e-5
    assert abs(chi[-1] - sr[-1].chi2) <= 1e-5 * sr[-1].chi2, (chi[-1], sr[-1].chi2)


def test_slam2d_marginals(g2o_amd_mod, oracle):
    """computeMarginals (block_solver.hpp:451-460) on a 3_2 graph: (i, i) and (i-1, i) blocks of Hpp^-1."""
    prob = _slam2d()
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    opt.set_algorithm("lm_hip_fix3_2")
    opt.initialize_optimization()
    opt.build_structure()
    opt.build_system()
    pd, _, npose, _ = opt.block_dims()
    pat = [(i, i) for i in range(npose)] + [(i - 1, i) for i in range(1, npose)]
    blocks = opt.compute_marginals(pat)
    assert blocks is not None and len(blocks) == len(pat)
    ref = oracle.OracleGraph(prob)
    r = ref.stage(0.0)
    Hpp, _, _ = ref.hessian_dense(r["np"], r["nl"])
    Hinv = np.linalg.inv(Hpp)
    num = den = 0.0
    for (i, j), B in blocks.items():
        R = Hinv[i * pd:(i + 1) * pd, j * pd:(j + 1) * pd]
        num += float(np.sum((B - R) ** 2))
        den += float(np.sum(R ** 2))
    assert np.sqrt(num / den) <= 1e-9


def test_slam2d_g2o_file_roundtrip(g2o_amd_mod, oracle, tmp_path):
    """VERTEX_XY / EDGE_SE2_XY tags (types_slam2d.cpp:40,46): the device writer's file read by the oracle's reader and
    the device reader, same chi2; then the same optimization from the file."""
    prob = _slam2d()
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    path = str(tmp_path / "slam2d.g2o")
    opt.save(path)
    text = open(path).read()
    assert "VERTEX_XY " in text and "EDGE_SE2_XY " in text and "FIX 0" in text
    ref = oracle.OracleGraph.load(path, marginalize_xyz=True)
    chi_ref = ref.chi2()
    back = g2o_amd_mod.SparseOptimizer(0)
    back.load(path, marginalize_xyz=True)
    assert abs(back.chi2() - chi_ref) <= 1e-12 * chi_ref
    assert abs(opt.chi2() - chi_ref) <= 1e-12 * chi_ref
    _, st = back.optimize(3)
    _, sr = ref.optimize(3, oracle.make_config(threads=8))
    _check_trajectory(back, st, ref, sr)


def test_slam2d_sharded(g2o_amd_mod, oracle):
    """Landmark shards with a pose-pose edge set: odometry edges are assembled once (rank 0), the
    observation edges by the rank owning their landmark, the reduced system summed over ranks."""
    prob = _slam2d()
    nranks, iters = 2, 4
    key = uuid.uuid4().hex
    opts = [g2o_amd_mod.SparseOptimizer(0).add_problem(prob) for _ in range(nranks)]
    for r, o in enumerate(opts):
        o.set_algorithm("lm_hip_fix3_2")
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
    ref = oracle.OracleGraph(prob)
    _, sr = ref.optimize(iters, oracle.make_config(threads=8))
    for r in range(nranks):
        _, st = res[r]
        for a, b in zip(st, sr):
            assert a.levenbergIterations == b.levenbergIterations
            assert abs(a.chi2 - b.chi2) <= RTOL * b.chi2
    # poses (ids first, 3 each) from rank 0; landmarks (2 each) from their owning shard
    N, L = prob.vertices[0].ids.size, prob.vertices[1].ids.size
    states = [o.minimal_state() for o in opts]
    x = states[0].copy()
    for r in range(nranks):
        a, b = L * r // nranks, L * (r + 1) // nranks
        x[3 * N + 2 * a: 3 * N + 2 * b] = states[r][3 * N + 2 * a: 3 * N + 2 * b]
    assert np.array_equal(states[1][:3 * N], states[0][:3 * N])
    xr = ref.minimal_state()
    assert np.linalg.norm(x - xr) <= RTOL * np.linalg.norm(xr)


# ---- row chunks split into parts with 3x3 blocks: schur_row_store<3>'s partial-block store (odd PD: the second column
# half holds one column only) and k_schur_part_sum<3> ----
_DENSE = {}  # the dense problem, its oracle results and the single-GPU run: computed once, shared, left unchanged


def _slam2d_dense():
    """slam2d(60, landmarks_per_cell=2.0, sensor_range=4.0, max_obs_per_pose=64): 59 free poses, 538 landmarks, 3840
    observations, up to 28 off-diagonal blocks per row. A row chunk is split only when it stages >= 512 blocks (its own
    observations + their partners in the chunk): 14 of the 58 chunks do (the largest stages 792), so 14 part groups with
    the target forced on one GPU; on 2 ranks with the default target 14 / 0, on 3 ranks 10 / 0 / 0. The pose count does
    not matter for the density (30 poses: 11 such chunks); 48 observations per pose leave 2 chunks, sensor range 3
    leaves 7; slam2d(300) with its defaults stages at most 143 blocks per chunk."""
    if "prob" not in _DENSE:
        _DENSE["prob"] = synth.slam2d(60, landmarks_per_cell=2.0, sensor_range=4.0, max_obs_per_pose=64)
    return _DENSE["prob"]


def _dense_oracle(oracle, iters):
    key = ("oracle", iters)
    if key not in _DENSE:
        ref = oracle.OracleGraph(_slam2d_dense())
        _, sr = ref.optimize(iters, oracle.make_config(threads=8))
        _DENSE[key] = ([(s.chi2, s.levenbergIterations) for s in sr], ref.minimal_state())
    return _DENSE[key]


def _run_3_2(g2o_amd_mod, prob, iters):
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    opt.set_algorithm("lm_hip_fix3_2")
    n, st = opt.optimize(iters)
    return opt, n, [(s.chi2, s.levenbergIterations) for s in st], opt.minimal_state()


def _check_against_oracle(traj, x, oracle_traj, xr):
    assert len(traj) == len(oracle_traj)
    for (chi, trials), (rchi, rtrials) in zip(traj, oracle_traj):
        assert trials == rtrials
        assert abs(chi - rchi) <= RTOL * abs(rchi), (chi, rchi)
    assert np.linalg.norm(x - xr) <= RTOL * np.linalg.norm(xr)


def test_slam2d_row_parts(g2o_amd_mod, oracle, monkeypatch):
    """Split row chunks (G2OHIP_SCHUR_SPLIT_TASKS forced, one GPU) on a BlockSolver_3_2 graph dense enough for them
    (_slam2d_dense: 14 part groups): the reduced system and solution against the oracle, every entry of Hschur and
    bschur within 1e-13 of the matrix scale of the unsplit pass (a differently ordered f64 sum of O(100) terms of that
    scale, as tests/test_gpu_schur_split.py), a 5-iteration trajectory against the unsplit pass and the oracle."""
    prob = _slam2d_dense()
    lam, iters = 1e-3, 5
    r = oracle.OracleGraph(prob).stage(lam)
    out, runs = {}, {}
    for target in ("1000000", "0"):
        monkeypatch.setenv("G2OHIP_SCHUR_SPLIT_TASKS", target)
        opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
        opt.set_algorithm("lm_hip_fix3_2")
        g = out[target] = opt.stage(lam)
        info = opt.factor_info()
        assert opt.block_dims()[:2] == [3, 2]
        if target == "0":
            assert info["schur_part_groups"] == 0 and info["schur_part_blocks"] == 0, info
        else:
            assert info["schur_part_groups"] > 0 and info["schur_part_blocks"] > 0, info
        assert g["ok"] == r["ok"] == 1
        for k in ("b", "bschur", "x"):
            assert np.linalg.norm(g[k] - r[k]) <= 1e-9 * np.linalg.norm(r[k]), (target, k)
        assert np.linalg.norm(g["Hschur"] - r["Hschur"]) <= 1e-11 * np.linalg.norm(r["Hschur"]), target
        runs[target] = _run_3_2(g2o_amd_mod, prob, iters)
    for k in ("Hschur", "bschur"):
        x, y = np.asarray(out["1000000"][k]), np.asarray(out["0"][k])
        scale = np.abs(y).max()
        err = np.abs(x - y).max() / scale
        print(f"{k}: split parts against the unsplit pass, max entry error / scale {err:.3e}")
        assert err <= 1e-13, (k, err)
    (_, n1, t1, x1), (_, n0, t0, x0) = runs["1000000"], runs["0"]
    assert n1 == n0 == iters
    assert [t for _, t in t1] == [t for _, t in t0]
    assert np.allclose([c for c, _ in t1], [c for c, _ in t0], rtol=1e-10, atol=0)
    assert np.linalg.norm(x1 - x0) <= 1e-10 * np.linalg.norm(x0)
    _check_against_oracle(t1, x1, *_dense_oracle(oracle, iters))


@pytest.mark.parametrize("nranks", [2, 3])
def test_slam2d_dense_sharded(g2o_amd_mod, oracle, nranks):
    """Landmark shards of the dense graph with the sharded path's default split target (2048 tasks; nothing forced):
    some rank splits row chunks, and the run follows the single-GPU trajectory (state 1e-9) and the oracle (1e-6)."""
    prob = _slam2d_dense()
    iters = 4
    key = uuid.uuid4().hex
    opts = [g2o_amd_mod.SparseOptimizer(0).add_problem(prob) for _ in range(nranks)]
    for r, o in enumerate(opts):
        o.set_algorithm("lm_hip_fix3_2")
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
        t.join(timeout=300)
    assert not errs, errs
    info = [o.factor_info() for o in opts]
    groups = [int(i["schur_part_groups"]) for i in info]
    print("schur_part_groups per rank:", groups, "schur_tasks:", [int(i["schur_tasks"]) for i in info])
    assert any(g > 0 for g in groups), info
    assert all(i["schur_part_blocks"] > 0 for i in info if i["schur_part_groups"] > 0), info
    if "single" not in _DENSE:
        _DENSE["single"] = _run_3_2(g2o_amd_mod, prob, iters)[1:]
    n1, traj1, xs = _DENSE["single"]
    oracle_traj, xr = _dense_oracle(oracle, iters)
    # poses (ids first, 3 each) from rank 0; each landmark (2 each, id order) from the rank whose shard holds it
    N, lm_ids = prob.vertices[0].ids.size, np.asarray(prob.vertices[1].ids)
    states = [o.minimal_state() for o in opts]
    x = states[0].copy()
    held = np.zeros(lm_ids.size, np.int32)
    for o, s in zip(opts, states):
        assert np.array_equal(s[:3 * N], states[0][:3 * N])
        lid = o.local_landmark_ids()
        k = np.searchsorted(lm_ids, lid)
        assert np.array_equal(lm_ids[k], lid)
        held[k] += 1
        rows = (3 * N + 2 * k[:, None] + np.arange(2)[None, :]).ravel()
        x[rows] = s[rows]
    assert np.all(held == 1)
    for r in range(nranks):
        n, st = res[r]
        assert n == n1 == iters
        traj = [(s.chi2, s.levenbergIterations) for s in st]
        assert [t for _, t in traj] == [t for _, t in traj1]
        _check_against_oracle(traj, x, oracle_traj, xr)
    assert np.linalg.norm(x - xs) <= 1e-9 * np.linalg.norm(xs)
