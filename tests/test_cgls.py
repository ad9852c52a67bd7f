"""The fork's matrix-free solver lm_pcg6_3_eigen (JacobiSolver_6_3 + LinearSolverPCGEigen).

CPU: the numpy restatement (oracle/cgls_ref.py) solves the damped normal equations exactly when eta -> 0 and its LM
loop reduces chi2. GPU: the device CGLS (g2o_amd/csrc/cgls.hip) behind the LM loop follows the restatement's LM
trajectory (chi2 and trial counts per iteration, final state) within the north_star 1e-6; "parity unpinned" against
reference outputs (the fork's solver needs Eigen).

One solve at a time (the EDGE_PROBLEMS below): the device's b, x and iteration count of a single
buildSystem / setLambda / solve against the restatement on problems built for the solver's structural edges — fixed
points (the fused group's edge order puts their edges first), cameras with more observations than one pass of the
256-thread camera loops, points with 1, 0-camera and > 64 observations, and informations other than the identity.
"""
import math

import numpy as np
import pytest

import cgls_ref
from g2o_amd import synth

RTOL = 1e-6
BTOL = 1e-12  # b and max diag(J^T J): the same sums in another order (the suite's chi2 pin)
# the stop test gamma < eta gamma_0 is decided identically on both sides only when gamma is not within rounding (x
# RTOL) of the threshold: asserted on the CPU for every case the GPU test counts iterations of
STOP_MARGIN = 1e-3
LAM_SCALES = (1e-3, 10.0)
ETAS = (0.1, 1e-3)
# eta -> 0 against np.linalg.solve: the loop stops at gamma < 1e-20 gamma_0, a preconditioned residual 1e-10 of the
# first; the preconditioned normal matrix has its spectrum in (0, 2) (two block groups, each an identity on its
# diagonal) and lambda >= 1e-3 max diag keeps the smallest eigenvalue above lambda / (6 max diag + lambda) > 1.6e-4,
# so the error is below 1e-10 * 2 / 1.6e-4 = 1.25e-6 of the solution (the measured distances are 1e-11 to 1e-9)
DIRECT_RTOL = 1.25e-6


def _tiny():
    return synth.ba(num_cameras=12, num_points=200, obs_per_point=5, window=8)


def _variant(base, name, fixed=None, info=None, keep=None):
    """`base` with the points' fixed flags, the edges' information or a subset of the edges replaced."""
    cams, pts = base.vertices
    if fixed is not None:
        pts = synth.VertexSet(pts.vtype, pts.ids, pts.est, np.asarray(fixed, np.int32), pts.marginalized)
    e = base.edges[0]
    info = e.info if info is None else np.ascontiguousarray(info)
    if keep is None:
        keep = np.ones(len(e.v0), bool)
    ev = synth.EdgeSet(e.etype, e.v0[keep], e.v1[keep], e.meas[keep], info[keep], e.params[keep])
    return synth.Problem(base.name + "_" + name, [cams, pts], [ev], 6, 3)


def _fixed_points(last):
    base = synth.ba(12, 150, obs_per_point=5, window=8)
    fixed = np.zeros(150, np.int32)
    if last:
        fixed[-22:] = 1  # as many as [::7], but the highest ids
    else:
        fixed[::7] = 1
    return _variant(base, "fixedlast" if last else "fixedpts", fixed=fixed)


def _wide_cameras(trim):
    """Every point sees all six cameras (two fixed): 400 observations per free camera, two passes of the 256-wide
    camera loops, the second partial. Trimmed: free cameras with exactly 256, 257 and 1 observations (and one with
    400); every point keeps the two fixed cameras' observations."""
    base = synth.ba(6, 400, obs_per_point=6, window=6)
    if not trim:
        return base
    e = base.edges[0]
    cam_ids = base.vertices[0].ids
    keep = np.ones(len(e.v0), bool)
    for cam, count in ((cam_ids[2], 256), (cam_ids[3], 257), (cam_ids[4], 1)):
        k = np.nonzero(e.v1 == cam)[0]
        keep[k[count:]] = False
    return _variant(base, "trim", keep=keep)


def _ragged_points():
    """256 points, 70 cameras (two fixed). Point 0 keeps all 70 observations (> 64: a landmark split over wave
    chunks), point 1 a single observation by a free camera, point 2 only the two fixed cameras (its camera rows are
    all zero), every other point four."""
    base = synth.ba(70, 256, obs_per_point=70, window=70)
    e = base.edges[0]
    cam0, pt0 = int(base.vertices[0].ids[0]), int(base.vertices[1].ids[0])
    c, p = e.v1 - cam0, e.v0 - pt0
    keep = np.zeros(len(p), bool)
    for j in range(4):
        keep |= (c == (7 * p + 17 * j + 2) % 70)
    keep[p == 0] = True
    keep[p == 1] = c[p == 1] == 33
    keep[p == 2] = c[p == 2] < 2
    return _variant(base, "ragged", keep=keep)


def _info(kind):
    base = synth.ba(12, 150, obs_per_point=5, window=8)
    n = base.num_edges
    rng = np.random.default_rng(11)
    if kind == "a":  # Omega = w_e I
        info = rng.uniform(0.25, 4.0, n)[:, None, None] * np.eye(2)[None]
    elif kind == "b":  # a random SPD, non-diagonal Omega per edge
        A = rng.standard_normal((n, 2, 2)) * 0.6
        info = 0.3 * np.eye(2)[None] + np.einsum("nij,nkj->nik", A, A)
    else:  # one Omega != I for every edge: the single shared record
        info = np.broadcast_to(np.array([[2.5, 0.4], [0.4, 0.6]]), (n, 2, 2)).copy()
    return _variant(base, "info" + kind, info=info)


EDGE_PROBLEMS = {
    "fixed_points": lambda: _fixed_points(False),
    "fixed_last": lambda: _fixed_points(True),
    "wide_cameras": lambda: _wide_cameras(False),
    "wide_trimmed": lambda: _wide_cameras(True),
    "ragged_points": _ragged_points,
    "info_scalar": lambda: _info("a"),
    "info_spd": lambda: _info("b"),
    "info_shared": lambda: _info("c"),
}
DIRECT_PROBLEMS = ("fixed_points", "info_spd")  # the eta -> 0 check on the device
# (problem, lambda scale) -> 10 x the restatement's own distance to the direct solve, measured on the CPU (see
# test_gpu_cgls_solve_reaches_direct_solution)
DIRECT_BOUND = {("fixed_points", 1e-3): 1.112e-10, ("fixed_points", 10.0): 1.834e-10,
                ("info_spd", 1e-3): 9.543e-11, ("info_spd", 10.0): 2.702e-10}
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _problem(name):
    return _cached(("prob", name), EDGE_PROBLEMS[name])


def _system(oracle, name):
    """(J, b, ncam, npt, max diag(J^T J)) of a problem at its initial estimates; computed once, never modified."""
    def make():
        prob = _problem(name)
        host = oracle.OracleGraph(prob)
        host.chi2()
        J, b, nc, npt = cgls_ref.linear_system(host, prob)
        J.setflags(write=False)
        b.setflags(write=False)
        return J, b, nc, npt, float(np.max(np.einsum("ij,ij->j", J, J)))
    return _cached(("sys", name), make)


def _solve_ref(oracle, name, scale, eta):
    """(x, iterations, gammas, lambda) of the restatement."""
    def make():
        J, b, nc, npt, dmax = _system(oracle, name)
        lam = scale * dmax
        g = []
        x, it = cgls_ref.cgls_solve(J, b, nc, npt, math.sqrt(lam), eta, gammas=g)
        x.setflags(write=False)
        return x, it, g, lam
    return _cached(("ref", name, scale, eta), make)


def _direct(oracle, name, scale):
    def make():
        J, b, nc, npt, dmax = _system(oracle, name)
        Jr = J[: J.shape[0] - J.shape[1]]
        xd = np.linalg.solve(Jr.T @ Jr + scale * dmax * np.eye(J.shape[1]), b)
        xd.setflags(write=False)
        return xd
    return _cached(("direct", name, scale), make)


def test_cgls_restatement_direct(oracle):
    prob = _tiny()
    host = oracle.OracleGraph(prob)
    host.chi2()
    J, _, nc, npt = cgls_ref.linear_system(host, prob)
    rng = np.random.default_rng(2)
    b = rng.standard_normal(J.shape[1])
    lam = 0.3
    x, it = cgls_ref.cgls_solve(J, b, nc, npt, math.sqrt(lam), eta=1e-28)
    Jr = J[: J.shape[0] - J.shape[1]]
    xd = np.linalg.solve(Jr.T @ Jr + lam * np.eye(J.shape[1]), b)
    assert 0 < it and np.linalg.norm(x - xd) <= 1e-8 * np.linalg.norm(xd)
    # the forcing term stops early: fewer iterations, an inexact but useful step
    x1, it1 = cgls_ref.cgls_solve(J, b, nc, npt, math.sqrt(lam), eta=0.1)
    assert it1 < it and np.linalg.norm(x1 - xd) < np.linalg.norm(xd)


def test_cgls_restatement_lm(oracle):
    prob = _tiny()
    host = oracle.OracleGraph(prob)
    c0 = host.chi2()
    st = cgls_ref.jacobi_lm(host, prob, 5)
    assert st[-1][0] < 0.05 * c0 and all(s[3] > 0 for s in st)


def test_cgls_restatement_columns_skip_fixed_points():
    """A fixed point has no column: pt_col is -1 on its edges and the free points are numbered by ascending id."""
    prob = _problem("fixed_points")
    cam_col, pt_col, nc, npt = cgls_ref.columns(prob)
    pts, e = prob.vertices[1], prob.edges[0]
    assert nc == 10 and npt == 150 - 22
    fixed_ids = set(pts.ids[pts.fixed != 0].tolist())
    on_fixed = np.array([int(p) in fixed_ids for p in e.v0])
    assert on_fixed.any() and np.all(pt_col[on_fixed] == -1) and np.all(pt_col[~on_fixed] >= 0)
    free_ids = np.sort(pts.ids[pts.fixed == 0])
    assert np.array_equal(free_ids[pt_col[~on_fixed]], e.v0[~on_fixed])


def test_cgls_edge_problems_have_their_edges():
    """The structural properties the problems are built for."""
    def obs_per_free_camera(prob):
        cams, e = prob.vertices[0], prob.edges[0]
        return sorted(int(np.sum(e.v1 == i)) for i in cams.ids[cams.fixed == 0])
    assert obs_per_free_camera(_problem("wide_cameras")) == [400] * 4
    trimmed = _problem("wide_trimmed")
    assert obs_per_free_camera(trimmed) == [1, 256, 257, 400]
    assert np.bincount(trimmed.edges[0].v0 - trimmed.vertices[1].ids[0], minlength=400).min() >= 2
    rag = _problem("ragged_points")
    cams, pts = rag.vertices
    e = rag.edges[0]
    assert len(pts.ids) == 256 and not pts.fixed.any()
    per_pt = np.bincount(e.v0 - pts.ids[0], minlength=256)
    assert per_pt[0] == 70 and per_pt[1] == 1 and per_pt[2] == 2 and per_pt.min() >= 1
    fixed_cams = set(cams.ids[cams.fixed != 0].tolist())
    assert all(int(c) in fixed_cams for c in e.v1[e.v0 == pts.ids[2]])
    assert int(e.v1[e.v0 == pts.ids[1]][0]) not in fixed_cams
    for name in ("info_scalar", "info_spd", "info_shared"):
        info = _problem(name).edges[0].info
        assert np.all(np.linalg.eigvalsh(info) > 0) and np.allclose(info, np.transpose(info, (0, 2, 1)))
    assert np.all(_problem("info_scalar").edges[0].info[:, 0, 1] == 0)
    assert np.all(_problem("info_spd").edges[0].info[:, 0, 1] != 0)
    shared = _problem("info_shared").edges[0].info
    assert np.all(shared == shared[0]) and shared[0, 0, 1] != 0


@pytest.mark.parametrize("name", list(EDGE_PROBLEMS))
def test_cgls_restatement_edge_problems(oracle, name):
    """On every problem of the device's one-solve test: the restatement with eta 1e-20 reproduces the direct solve of
    (J^T J + lambda I) x = b (J: the edge rows; b: jacobi_lm's), and at the etas the device is run with no stop test
    is a near-tie: gamma at the stopping iteration and at the one before it is more than STOP_MARGIN away from
    eta gamma_0 (relative), so that the device's iteration count can be asserted equal."""
    J, b, nc, npt, dmax = _system(oracle, name)
    assert np.linalg.norm(b) > 0 and dmax > 0
    for scale in LAM_SCALES:
        xd = _direct(oracle, name, scale)
        x, it, g, _ = _solve_ref(oracle, name, scale, 1e-20)
        dist = np.linalg.norm(x - xd) / np.linalg.norm(xd)
        print(f"{name} lambda {scale:g} max diag: eta 1e-20 {it} iterations, distance to the direct solve {dist:.3e}")
        assert 0 < it < J.shape[0] and dist <= DIRECT_RTOL, (scale, it, dist)
        for eta in ETAS:
            x1, it1, g, _ = _solve_ref(oracle, name, scale, eta)
            thr, gam = g[0], g[1:]
            assert 0 < it1 < it and len(gam) == it1 + 1 and gam[-1] < thr <= gam[-2]
            margins = [abs(v - thr) / thr for v in gam[-2:]]
            print(f"{name} lambda {scale:g} eta {eta:g}: {it1} iterations, stop margins {margins[0]:.3e} {margins[1]:.3e}")
            assert min(margins) > STOP_MARGIN, (scale, eta, margins)


def _device_solve(g2o_amd_mod, prob, lam, eta):
    opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    opt.set_algorithm("lm_pcg6_3_eigen")
    opt.set_eta(eta)
    opt.initialize_optimization()
    opt.build_structure()
    opt.build_system()
    opt.set_lambda(lam)
    assert opt.solve()
    return opt


@pytest.mark.gpu
@pytest.mark.parametrize("eta", ETAS)
@pytest.mark.parametrize("scale", LAM_SCALES)
@pytest.mark.parametrize("name", list(EDGE_PROBLEMS))
def test_gpu_cgls_solve_matches_restatement(g2o_amd_mod, oracle, name, scale, eta):
    """One buildSystem / setLambda / solve on the device against the restatement: b (1e-12), max diag(J^T J)
    (computeLambdaInit's input, 1e-12), x (1e-6) and the iteration count (equal; the CPU test above keeps every stop
    test clear of a tie). fixed_points / fixed_last pin the points' edge ranges: while they started at edge 0 and not
    past the fixed points' edges (which sort first), x was off by 4.2 to 4.7 of |x| at 1e-3 max diag (iterations 2 / 1,
    4 / 5, 3 / 4) and by 1.8e-4 at 10 max diag, with b exact."""
    J, b, nc, npt, dmax = _system(oracle, name)
    x, it, _, lam = _solve_ref(oracle, name, scale, eta)
    opt = _device_solve(g2o_amd_mod, _problem(name), lam, eta)
    assert opt.vector_size() == len(b)
    dg = opt.diag_absmax()
    assert abs(dg - dmax) <= BTOL * dmax, (dg, dmax)
    bg, xg, itg = opt.b(), opt.x(), opt.linear_iterations()
    eb, ex = np.linalg.norm(bg - b) / np.linalg.norm(b), np.linalg.norm(xg - x) / np.linalg.norm(x)
    print(f"{name} lambda {scale:g} eta {eta:g}: b {eb:.3e} x {ex:.3e} iterations {itg} / {it}")
    assert eb <= BTOL, eb
    assert ex <= RTOL, (ex, itg, it)
    assert itg == it, (itg, it)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", LAM_SCALES)
@pytest.mark.parametrize("name", DIRECT_PROBLEMS)
def test_gpu_cgls_solve_reaches_direct_solution(g2o_amd_mod, oracle, name, scale):
    """eta 1e-20: the device's x against np.linalg.solve of the damped normal equations, independent of the
    restatement's recurrence. Bound: 10 x the restatement's own distance to that direct solve on the same system,
    measured on the CPU (relative to |x|; test_cgls_restatement_edge_problems prints it):
        fixed_points  lambda 1e-3 max diag  1.112e-11  bound 1.112e-10     10 max diag  1.834e-11  bound 1.834e-10
        info_spd      lambda 1e-3 max diag  9.543e-12  bound 9.543e-11     10 max diag  2.702e-11  bound 2.702e-10
    """
    xd = _direct(oracle, name, scale)
    _, _, _, lam = _solve_ref(oracle, name, scale, 1e-20)
    opt = _device_solve(g2o_amd_mod, _problem(name), lam, 1e-20)
    dist = np.linalg.norm(opt.x() - xd) / np.linalg.norm(xd)
    print(f"{name} lambda {scale:g}: device distance to the direct solve {dist:.3e}, bound {DIRECT_BOUND[name, scale]:.1e}")
    assert opt.linear_iterations() > 0 and dist <= DIRECT_BOUND[name, scale], (dist, DIRECT_BOUND[name, scale])


@pytest.mark.gpu
@pytest.mark.parametrize("eta", [0.1, 1e-3])
def test_gpu_cgls_lm_matches_restatement(g2o_amd_mod, oracle, eta):
    for prob in (_tiny(), synth.ba(num_cameras=20, num_points=400, obs_per_point=6, window=10, seed=9),
                 _problem("fixed_points"), _problem("info_spd")):
        opt = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
        opt.set_algorithm("lm_pcg6_3_eigen")
        opt.set_eta(eta)
        n, st = opt.optimize(5)
        host = oracle.OracleGraph(prob)
        sr = cgls_ref.jacobi_lm(host, prob, 5, eta=eta)
        assert n == len(sr)
        for a, b in zip(st, sr):
            assert a.levenbergIterations == b[1]
            assert abs(a.chi2 - b[0]) <= RTOL * b[0], (a.chi2, b[0])
        xg, xr = opt.minimal_state(), host.minimal_state()
        assert np.linalg.norm(xg - xr) <= RTOL * np.linalg.norm(xr)


@pytest.mark.gpu
def test_gpu_cgls_c4_small_reaches_cholesky_chi2(g2o_amd_mod):
    """On C4-small the inexact CGLS steps (eta 0.1) still converge to the Cholesky path's chi2 within 1 %."""
    prob = synth.by_name("C4", "small")
    a = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    a.set_algorithm("lm_pcg6_3_eigen")
    n, st = a.optimize(10)
    b = g2o_amd_mod.SparseOptimizer(0).add_problem(prob)
    nb, sb = b.optimize(10)
    assert abs(st[-1].chi2 - sb[-1].chi2) <= 1e-2 * sb[-1].chi2 and a.linear_iterations() > 0
