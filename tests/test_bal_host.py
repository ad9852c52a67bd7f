"""tests/bal_ref.py checked on the host (no GPU): its Jacobians against central differences in longdouble, the float64
floors and the generator conditions tests/test_gpu_bal.py leans on, and the BAL text writer against its parser.

Measured here (x86-64, numpy longdouble = 80-bit extended):
  Jacobians, theta in [0.1, 3]   float64 analytic against longdouble central differences (h = 1e-6; 1 and 1e-2 for f, k1
                                 and k2, in which the error is linear): 1.1e-12 of a column's largest entry at worst.
                                 The bound 1e-9 is the differences' own h^2 truncation, 1e-12 times the third
                                 derivatives' scale, with margin
  theta = 0                      the Taylor branch is taken (dP/dw = -[X]x exactly); central differences across it, whose
                                 both arms lie in the theta > 0 branch, agree to 4e-13
  theta = 1e-8                   float64 against bal_ref's own Jacobians in longdouble: 2.7e-8 of a column. That is the
                                 float64 value of 1 - cos(theta) (absolute error eps / 2; here it rounds to 0) times
                                 dv/dw ~ 1 / theta in two terms: 2 eps / theta = 4.4e-8 per unit |X|, the bound. ceres'
                                 Jets hold the same value of 1 - cos(theta), so the reference's autodiff has it too. A
                                 closed form dividing by theta^2 would lose eps / theta^2 = 2.2: every digit
  chi2 floor                     float64 against longdouble, on every staged graph, the outlier graph (after its three
                                 LM iterations the four set-aside edges: 2e-15) and the Huber-robustified pins and 65-edge case: 8e-15 in total,
                                 6e-14 per edge at worst
  x floor of the staged systems  under 1e-11 everywhere (worst 8.5e-12, balschur_1; under 4e-13 beyond the tiny graphs)
                                 but bal1p, one free point under two observations: 3.4e-10 (bal_ref.X_FLOOR: its x is
                                 compared at 64 x that on the GPU, every other x at 1e-9)
  LM                             every trial's rho is at least 0.48; dogleg's rho stay 0.07 away from 0, 0.25 and 0.75
"""
import numpy as np
import pytest

import bal_ref as B
import dogleg_ref
from g2o_amd import synth

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)


def _central(cam, X, h=1e-6):
    """d error / d (camera, point) [2, 12] by central differences in longdouble. The error is linear in f, k1 and k2:
    their differences have no truncation error and take steps of 1 and 1e-2, which keeps the differences' rounding
    (eps_longdouble |e| / h) off their small columns."""
    cam, X = cam.astype(LD), X.astype(LD)
    z = np.zeros((1, 2), LD)
    J = np.zeros((2, 12), LD)
    for k in range(12):
        d = np.zeros(12, LD)
        d[k] = LD({6: 1.0, 7: 1e-2, 8: 1e-2}.get(k, h))
        J[:, k] = (B.error(cam + d[None, :9], X + d[None, 9:], z, LD) - B.error(cam - d[None, :9], X - d[None, 9:], z, LD))[0] / (2 * d[k])
    return J


def _case(theta, seed):
    rng = np.random.default_rng(9600 + seed)
    cam = B._rand_cams(rng, 1, theta)
    return cam, B._points_seen_by(rng, cam[0], 1)


def _both(cam, X, dtype=np.float64):
    Ji, Jj = B.jacobians(cam, X, dtype)
    return np.concatenate([Ji[0], Jj[0]], 1)


def test_type_codes():
    assert (synth.V_CAM_BAL, synth.E_OBSERVATION_BAL) == (B.V_CAM, B.E) == (8, 30)
    assert synth.EST_DIM[synth.V_CAM_BAL] == 9 and synth.MEAS_DIM[B.E] == synth.ERR_DIM[B.E] == 2


@pytest.mark.parametrize("theta", [0.1, 0.4, 1.0, 2.0, 3.0])
def test_jacobians_against_central_differences(theta):
    for seed in range(4):
        cam, X = _case(theta, seed)
        J, Jn = _both(cam, X), _central(cam, X)
        err = float(np.max(np.abs(J - Jn) / np.max(np.abs(Jn), 0)))
        print(f"theta {theta} seed {seed}: {err:.2e}")
        assert err <= 1e-9
        assert np.all(np.max(np.abs(Jn), 0) > 0)  # every parameter moves the pixels, both distortion terms among them


def test_theta_zero_takes_the_taylor_branch():
    cam, X = _case(0.0, 0)
    assert not cam[0, :3].any()
    P, dPw, dPX = B.rotate(cam[:, :3], X, jac=True)
    assert np.array_equal(P, X) and np.array_equal(dPX[0], np.eye(3))
    assert np.array_equal(dPw[0], -B._skew(X)[0])
    J, Jn = _both(cam, X), _central(cam, X)  # both arms of the difference lie in the theta > 0 branch
    err = float(np.max(np.abs(J - Jn) / np.max(np.abs(Jn), 0)))
    print(f"theta 0 against central differences across the branch: {err:.2e}")
    assert err <= 1e-9


def test_small_theta_against_longdouble():
    theta = 1e-8
    for seed in range(4):
        cam, X = _case(theta, seed)
        assert abs(np.linalg.norm(cam[0, :3]) - theta) < 1e-20
        J, JL = _both(cam, X), _both(cam, X, LD)
        scale = np.max(np.abs(JL), 0)
        err = float(np.max(np.abs(J - JL) / scale))
        bound = 2 * EPS / theta * float(np.linalg.norm(X))
        print(f"theta 1e-8 seed {seed}: {err:.2e} (bound {bound:.2e})")
        assert err <= bound
        # everything outside dP/dw is at float64's own precision
        assert float(np.max(np.abs(J - JL)[:, 3:] / scale[3:])) <= 64 * EPS


def test_chi2_floor():
    for prob, robust in B.chi2_cases():
        g = B.Graph(prob)
        c64, cl = g.edge_chi2(), g.edge_chi2(dtype=LD)
        t64, tl = g.chi2_in(np.float64, robust=robust), g.chi2_in(LD, robust=robust)
        tot, edge = float(abs(t64 - tl) / tl), float(np.max(np.abs(c64 - cl) / cl))
        print(f"{prob.name} {robust}: total {tot:.2e} per edge {edge:.2e}")
        assert tot < 1e-13 and edge < 1e-13
        # the per-edge path of unary_ref.Graph, which the GPU tests compare with
        ref = g.chi2(robust={B.E: robust} if robust else None)
        assert abs(ref - t64) <= 1e-13 * t64
        if robust:  # the kernel is at work
            assert t64 < 0.999 * c64.sum()


def test_generators():
    for prob in B.staged_cases():
        cams, pts = (next(v for v in prob.vertices if v.vtype == t) for t in (B.V_CAM, B.V_XYZ))
        (es,) = prob.edges
        c, X = cams.est[np.searchsorted(cams.ids, es.v0)], pts.est[np.searchsorted(pts.ids, es.v1)]
        P = B.rotate(c[:, :3], X) + c[:, 3:6]
        res = np.linalg.norm(B.error(c, X, es.meas), axis=1)
        assert np.all(P[:, 2] < -2.0) and np.all(P[:, 2] > -8.0), prob.name  # in front of a camera that looks down -z
        assert np.all((cams.est[:, 6] > 399) & (cams.est[:, 6] < 601)) and np.all(np.abs(cams.est[:, 7]) <= 0.0501)
        assert np.all(np.abs(cams.est[:, 8]) <= 0.0101)
        assert res.min() > 1.0 and res.max() < 12.0, (prob.name, res.min(), res.max())  # never near zero


def test_x_floor_of_the_staged_systems():
    worst = 0.0
    for prob in B.staged_cases():
        x64, xl = B.solve_in(prob, np.float64), B.solve_in(prob, LD)
        floor = float(np.linalg.norm(x64 - xl) / np.linalg.norm(xl))
        print(f"{prob.name}: n {len(xl)} floor {floor:.2e}")
        if prob.name in B.X_FLOOR:
            assert 1e-11 < floor <= 2 * B.X_FLOOR[prob.name], (prob.name, floor)
        else:
            assert floor <= 1e-11, (prob.name, floor)
            worst = max(worst, floor)
        # the dense solve of unary_ref.solve, which the GPU tests compare with, is the same x
        r = B.numpy_stage(prob)
        assert np.linalg.norm(r["x"] - x64) <= max(64 * floor, 1e-11) * np.linalg.norm(x64), prob.name
    print(f"worst floor outside X_FLOOR {worst:.2e}")


@pytest.mark.parametrize("algo,fixed", B.TRAJECTORIES)
def test_trajectory_margins(algo, fixed):
    prob = B.trajectory_case(fixed)
    d = B.Dense(prob)
    chi0 = float(d.chi2())
    if algo == "lm":
        for robust in (None, B.HUBER):
            out = B.lm(B.Dense(prob, robust=robust), 5)
            rhos = [r for _, _, rh in out for r in rh]
            print(f"lm fixed {fixed} robust {robust}: chi2 {[c for c, _, _ in out]} rho {rhos}")
            assert len(out) == 5 and min(abs(r) for r in rhos) >= 1e-3
            assert out[-1][0] < (0.8 if not robust else 1.0) * chi0
    elif algo == "gn":
        out = B.gn(d, 5)
        print(f"gn fixed {fixed}: {out}")
        assert len(out) == 5 and all(b < a for a, b in zip([chi0] + out, out))
    else:
        n, its = dogleg_ref.optimize(d, 5)
        print(f"dl fixed {fixed}: {[(i.chi2, i.tries, i.rho_margin, i.norm_margin) for i in its]}")
        assert n == 5 and all(i.was_pd and i.rho_margin >= 1e-3 and i.norm_margin >= 1e-3 for i in its)
        assert its[-1].chi2 < 0.8 * chi0


def test_huber_is_at_work():
    prob = B.trajectory_case(())
    c = B.Dense(prob).edge_chi2()
    assert 0.2 < np.mean(c > B.HUBER[1] ** 2) < 0.95  # both branches of the kernel


def test_outlier_case_separates():
    prob, bad = B.outlier_case()
    c = B.Graph(prob).edge_chi2()
    assert bad.sum() == 4 and c[bad].min() > 1000 > 100 > c[~bad].max()
    d = B.Dense(B.without(prob, bad))
    out = B.lm(d, 3)  # the run the GPU test follows once the four are set aside
    assert len(out) == 3 and min(abs(r) for _, _, rh in out for r in rh) >= 1e-3
    # at that state the chi2 of the four set-aside edges is compared at 1e-12 (the device follows the run to 1e-6). The
    # active edges are not: LM has fitted them, their chi2 falls to 0.07 and the float64 floor rises to 1.0e-13
    est = {t: v.astype(np.float64) for t, v in d.est.items()}
    c64, cl = B.Graph(prob).edge_chi2(est), B.Graph(prob).edge_chi2(est, LD)
    floor = np.abs(c64 - cl) / cl
    print(f"per-edge floor after 3 iterations: set aside {float(floor[bad].max()):.2e}, active {float(floor[~bad].max()):.2e}, "
          f"smallest chi2 {c64.min():.3g}")
    assert float(floor[bad].max()) < 1e-13 and c64[bad].min() > 1000


def test_text_round_trip_is_bitwise():
    prob = B.trajectory_case(())
    for sep in ("\n", " ", "\t\r\n  "):
        cams, pts, ci, pi, obs = B.parse_bal(B.bal_text(prob, sep))
        (es,) = prob.edges
        assert np.array_equal(cams, prob.vertices[0].est) and np.array_equal(pts, prob.vertices[1].est)
        assert np.array_equal(ci, es.v0) and np.array_equal(pi + len(cams), es.v1) and np.array_equal(obs, es.meas)
    again = B.problem_of(cams, pts, ci, pi, obs)
    assert B.bal_text(again) == B.bal_text(prob)
