"""tests/pose_edges_ref.py proved on the CPU before the GPU tests trust it.

* Its closed-form Jacobians, in longdouble, against central differences (step 1e-6) of its longdouble error under the
  vertex's own oplus: 1e-9 on every generated case (the strategy and the figures of tests/test_oracle_pins.py, at
  extended precision).
* Its float64 path against its longdouble path. Measured floors (x86-64 extended precision, eps 1.1e-19), the largest
  over all generated cases of max |float64 - longdouble| / max |longdouble|:
      EdgeSE3         e 3.4e-16   Ji 5.6e-16   Jj 7.0e-16
      EdgeSE3Prior    e 6.7e-16   J  5.6e-16
      EdgeSE2         e 1.6e-16   Ji 9.6e-17   Jj 8.5e-17
      EdgeSE2PointXY  e 7.6e-17   Ji 7.2e-17   Jj 4.9e-17
  and the largest absolute deviation of each oplus map over pose_edges_ref.oplus_cases, relative to max(1, |value|):
      V_SE3_EXPMAP 4.6e-13   V_XYZ 2.8e-17   V_SE3_QUAT 1.8e-16 (rotation matrix and translation)   V_SE2 9.5e-17
      V_XY 4.9e-17
  The edge floors are far below a tenth of the single-edge tolerances 1e-9 / 1e-11 of tests/test_gpu_pose_edges.py: no
  case had to be moved. The oplus floors are pose_edges_ref.OPLUS_FLOOR, which tests/test_gpu_oplus.py multiplies by 8;
  all but one are below 64 eps = 1.4e-14, the floor of that tolerance. The exception is the expmap's theta = 2e-5 case:
  just above its series threshold SE3Quat::exp forms (1 - cos theta) / theta^2, where half an ulp of cos (5.5e-17 out
  of 2e-10) moves V by eps / (2 theta^2) and the translation V upsilon by eps |upsilon| / (2 theta) = 5.5e-12 |upsilon|.
  That is the reference's own formula, so it is the rule here too; test_float64_floor_oplus bounds the floor by it.
  The other expmap cases deviate by 6e-16 at most.
* The CPU oracle (the restatement the rest of the suite trusts) against the reference on every single-edge problem of the
  binary types: b, x and Hschur at lambda = 1e-3. The oracle restates no unary edge; the SE3 prior is tied to
  unary_ref's float64 forms instead, which tests/test_unary_host.py pins.
* The branch census: all seven rotation labels, both wrap directions, and the label each case was built for.
"""
import numpy as np
import pytest

import pose_edges_ref as R
import unary_ref
from g2o_amd import synth
from pose_edges_ref import LD

EPS = float(np.finfo(np.float64).eps)
FLOOR_MAX = 64 * EPS
H, JTOL = LD(1e-6), 1e-9


def _unit_pose(x):
    """The pose in longdouble with its quaternion of norm 1 to 1e-19: the differences below then see no change of norm."""
    x = np.asarray(x, LD).copy()
    x[3:] /= np.sqrt(np.sum(x[3:] * x[3:]))
    return x


def _se3_plus(x, u):
    Rn, tn, _ = R.oplus_se3quat(R.rot(x[3:], LD, False), x[None, :3], u[None], LD)
    return np.concatenate([tn[0], R.quat(Rn)[0]])


def _se2_plus(x, u):
    return R.oplus_se2(x, u, LD)[0]


def _add(x, u):
    return x + u


def _numeric(f, xs, plus, dims):
    """Central differences of f(*xs) under each argument's oplus: one Jacobian [D, dim] per argument."""
    out = []
    for a, (x, op, d) in enumerate(zip(xs, plus, dims)):
        cols = []
        for k in range(d):
            u = np.zeros(d, LD)
            u[k] = H
            hi = f(*[op(x, u) if b == a else y for b, y in enumerate(xs)])
            lo = f(*[op(x, -u) if b == a else y for b, y in enumerate(xs)])
            cols.append((hi - lo) / (2 * H))
        out.append(np.stack(cols, 1))
    return out


def _worst(pairs):
    return max(float(np.abs(a - b).max()) for a, b in pairs)


def test_se3_jacobians_vs_numeric():
    for label, xi, xj, z in R.se3_branch_cases():
        xi, xj = _unit_pose(xi), _unit_pose(xj)
        _, Ji, Jj = R.se3_edge(xi, xj, z, LD)
        Ni, Nj = _numeric(lambda a, b: R.se3_edge(a, b, z, LD, jac=False)[0], (xi, xj), (_se3_plus,) * 2, (6, 6))
        w = _worst([(Ji[0], Ni), (Jj[0], Nj)])
        print(f"EdgeSE3 {label}: {w:.2e}")
        assert w <= JTOL, (label, w)


def test_prior_jacobians_vs_numeric():
    for label, x, z, P in R.prior_branch_cases():
        x = _unit_pose(x)
        _, J = R.se3_prior(x, z, P, LD)
        N, = _numeric(lambda a: R.se3_prior(a, z, P, LD, jac=False)[0], (x,), (_se3_plus,), (6,))
        w = _worst([(J[0], N)])
        print(f"EdgeSE3Prior {label}: {w:.2e}")
        assert w <= JTOL, (label, w)


def test_se2_jacobians_vs_numeric():
    for label, xi, xj, z in R.se2_wrap_cases():
        xi, xj = np.asarray(xi, LD), np.asarray(xj, LD)
        _, Ji, Jj = R.se2_edge(xi, xj, z, LD)
        Ni, Nj = _numeric(lambda a, b: R.se2_edge(a, b, z, LD, jac=False)[0], (xi, xj), (_se2_plus,) * 2, (3, 3))
        w = _worst([(Ji[0], Ni), (Jj[0], Nj)])
        print(f"EdgeSE2 {label}: {w:.2e}")
        assert w <= JTOL, (label, w)


def test_se2xy_jacobians_vs_numeric():
    for label, xi, l, z in R.se2xy_wrap_cases():
        xi, l = np.asarray(xi, LD), np.asarray(l, LD)
        _, Ji, Jj = R.se2xy_edge(xi, l, z, LD)
        Ni, Nj = _numeric(lambda a, b: R.se2xy_edge(a, b, z, LD, jac=False)[0], (xi, l), (_se2_plus, _add), (3, 2))
        w = _worst([(Ji[0], Ni), (Jj[0], Nj)])
        print(f"EdgeSE2PointXY {label}: {w:.2e}")
        assert w <= JTOL, (label, w)


def _rel(a, b):
    return float(np.abs(np.asarray(a, LD) - b).max() / np.abs(b).max())


def test_float64_floor_edges():
    """The figures of the module text."""
    fl = {}

    def note(name, parts64, partsld):
        for k, (a, b) in enumerate(zip(parts64, partsld)):
            fl[name, k] = max(fl.get((name, k), 0.0), _rel(a[0], b[0]))

    for _, xi, xj, z in R.se3_branch_cases():
        note("EdgeSE3", R.se3_edge(xi, xj, z), R.se3_edge(xi, xj, z, LD))
    for _, x, z, P in R.prior_branch_cases():
        note("EdgeSE3Prior", R.se3_prior(x, z, P), R.se3_prior(x, z, P, LD))
    for _, xi, xj, z in R.se2_wrap_cases():
        note("EdgeSE2", R.se2_edge(xi, xj, z), R.se2_edge(xi, xj, z, LD))
    for _, xi, l, z in R.se2xy_wrap_cases():
        note("EdgeSE2PointXY", R.se2xy_edge(xi, l, z), R.se2xy_edge(xi, l, z, LD))
    for k, v in sorted(fl.items()):
        print(f"floor {k[0]} part {k[1]}: {v:.1e}")
    assert max(fl.values()) <= FLOOR_MAX, fl


def oplus_floor(vtype):
    """max |float64 - longdouble| / max(1, |longdouble|) of one oplus map over its cases (SE3_QUAT: R and t)."""
    _, est, u = R.oplus_cases(vtype)
    if vtype == synth.V_SE3_QUAT:
        a = R.oplus_se3quat(R.rot(est[:, 3:], np.float64, False), est[:, :3], u)[:2]
        b = R.oplus_se3quat(R.rot(est[:, 3:], LD, False), est[:, :3], u, LD)[:2]
        return max(float((np.abs(x - y) / np.maximum(1, np.abs(y))).max()) for x, y in zip(a, b))
    a, b = R.oplus(vtype, est, u), R.oplus(vtype, est, u, LD)
    return float((np.abs(a - b) / np.maximum(1, np.abs(b))).max())


def test_float64_floor_oplus():
    """The floors written down (pose_edges_ref.OPLUS_FLOOR, the figures of the module text) are a record of one
    machine: another numpy build may round cos or order a sum differently. What must hold everywhere is the reasoning:
    every map is a handful of rounded operations on values of order one, so its floor is below 64 eps; the expmap's is
    bounded by the module text's eps |upsilon| / (2 theta) per half ulp of cos, taken here for a cos good to 4 ulp."""
    for vt in (synth.V_SE3_EXPMAP, synth.V_XYZ, synth.V_SE3_QUAT, synth.V_SE2, synth.V_XY):
        f = oplus_floor(vt)
        print(f"oplus floor vertex type {vt}: measured {f:.1e}, written down {R.OPLUS_FLOOR[vt]:.1e}")
        bound = 8 * EPS * np.sqrt(3) / (2 * 2e-5) if vt == synth.V_SE3_EXPMAP else FLOOR_MAX
        assert f <= bound and R.OPLUS_FLOOR[vt] <= bound, (vt, f, bound)


def test_oplus_rules():
    """The rules that are not maths: identity above |dq|^2 = 1, the series below theta = 1e-5, the wrap's interval."""
    _, est, u = R.oplus_cases(synth.V_SE3_QUAT)
    R0 = R.rot(est[:, 3:], np.float64, False)
    R1, t1, _ = R.oplus_se3quat(R0, est[:, :3], u)
    big = np.sum(u[:, 3:] ** 2, 1) > 1
    assert big.sum() == 2 and np.array_equal(R1[big], R0[big]) and not np.array_equal(t1[big], est[big, :3])
    assert all(not np.array_equal(a, b) for a, b in zip(R1[~big][1:], R0[~big][1:]))
    Rs, _ = R.se3_exp(np.array([[3e-6, 4e-6, 0, 0, 0, 0]]))  # theta = 5e-6: I + W + W^2 / 2, not Rodrigues
    assert Rs[0, 1, 2] == -3e-6 and abs(Rs[0, 0, 1] - 6e-12) <= 1e-26  # Rodrigues: -3e-6 (1 - theta^2 / 6)
    w = R.wrap(np.array([-R.PI, R.PI, 3 * R.PI, -3 * R.PI, 7.0]))
    assert w[0] == -R.PI and w[1] == -R.PI and np.all((w >= -R.PI) & (w < R.PI)) and abs(w[4] - (7 - 2 * R.PI)) < 1e-15
    # 1001 calls: the counter triggers one re-orthogonalisation and restarts
    Rk, tk, calls = R.rot([[0.1, 0.2, 0.3, 0.93]], np.float64, False), np.zeros((1, 3)), 0  # not a unit quaternion
    drift0 = np.abs(Rk[0].T @ Rk[0] - np.eye(3)).max()
    for k in range(1001):
        Rk, tk, calls = R.oplus_se3quat(Rk, tk, np.array([[0, 0, 0, 1e-4, 0, 0]]), calls=calls)
        if k == 999:
            assert calls == 1000 and np.abs(Rk[0].T @ Rk[0] - np.eye(3)).max() > 0.5 * drift0
    assert calls == 0 and np.abs(Rk[0].T @ Rk[0] - np.eye(3)).max() < 2 * drift0 ** 2


def test_unary_ref_oplus_follows_the_reference_above_one():
    """unary_ref.oplus for V_SE3_QUAT: the identity rotation when |dq|^2 > 1, and equal to this reference everywhere."""
    _, est, u = R.oplus_cases(synth.V_SE3_QUAT)
    for k in range(len(est)):
        a = unary_ref.oplus(synth.V_SE3_QUAT, est[k], u[k])
        b = R.oplus(synth.V_SE3_QUAT, est[k], u[k])[0]
        assert np.abs(a - b).max() <= 1e-14, (k, a, b)
        if u[k, 3:] @ u[k, 3:] > 1:
            assert np.abs(unary_ref._R(a[3:]) - unary_ref._R(est[k, 3:])).max() <= 4 * EPS


def test_prior_against_unary_ref():
    for label, x, z, P in R.prior_branch_cases():
        e, J = R.se3_prior(x, z, P)
        e0 = unary_ref.prior_error(synth.E_SE3_PRIOR, x, z, P)
        J0 = unary_ref.prior_jacobian(synth.E_SE3_PRIOR, x, z, P)
        assert np.abs(e[0] - e0).max() <= 1e-14 and np.abs(J[0] - J0).max() <= 1e-14, label


def _oracle_against(oracle, prob, tag):
    lam = 1e-3
    s = oracle.OracleGraph(prob).stage(lam)
    r = R.numpy_stage(prob, lam)
    assert s["ok"] == 1 and (s["n"], s["np"]) == (r["n"], r["np"])
    for k, tol in (("b", 1e-9), ("x", 1e-9), ("Hschur", 1e-11)):
        err = np.linalg.norm(s[k] - r[k]) / np.linalg.norm(r[k])
        print(f"oracle {tag} {k}: {err:.2e}")
        assert err <= tol, (tag, k, err)


def test_oracle_single_edges(oracle):
    for k, c in enumerate(R.se3_branch_cases()):
        _oracle_against(oracle, R.se3_problem(c, k), f"EdgeSE3 {c[0]}")
    for k, c in enumerate(R.se2_wrap_cases()):
        _oracle_against(oracle, R.se2_problem(c, k), f"EdgeSE2 {c[0]}")
    for k, c in enumerate(R.se2xy_wrap_cases()):
        _oracle_against(oracle, R.se2xy_problem(c, k), f"EdgeSE2PointXY {c[0]}")


@pytest.mark.parametrize("ne", [1, 63, 64, 65, 257])
def test_oracle_chains(oracle, ne):
    """The graphs of the GPU stage tests: the conditioning their tolerances rely on, shown on the CPU."""
    _oracle_against(oracle, R.se3_chain(ne)[0], f"se3 chain {ne}")
    _oracle_against(oracle, R.se2_chain(ne)[0], f"se2 chain {ne}")
    _oracle_against(oracle, R.se2xy_fan(ne), f"se2xy fan {ne}")


def error_rotation(e):
    return R.rot(np.concatenate([e[3:], [np.sqrt(1 - e[3:] @ e[3:])]]), LD)[0]


def test_branch_census():
    se3 = R.se3_branch_cases()
    pri = R.prior_branch_cases()
    for cases, err in ((se3, lambda c: R.se3_edge(c[1], c[2], c[3], LD, jac=False)[0]),
                       (pri, lambda c: R.se3_prior(c[1], c[2], c[3], LD, jac=False)[0])):
        assert [c[0] for c in cases] == list(R.LABELS) + ["tr0+", "tr0-", "wneg"]
        got = [R.branch_of(error_rotation(err(c))) for c in cases]
        assert got[:7] == list(R.LABELS) and set(got) == set(R.LABELS), got
        assert got[7] == "tr+" and got[8] != "tr+"  # the pair straddles trace = 0
        tr = [float(np.trace(error_rotation(err(c)))) for c in cases[7:9]]
        assert 0.5e-3 < tr[0] < 2e-3 and -2e-3 < tr[1] < -0.5e-3, tr
        z = cases[9][3] if cases is se3 else cases[9][2]
        assert z[6] < 0 and abs(np.linalg.norm(z[3:]) - 1.3) < 1e-12
    for ne in (63, 257):
        assert set(R.se3_chain(ne)[1]) == set(R.LABELS)
        assert set(R.se2_chain(ne)[1]) == {"up", "down"}
    assert {c[0] for c in R.se2_wrap_cases()} == {"up", "down"}
    assert {c[0] for c in R.se2xy_wrap_cases()} == {"edge", "outside"}
    used = {float(c[1][2]) for c in R.se2_wrap_cases()} | {float(c[2][2]) for c in R.se2_wrap_cases()}
    assert used == set(R.SE2_ANGLES)
