"""CPU checks behind tests/test_gpu_icp.py: the numpy restatement of Edge_V_V_GICP and Edge_XYZ_VSC (tests/icp_ref.py)
against central differences through the vertices' oplus in extended precision, the float64 floor of chi2 under
re-association, gicp_prec / gicp_cov against their formulas, the generators, the twin's whitened records, and the Python
constants and C exports against the header. They check the reference restatement, not the device.

The step sweep of test_jacobians_vs_numeric_step_sweep (h = 1e-2 .. 1e-8, longdouble, the worst entry over the cases):
the difference falls as h^2 (3.3 h^2 for Edge_V_V_GICP, 880 h^2 for Edge_XYZ_VSC, whose entries are of order
fx |pc| / z ~ 1e3) until rounding takes over. The smallest difference observed is FLOOR_GICP = 3.3e-12 (at h = 1e-6;
4.4e-12 at 1e-7) and FLOOR_VSC = 2.1e-10 (at h = 1e-7; 8.6e-10 at 1e-6, 1.4e-9 at 1e-8). The assertions stand at ten
times these floors."""
import os
import re

import numpy as np
import pytest

import icp_ref as I
import pose_edges_ref as R
from g2o_amd import synth
from icp_ref import GICP, VSC

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR_GICP, FLOOR_VSC = 3.3e-12, 2.1e-10
STEPS = (1e-2, 1e-3, 1e-4, 1e-5, 1e-6, 1e-7, 1e-8)


def _unit_pose(x):
    x = np.asarray(x, LD).copy()
    x[3:] /= np.sqrt(np.sum(x[3:] * x[3:]))
    return x


def _se3_plus(x, u):
    Rn, tn, _ = R.oplus_se3quat(R.rot(x[3:], LD, False), x[None, :3], u[None], LD)
    return np.concatenate([tn[0], R.quat(Rn)[0]])


def _add(x, u):
    return x + u


def _numeric(f, xs, plus, dims, h):
    out = []
    for a, (x, op, d) in enumerate(zip(xs, plus, dims)):
        cols = []
        for k in range(d):
            u = np.zeros(d, LD)
            u[k] = h
            hi = f(*[op(x, u) if b == a else y for b, y in enumerate(xs)])
            lo = f(*[op(x, -u) if b == a else y for b, y in enumerate(xs)])
            cols.append((hi - lo) / (2 * LD(h)))
        out.append(np.stack(cols, 1))
    return out


def _gicp_worst(h, seed):
    x0, x1, meas, _, _ = I.gicp_case(3, seed=seed)
    worst = 0.0
    for k in range(len(meas)):
        a, b, m = _unit_pose(x0[k]), _unit_pose(x1[k]), meas[k:k + 1]
        _, Ji, Jj = I.gicp_edge(a[None], b[None], m, LD)
        Ni, Nj = _numeric(lambda u, v: I.gicp_edge(u[None], v[None], m, LD, jac=False)[0], (a, b), (_se3_plus,) * 2, (6, 6), h)
        worst = max(worst, float(np.abs(Ji[0] - Ni).max()), float(np.abs(Jj[0] - Nj).max()))
    return worst


def _vsc_worst(h, seed):
    pt, x, meas, K, _ = I.vsc_case(3, seed=seed)
    worst = 0.0
    for k in range(len(meas)):
        p, c, m, kk = np.asarray(pt[k], LD), _unit_pose(x[k]), meas[k:k + 1], K[k:k + 1]
        _, Ji, Jj = I.vsc_edge(p[None], c[None], m, kk, LD)
        Ni, Nj = _numeric(lambda u, v: I.vsc_edge(u[None], v[None], m, kk, LD, jac=False)[0], (p, c), (_add, _se3_plus), (3, 6), h)
        worst = max(worst, float(np.abs(Ji[0] - Ni).max()), float(np.abs(Jj[0] - Nj).max()))
    return worst


def test_jacobians_vs_numeric_step_sweep():
    """Both types: the analytic Jacobians against central differences at every step of the sweep; the best step's
    difference within ten times the floor the docstring records."""
    for name, fn, floor in (("Edge_V_V_GICP", _gicp_worst, FLOOR_GICP), ("Edge_XYZ_VSC", _vsc_worst, FLOOR_VSC)):
        sweep = [max(fn(h, s) for s in range(3)) for h in STEPS]
        for h, w in zip(STEPS, sweep):
            print(f"{name} h={h:.0e}: {w:.2e}")
        best = min(sweep)
        print(f"{name}: smallest difference {best:.2e} at h={STEPS[int(np.argmin(sweep))]:.0e}")
        assert best <= 10 * floor, (name, best)


def test_reference_jacobian_columns():
    """The reference's constant matrices: [dRidx p, dRidy p, dRidz p] = 2 [p]x and their transposes' = -2 [p]x
    (types_icp.cpp:49-57), which is what icp_ref's Ji / Jj are written with."""
    dRidx = np.array([[0.0, 0, 0], [0, 0, 2], [0, -2, 0]])
    dRidy = np.array([[0.0, 0, -2], [0, 0, 0], [2, 0, 0]])
    dRidz = np.array([[0.0, 2, 0], [-2, 0, 0], [0, 0, 0]])
    p = np.array([0.3, -1.2, 2.5])
    cols = np.stack([dRidx @ p, dRidy @ p, dRidz @ p], 1)
    assert np.array_equal(cols, 2 * R.skew(p[None])[0])
    colsT = np.stack([dRidx.T @ p, dRidy.T @ p, dRidz.T @ p], 1)
    assert np.array_equal(colsT, -2 * R.skew(p[None])[0])
    x0, x1, meas, _, _ = I.gicp_case(1)
    _, Ji, Jj = I.gicp_edge(x0, x1, meas)
    R0, R1 = R.rot(x0[:, 3:], normalize=False)[0], R.rot(x1[:, 3:], normalize=False)[0]
    p1 = meas[0, 6:9]
    p1t = R0.T @ (R1 @ p1 + x1[0, :3] - x0[0, :3])
    assert np.allclose(Ji[0, :, 3:], np.stack([dRidx @ p1t, dRidy @ p1t, dRidz @ p1t], 1), rtol=0, atol=1e-14)
    R01 = R0.T @ R1
    assert np.allclose(Jj[0, :, 3:], np.stack([R01 @ dRidx.T @ p1, R01 @ dRidy.T @ p1, R01 @ dRidz.T @ p1], 1), rtol=0, atol=1e-14)
    assert np.allclose(Jj[0, :, :3], R01, rtol=0, atol=1e-15) and np.array_equal(Ji[0, :, :3], -np.eye(3))


def chi2_cases():
    """Every kind of problem whose chi2 the GPU tests compare with icp_ref at the project's 1e-12."""
    out = [("gicp one edge", I.one_edge(GICP)), ("gicp one edge pl_pl", I.one_edge(GICP, True)),
           ("vsc one edge", I.one_edge(VSC))]
    for n in (1, 63, 64, 65, 129):
        out.append((f"gicp_pair {n}", synth.gicp_pair(n)))
    out.append(("gicp_pair 4097", synth.gicp_pair(4097)))
    out.append(("gicp_pair 129 pl_pl", synth.gicp_pair(129, pl_pl=True)))
    out.append(("gicp_scans", synth.gicp_scans(6, 2, (1, 64, 200), fixed=(0, 1))))
    out.append(("gicp_scans pl_pl", synth.gicp_scans(6, 2, (1, 64, 200), pl_pl=True)))
    out.append(("gicp_sba", synth.gicp_sba()))
    return out


def test_chi2_float64_floor_under_reassociation():
    """chi2 in float64 under the three associations of the GICP error (the reference's T0^-1 (T1 p), (T0^-1 T1) p and
    R0^T ((R1 p + t1) - t0)) and against longdouble: the floor stays under 1e-13, so the GPU tests compare at 1e-12."""
    worst = 0.0
    for name, prob in chi2_cases():
        g = I.Graph(prob)
        c80 = LD(0)
        c64 = [0.0, 0.0, 0.0]
        for es in prob.edges:
            if es.etype == GICP:
                xi, xj = g._rows(None, es.v0), g._rows(None, es.v1)
                e = I.gicp_edge(xi, xj, es.meas, LD, False)
                c80 += np.sum(np.einsum("ni,nij,nj->n", e, I.gicp_omega(xi, xj, es.info, es.params, LD), e))
                Om = I.gicp_omega(xi, xj, es.info, es.params)
                for a in range(3):
                    e = I.gicp_edge(xi, xj, es.meas, jac=False, assoc=a)
                    c64[a] += float(np.sum(np.einsum("ni,nij,nj->n", e, Om, e)))
            elif es.etype == VSC:
                e, _, _, Om = g.terms(es, dtype=LD, jac=False)
                c80 += np.sum(np.einsum("ni,nij,nj->n", e, Om, e))
                e, _, _, Om = g.terms(es, jac=False)
                for a in range(3):
                    c64[a] += float(np.sum(np.einsum("ni,nij,nj->n", e, Om, e)))
        rel = max(float(abs(LD(c) - c80) / c80) for c in c64)
        print(f"{name}: chi2 {float(c80):.6g} float64 floor {rel:.2e}")
        worst = max(worst, rel)
    print(f"worst float64 floor {worst:.2e}")
    assert worst <= 1e-13, worst


def test_edge_chi2_float64_floor():
    """Per edge, on the graphs whose g2ohip_edge_chi2 the GPU test compares at 1e-12 (the ring with a position noise of
    0.3 and the VSC edges of gicp_sba). With the demo's noise of 0.01 the smallest errors are 1e-3 of the points'
    coordinates and the floor is 3.2e-13: that scene serves the summed chi2 only."""
    for et, prob in ((GICP, synth.gicp_scans(6, 2, (1, 64, 200), fixed=(0, 1), euc_noise=0.3)),
                     (VSC, synth.gicp_sba(200, 100, 3))):
        g = I.Graph(prob)
        c64, c80 = g.edge_chi2(et), g.edge_chi2(et, dtype=LD)
        rel = float(np.max(np.abs(c64.astype(LD) - c80) / c80))
        print(f"type {et}: per-edge chi2 floor {rel:.2e}, smallest chi2 {float(np.min(c80)):.3g}")
        assert rel <= 1e-13, rel


def test_gicp_prec_cov_formulas():
    import g2o_amd
    rng = np.random.default_rng(5)
    for _ in range(20):
        n = rng.standard_normal(3)
        n /= np.linalg.norm(n)
        y = np.array([0, 1.0, 0]) - n[1] * n
        y /= np.linalg.norm(y)
        R0 = np.stack([np.cross(n, y), y, n])  # makeRot0 (types_icp.h:84-96)
        assert np.allclose(R0 @ R0.T, np.eye(3), atol=1e-14)
        P, Cv = g2o_amd.gicp_prec(n, 0.01), g2o_amd.gicp_cov(n, 0.01)
        assert np.allclose(P, R0.T @ np.diag([0.01, 0.01, 1.0]) @ R0, rtol=0, atol=1e-15)
        assert np.allclose(Cv, R0.T @ np.diag([1.0, 1.0, 0.01]) @ R0, rtol=0, atol=1e-15)
        # the plane's normal is the stiff direction of the precision and the thin one of the covariance
        assert abs(n @ P @ n - 1.0) < 1e-14 and abs(n @ Cv @ n - 0.01) < 1e-14
        assert np.allclose(P @ Cv, 0.01 * np.eye(3), atol=1e-15)
        assert np.allclose(I.unpack(g2o_amd.gicp_pack(Cv))[0], Cv, rtol=0, atol=1e-16)  # packed upper and back
    for bad in ([0, 1.0, 0], [0, -1.0, 0]):
        with pytest.raises(ValueError):
            g2o_amd.gicp_prec(bad)
        with pytest.raises(ValueError):
            g2o_amd.gicp_cov(bad)


def test_whitened_twin_records():
    """The plane-to-plane twin: identity information and [L^T e | L^T Ji | L^T Jj] give the set's quadratic form."""
    prob = synth.gicp_scans(4, 1, 7, pl_pl=True)
    tw = synth.icp_twin(prob)
    assert tw.edges[0].etype == I.HOSTJ3 and tw.edges[0].meas is None and tw.edges[0].params is None
    assert np.array_equal(tw.edges[0].info, np.broadcast_to(np.eye(3), (len(prob.edges[0].v0), 3, 3)))
    g = I.Graph(prob)
    e, Ji, Jj, Om = g.terms(prob.edges[0])
    rec = g.payload().reshape(len(e), 39)
    we, wi, wj = rec[:, :3], rec[:, 3:21].reshape(-1, 3, 6), rec[:, 21:].reshape(-1, 3, 6)
    assert np.allclose(np.einsum("ni,ni->n", we, we), np.einsum("ni,nij,nj->n", e, Om, e), rtol=1e-13)
    assert np.allclose(np.einsum("nia,nib->nab", wi, wj), np.einsum("nia,nij,njb->nab", Ji, Om, Jj), rtol=1e-12, atol=1e-12)
    assert np.allclose(np.einsum("nia,ni->na", wi, we), np.einsum("nia,nij,nj->na", Ji, Om, e), rtol=1e-12, atol=1e-12)
    # Omega follows the state: another R01 gives another information
    est = {synth.V_SE3_QUAT: prob.vertices[0].est.copy()}
    q = est[synth.V_SE3_QUAT][1, 3:] + np.array([0.2, -0.1, 0.05, 0.0])
    est[synth.V_SE3_QUAT][1, 3:] = q / np.linalg.norm(q)
    assert not np.allclose(g.terms(prob.edges[0], est)[3], Om)


def test_synth_generators():
    a, b = synth.gicp_pair(65), synth.gicp_pair(65)
    assert np.array_equal(a.edges[0].meas, b.edges[0].meas) and np.array_equal(a.edges[0].info, b.edges[0].info)
    es = a.edges[0]
    assert es.etype == GICP and es.meas.shape == (65, 12) and es.info.shape == (65, 3, 3) and es.params is None
    assert list(a.vertices[0].fixed) == [1, 0] and abs(a.vertices[0].est[1, 2] - 0.2) < 1e-15
    assert np.allclose(np.linalg.norm(es.meas[:, 3:6], axis=1), 1.0) and np.array_equal(es.meas[:, 3:6], es.meas[:, 9:12])
    pl = synth.gicp_pair(65, pl_pl=True).edges[0]
    assert pl.info is None and pl.params.shape == (65, 12)
    sc = synth.gicp_scans(6, 2, (1, 64, 200), fixed=(0, 1))
    es = sc.edges[0]
    pairs = {}
    for u, v in zip(es.v0, es.v1):
        pairs.setdefault((min(u, v), max(u, v)), set()).add((int(u), int(v)))
    counts = sorted({int(np.sum((np.minimum(es.v0, es.v1) == p[0]) & (np.maximum(es.v0, es.v1) == p[1]))) for p in pairs})
    assert len(pairs) == 12 and counts == [1, 64, 200], (len(pairs), counts)
    assert any(len(o) == 2 for o in pairs.values())  # a pair entered both ways round
    assert (0, 1) in pairs and list(sc.vertices[0].fixed[:2]) == [1, 1]  # one pair with both ends fixed
    chi = I.Graph(sc).chi2()
    assert 0 < chi < 100.0 * len(es.v0)
    sb = synth.gicp_sba()
    assert [e.etype for e in sb.edges] == [GICP, VSC] and sb.landmark_dim == 3
    assert np.all(sb.vertices[1].marginalized == 1) and sb.edges[1].params.shape[1] == 5
    assert len(np.unique(sb.edges[1].params, axis=0)) == 1
    tw = synth.icp_twin(sb)
    assert [e.etype for e in tw.edges] == [I.HOSTJ3, I.HOSTJ3]


def test_python_constants_and_exports_equal_the_header():
    import g2o_amd
    text = open(os.path.join(ROOT, "include", "g2o_hip.h")).read()

    def define(name):
        return int(re.search(rf"#define {name} (\d+)u?\b", text).group(1))

    assert g2o_amd.E_V_V_GICP == synth.E_V_V_GICP == define("G2OHIP_E_V_V_GICP") == 25
    assert g2o_amd.E_XYZ_VSC == synth.E_XYZ_VSC == define("G2OHIP_E_XYZ_VSC") == 26
    assert g2o_amd.LOAD_ICP == define("G2OHIP_LOAD_ICP") == 64
    assert g2o_amd.ICP_EDGE_TAGS == {GICP: "EDGE_V_V_GICP"}
    assert synth.ERR_DIM[GICP] == synth.ERR_DIM[VSC] == 3 and synth.MEAS_DIM[GICP] == 12 and synth.MEAS_DIM[VSC] == 3
    assert synth.PARAM_DIM[GICP] == 12 and synth.PARAM_DIM[VSC] == 5
    for name in ("g2ohip_set_pair_major", "g2ohip_pair_major_info"):
        assert name in g2o_amd.EXPORTS and re.search(rf"\bint {name}\(g2ohip_graph\* g", text), name
    capi = open(os.path.join(ROOT, "g2o_amd", "csrc", "capi.cpp")).read()
    for name in ("g2ohip_set_pair_major", "g2ohip_pair_major_info"):
        assert re.search(rf"^int {name}\(", capi, re.M), name
