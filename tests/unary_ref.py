"""Plain-numpy restatement of the unary edge types (test reference; nothing here comes from the oracle or the library).

  EdgeSE2Prior      types/slam2d/edge_se2_prior.h:39-77      e = (Z^-1 * x).toVector(),  J = [R(Z^-1) 0; 0 1]
  EdgeSE2XYPrior    types/slam2d/edge_se2_xyprior.h:39-71    e = t(x) - z,               J = [I 0]
  EdgeXYPrior       types/slam2d/edge_xy_prior.h             e = l - z,                  J = I
  EdgeXYZPrior      types/slam3d/edge_xyz_prior.cpp:63-70    e = p - z,                  J = I
  EdgeSE3Prior      types/slam3d/edge_se3_prior.cpp:89-102   e = toVectorMQT(Z^-1 X P),  J from E(d) = (Z^-1 X) exp(d) P

and of what a graph holding them needs: the oplus of the five vertex types, the nine robust kernels
(robust_kernel_impl.cpp), the weighted quadratic form of base_unary_edge.hpp:57-77, the dense normal equations in the
hessian order (free non-marginalized vertices by id, then the free marginalized ones by id; only vertices that have an
edge), the dense Schur complement and the solve at a given lambda.

The SE3 prior's Jacobian is derived here on its own, not copied from isometry3d_gradients.h: with E(d) = A exp(d) B,
A = Z^-1 X, B = P, exp(d) = (t = d[0:3], q = (d[3:6], sqrt(1 - |d[3:6]|^2))),
  dt_e/dt = Ra,  dt_e/dq = -2 Ra [tb]x,  dq_e/dq = (w I + [q_v]x) Rb^T   (q_e = (q_v, w) of Re, w >= 0),
because Ra (2 [e_k]x) Rb = Re [2 Rb^T e_k]x and a right perturbation Re (I + [w]x) moves q_v by (w_q w + q_v x w) / 2.

Binary edges of a graph: EdgeSE2 and EdgeSE2PointXY are restated here too (edge_se2.cpp:77-103,
edge_se2_pointxy.cpp:63-92); the others (EdgeSE3, the BA projections) are taken as host-J style records [e | Ji | Jj]
the caller supplies per edge type (`binary`).
"""
import numpy as np

import stereo_ref
from g2o_amd import synth

V_DIM = {synth.V_SE3_EXPMAP: 6, synth.V_XYZ: 3, synth.V_SE3_QUAT: 6, synth.V_SE2: 3, synth.V_XY: 2}
PRIORS = (synth.E_SE2_PRIOR, synth.E_SE2_XY_PRIOR, synth.E_XY_PRIOR, synth.E_SE3_PRIOR, synth.E_XYZ_PRIOR)
IDENT7 = np.array([0, 0, 0, 0, 0, 0, 1.0])


def _norm_theta(t):
    return np.mod(t + np.pi, 2 * np.pi) - np.pi if not (-np.pi <= t < np.pi) else t


def _skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0.0]])


def _R(q):
    return synth.quat_to_rot(np.asarray(q, np.float64)[None] / np.linalg.norm(q))[0]


def _quat(R):
    return synth.rot_to_quat(R[None])[0]  # normalized, w >= 0


def _rot2(t):
    return np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])


# ---------------------------------------------------------------- SE2 (se2.h)
def se2_inv(a):
    t = _norm_theta(-a[2])
    return np.concatenate([_rot2(t) @ (-a[:2]), [t]])


def se2_mul(a, b):
    return np.concatenate([a[:2] + _rot2(a[2]) @ b[:2], [_norm_theta(a[2] + b[2])]])


# ---------------------------------------------------------------- vertex oplus
def oplus(vtype, est, u):
    est, u = np.asarray(est, np.float64), np.asarray(u, np.float64)
    if vtype in (synth.V_XYZ, synth.V_XY):  # types_sba.h:149-153, vertex_point_xy.h
        return est + u
    if vtype == synth.V_SE2:  # vertex_se2.h:51-58: translation += u[0:2], angle = normalize_theta(angle + u[2])
        return np.array([est[0] + u[0], est[1] + u[1], _norm_theta(est[2] + u[2])])
    if vtype == synth.V_SE3_QUAT:  # vertex_se3.h:105-113: estimate * fromVectorMQT(u)
        R = _R(est[3:7])
        w2 = 1.0 - u[3:6] @ u[3:6]  # fromCompactQuaternion (isometry3d_mappings.cpp:85-92): identity when |dq|^2 > 1
        inc = np.eye(3) if w2 < 0 else _R(np.concatenate([u[3:6], [np.sqrt(w2)]]))
        return np.concatenate([est[:3] + R @ u[:3], _quat(R @ inc)])
    if vtype == synth.V_SE3_EXPMAP:  # types_six_dof_expmap.h:97-100: exp(u) * estimate
        return stereo_ref.oplus_cam(est, u)
    raise KeyError(vtype)


# ---------------------------------------------------------------- the five priors
def prior_error(etype, est, meas, offset=None):
    est, meas = np.asarray(est, np.float64), np.asarray(meas, np.float64)
    if etype == synth.E_SE2_PRIOR:
        return se2_mul(se2_inv(meas), est)
    if etype == synth.E_SE2_XY_PRIOR:
        return est[:2] - meas
    if etype in (synth.E_XY_PRIOR, synth.E_XYZ_PRIOR):
        return est - meas
    if etype == synth.E_SE3_PRIOR:
        P = IDENT7 if offset is None else np.asarray(offset, np.float64)
        Rz, Rx, Rp = _R(meas[3:7]), _R(est[3:7]), _R(P[3:7])
        Re = Rz.T @ Rx @ Rp
        te = Rz.T @ (Rx @ P[:3] + est[:3] - meas[:3])
        return np.concatenate([te, _quat(Re)[:3]])
    raise KeyError(etype)


def prior_jacobian(etype, est, meas, offset=None):
    est, meas = np.asarray(est, np.float64), np.asarray(meas, np.float64)
    if etype == synth.E_SE2_PRIOR:
        J = np.zeros((3, 3))
        J[:2, :2] = _rot2(se2_inv(meas)[2])
        J[2, 2] = 1.0
        return J
    if etype == synth.E_SE2_XY_PRIOR:
        return np.array([[1.0, 0, 0], [0, 1.0, 0]])
    if etype == synth.E_XY_PRIOR:
        return np.eye(2)
    if etype == synth.E_XYZ_PRIOR:
        return np.eye(3)
    if etype == synth.E_SE3_PRIOR:
        P = IDENT7 if offset is None else np.asarray(offset, np.float64)
        Ra, Rb = _R(meas[3:7]).T @ _R(est[3:7]), _R(P[3:7])
        q = _quat(Ra @ Rb)
        J = np.zeros((6, 6))
        J[:3, :3] = Ra
        J[:3, 3:] = -2.0 * Ra @ _skew(P[:3])
        J[3:, 3:] = (q[3] * np.eye(3) + _skew(q[:3])) @ Rb.T
        return J
    raise KeyError(etype)


# ---------------------------------------------------------------- robust kernels (robust_kernel_impl.cpp:65-200)
def robustify(kind, delta, e2):
    """(rho, rho') of one squared error under RobustKernel<kind> with setDelta(delta)."""
    d2 = delta * delta
    if kind in (None, "none"):
        return e2, 1.0
    if kind == "Huber":
        return (e2, 1.0) if e2 <= d2 else (2 * np.sqrt(e2) * delta - d2, delta / np.sqrt(e2))
    if kind == "PseudoHuber":
        a = np.sqrt(e2 / d2 + 1.0)
        return 2 * d2 * (a - 1), 1.0 / a
    if kind == "Cauchy":
        a = e2 / d2 + 1.0
        return d2 * np.log(a), 1.0 / a
    if kind == "GemanMcClure":
        a = delta / (delta + e2)
        return e2 * a, a * a
    if kind == "Welsch":
        a = np.exp(-e2 / d2)
        return d2 * (1 - a), a
    if kind == "Fair":
        a = np.sqrt(e2) / delta
        return 2 * d2 * (a - np.log1p(a)), 1.0 / (1 + a)
    if kind == "Tukey":
        if np.sqrt(e2) <= delta:
            a = 1 - e2 / d2
            return d2 * (1 - a ** 3) / 3, a * a
        return d2 / 3, 0.0
    if kind == "Saturated":
        return (e2, 1.0) if e2 <= d2 else (d2, 0.0)
    if kind == "DCS":
        s = min(1.0, 2 * delta / (delta + e2))
        return s * e2 * s, s * s
    raise KeyError(kind)


# ---------------------------------------------------------------- binary edges restated here
def se2_edge(xi, xj, z):
    """EdgeSE2: (e, Ji, Jj) (edge_se2.h:46-52, edge_se2.cpp:77-103)."""
    zi = se2_inv(z)
    e = se2_mul(zi, se2_mul(se2_inv(xi), xj))
    c, s = np.cos(xi[2]), np.sin(xi[2])
    dx, dy = xj[0] - xi[0], xj[1] - xi[1]
    A = np.array([[-c, -s, -s * dx + c * dy], [s, -c, -c * dx - s * dy], [0, 0, -1.0]])
    B = np.array([[c, s, 0], [-s, c, 0], [0, 0, 1.0]])
    Z = np.eye(3)
    Z[:2, :2] = _rot2(zi[2])
    return e, Z @ A, Z @ B


def se2_xy_edge(xi, l, z):
    """EdgeSE2PointXY: (e, Ji, Jj) (edge_se2_pointxy.h:44-49, edge_se2_pointxy.cpp:63-92)."""
    c, s = np.cos(xi[2]), np.sin(xi[2])
    d = l - xi[:2]
    e = np.array([c * d[0] + s * d[1], -s * d[0] + c * d[1]]) - z
    Ji = np.array([[-c, -s, -s * d[0] + c * d[1]], [s, -c, -c * d[0] - s * d[1]]])
    Jj = np.array([[c, s], [-s, c]])
    return e, Ji, Jj


# ---------------------------------------------------------------- graphs
class Graph:
    """A synth.Problem with priors. est: {vertex type: estimates}, the problem's own unless given. robust: {edge
    type: (kind, delta)}. binary: {edge type: records [n, D + D*di + D*dj]} for the binary types not restated here."""

    def __init__(self, prob):
        self.prob = prob
        self.row = {}  # vertex id -> (vertex set, row)
        for vs in prob.vertices:
            for k, i in enumerate(vs.ids):
                self.row[int(i)] = (vs, k)
        has = set()
        for es in prob.edges:
            has.update(int(i) for i in es.v0)
            if es.v1 is not None:
                has.update(int(i) for i in es.v1)
        free = [(int(vs.marginalized[k]), i) for i, (vs, k) in self.row.items() if i in has and not vs.fixed[k]]
        self.order = [i for _, i in sorted(free)]  # poses by id, then landmarks by id
        self.off, o = {}, 0
        for i in self.order:
            self.off[i] = o
            o += V_DIM[self.row[i][0].vtype]
        self.n = o
        self.npose = sum(V_DIM[self.row[i][0].vtype] for i in self.order if not self.row[i][0].marginalized[self.row[i][1]])

    def _est(self, est, i):
        vs, k = self.row[int(i)]
        src = vs.est if est is None or vs.vtype not in est else np.asarray(est[vs.vtype])
        return vs.vtype, np.asarray(src[k], np.float64)

    def active(self, es, k):
        """A unary edge on a fixed vertex is inactive (sparse_optimizer.cpp:241)."""
        vs, r = self.row[int(es.v0[k])]
        return es.v1 is not None or not vs.fixed[r]

    def edge(self, es, k, est=None, binary=None):
        """(e, [(vertex id, J), ...]) of edge k of an edge set."""
        i = int(es.v0[k])
        _, xi = self._est(est, i)
        if es.v1 is None:
            off = None if es.params is None else es.params[k]
            return prior_error(es.etype, xi, es.meas[k], off), [(i, prior_jacobian(es.etype, xi, es.meas[k], off))]
        j = int(es.v1[k])
        _, xj = self._est(est, j)
        if es.etype == synth.E_SE2:
            e, Ji, Jj = se2_edge(xi, xj, es.meas[k])
        elif es.etype == synth.E_SE2_XY:
            e, Ji, Jj = se2_xy_edge(xi, xj, es.meas[k])
        else:
            D = synth.ERR_DIM[es.etype]
            di, dj = V_DIM[self.row[i][0].vtype], V_DIM[self.row[j][0].vtype]
            rec = np.asarray(binary[es.etype]).reshape(len(es.v0), D * (1 + di + dj))[k]
            e, Ji, Jj = rec[:D], rec[D:D + D * di].reshape(D, di), rec[D + D * di:].reshape(D, dj)
        return e, [(i, Ji), (j, Jj)]

    def chi2(self, est=None, robust=None, binary=None, only=None):
        c = 0.0
        for es in self.prob.edges:
            if only is not None and es.etype not in only:
                continue
            kind, delta = (robust or {}).get(es.etype, (None, 1.0))
            for k in range(len(es.v0)):
                if self.active(es, k):
                    e, _ = self.edge(es, k, est, binary)
                    c += robustify(kind, delta, float(e @ es.info[k] @ e))[0]
        return c

    def prior_payload(self, etype, est=None):
        """[e | Ji] row-major per edge of one prior type: its G2OHIP_E_HOSTJ_UNARY(D) records."""
        out = []
        for es in self.prob.edges:
            if es.etype == etype:
                for k in range(len(es.v0)):
                    e, ((_, J),) = self.edge(es, k, est)
                    out += [e, J.ravel()]
        return np.concatenate(out)

    def dense_system(self, est=None, robust=None, binary=None):
        """(H, b): b = -sum rho' J^T Omega e, H = sum J^T (rho' Omega) J (base_unary_edge.hpp:57-77 and its binary
        counterpart) over the active edges, hessian order."""
        H, b = np.zeros((self.n, self.n)), np.zeros(self.n)
        for es in self.prob.edges:
            kind, delta = (robust or {}).get(es.etype, (None, 1.0))
            for k in range(len(es.v0)):
                if not self.active(es, k):
                    continue
                e, Js = self.edge(es, k, est, binary)
                Om = np.asarray(es.info[k], np.float64)
                Om = Om * robustify(kind, delta, float(e @ Om @ e))[1]
                Js = [(self.off[i], J) for i, J in Js if i in self.off]
                for oa, Ja in Js:
                    b[oa:oa + Ja.shape[1]] -= Ja.T @ Om @ e
                    for ob, Jb in Js:
                        H[oa:oa + Ja.shape[1], ob:ob + Jb.shape[1]] += Ja.T @ Om @ Jb
        return H, b


def solve(H, b, npose, lam, ld=0):
    """BlockSolver::solve at lambda: (Hschur, bschur, x); without landmarks Hschur = Hpp + lam I, bschur = b."""
    n = len(b)
    Hd = H + lam * np.eye(n)
    if n == npose:
        return Hd, b.copy(), np.linalg.solve(Hd, b)
    Hpp, Hpl, Hll = Hd[:npose, :npose], Hd[:npose, npose:], Hd[npose:, npose:]
    Dinv = np.zeros_like(Hll)
    for o in range(0, n - npose, ld):
        Dinv[o:o + ld, o:o + ld] = np.linalg.inv(Hll[o:o + ld, o:o + ld])
    W = Hpl @ Dinv
    Hs, bs = Hpp - W @ Hpl.T, b[:npose] - W @ b[npose:]
    xp = np.linalg.solve(Hs, bs)
    return Hs, bs, np.concatenate([xp, Dinv @ (b[npose:] - Hpl.T @ xp)])
