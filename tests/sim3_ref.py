"""Plain-numpy restatement of types/sim3 (test reference; nothing here is taken from the library). It forms M and the
adjoints as 7x7 matrices, which the device never does; the scalar derivatives of A, B, C in _coef are the same
closed-form expressions the device differentiates, so what makes this a reference is tests/test_sim3_host.py, which pins
every branch of it against central differences in longdouble.

A similarity g = (q, t, s) acts as x -> s R(q) x + t; records are [n, 8] tx ty tz qx qy qz qw s, the layout of the
vertex estimate and of the measurement. Tangent vectors are (omega, upsilon, sigma).

  exp(u)     s = e^sigma, R = Rodrigues(omega), t = W upsilon, W = A [omega]x + B [omega]x^2 + C I, with A, B, C in the
             reference's four branches: |sigma| < 1e-5 or not, theta < 1e-5 or not (the series R = I + O + O^2 / 2 in
             the small-theta ones); the rotation becomes a quaternion by Eigen's Quaternion(Matrix3), not normalised.
  log(g)     sigma = ln s; d = (tr R - 1) / 2; omega = deltaR / 2 when d > 1 - 1e-5, else acos(d) / (2 sqrt(1 - d^2))
             deltaR; A, B, C again by branch; upsilon = W^-1 t.
  g * h      (q_g q_h, s_g R_g t_h + t_g, s_g s_h), nothing normalised;  g^-1 = (conj q, conj q * (-t / s), 1 / s) with
             the quaternion then brought to unit length and w >= 0 (the constructor's normalizeRotation).
  oplus      exp(u) * g, update[6] zeroed first under fix_scale; nothing normalised afterwards.
  EdgeSim3   E = C * S0 * S1^-1, e = log E.

Jacobians. Moving S0 by exp(u) moves E to exp(Ad_C u) E, moving S1 moves it to exp(-Ad_E u) E, with
Ad(g) = [[R, 0, 0], [[t]x R, s R, -t], [0, 0, 1]]. So Ji = M Ad(C), Jj = -M Ad(E), M = d log(exp(d) E) / d d at 0, and
to first order exp(d) E = ((I + [dw]x) R, t + dw x t + dv + ds t, s (1 + ds)):
  omega rows   omega = k(d) deltaR(R): d deltaR / d dw = tr(R) I - R, d d / d dw = -deltaR^T / 2, so
               J_w = k (tr(R) I - R) - k'(d) / 2 deltaR deltaR^T; k = 1/2, k' = 0 in the small-angle branch, else
               k = theta / (2 sin theta), k' = (d theta / sin theta - 1) / (2 sin^2 theta)
  sigma row    (0, 0, 1)
  upsilon rows W upsilon = t, so d upsilon = W^-1 (dt - dW upsilon), dt = [-[t]x | I | t] d, and
               dW upsilon = P d omega + p_s d sigma,
               P = (A_th O u + B_th O^2 u) omega^T / theta - A [u]x - B ([O u]x + O [u]x),  p_s = A_s O u + B_s O^2 u + C_s u
               (O = [omega]x, u = upsilon); A_th .. C_s are the derivatives of each branch's own formula, zero where the
               branch takes a constant. theta is acos(d) = |omega| in the branches that use it.
Under fix_scale column 6 of Ji and Jj is zero: the reference differentiates numerically through oplusImpl, which zeroes
update[6].

Every function takes batches and a dtype; np.longdouble is the high-precision mode. Graph plugs EdgeSim3 into
unary_ref.Graph (dense system, chi2, robust kernels); Dense wraps a problem for dogleg_ref.Dogleg and the LM loop below.
"""
import numpy as np

import unary_ref
from g2o_amd import synth
from pose_edges_ref import LD, _T, _a, _es, _mv, _spd, _vs, skew

V_SIM3, E_SIM3 = synth.V_SIM3, synth.E_SIM3
HOSTJ = 32 + 7
EPS = 0.00001  # the reference's threshold, a double constant in every dtype
TAGS = {"vertex": "VERTEX_SIM3:EXPMAP", "edge": "EDGE_SIM3:EXPMAP"}
unary_ref.V_DIM.setdefault(V_SIM3, 7)


# ---------------------------------------------------------------- quaternions as Eigen treats them
def rotm(q):
    """toRotationMatrix of (x, y, z, w) [n, 4], no normalisation: I + 2 w [v]x + 2 [v]x^2."""
    S = skew(q[:, :3])
    return np.eye(3, dtype=q.dtype) + 2 * q[:, 3, None, None] * S + 2 * (S @ S)


def qrot(q, v):
    """Quaternion * vector: v + 2 w (q_v x v) + 2 q_v x (q_v x v)."""
    uv = 2 * np.cross(q[:, :3], v)
    return v + q[:, 3:4] * uv + np.cross(q[:, :3], uv)


def qmul(a, b):
    av, aw, bv, bw = a[:, :3], a[:, 3:4], b[:, :3], b[:, 3:4]
    return np.concatenate([aw * bv + bw * av + np.cross(av, bv), aw * bw - np.sum(av * bv, 1, keepdims=True)], 1)


def quat_of(R):
    """Quaternion(Matrix3) [n, 3, 3] -> (x, y, z, w), not normalised: from the trace when it is positive, else from the
    largest diagonal entry."""
    out = np.zeros((len(R), 4), R.dtype)
    for n, M in enumerate(R):
        tr = M[0, 0] + M[1, 1] + M[2, 2]
        if tr > 0:
            r = np.sqrt(tr + 1)
            out[n] = [(M[2, 1] - M[1, 2]) / (2 * r), (M[0, 2] - M[2, 0]) / (2 * r), (M[1, 0] - M[0, 1]) / (2 * r), r / 2]
        else:
            i = int(np.argmax([M[0, 0], M[1, 1], M[2, 2]]))
            j, k = (i + 1) % 3, (i + 2) % 3
            r = np.sqrt(M[i, i] - M[j, j] - M[k, k] + 1)
            out[n, i], out[n, 3] = r / 2, (M[k, j] - M[j, k]) / (2 * r)
            out[n, j], out[n, k] = (M[j, i] + M[i, j]) / (2 * r), (M[k, i] + M[i, k]) / (2 * r)
    return out


# ---------------------------------------------------------------- the group
def parts(S, dtype=np.float64):
    S = _a(S, dtype)
    return S[:, 3:7], S[:, 0:3], S[:, 7]


def pack(q, t, s):
    return np.concatenate([t, q, np.asarray(s)[:, None]], 1)


def normalized(S, dtype=np.float64):
    """Sim3(q, t, s)'s normalizeRotation: w >= 0, unit length. What the handle does to estimates and measurements."""
    q, t, s = parts(S, dtype)
    q = np.where(q[:, 3:4] < 0, -q, q)
    return pack(q / np.sqrt(np.sum(q * q, 1, keepdims=True)), t, s)


def mul(a, b, dtype=np.float64):
    (qa, ta, sa), (qb, tb, sb) = parts(a, dtype), parts(b, dtype)
    return pack(qmul(qa, qb), sa[:, None] * qrot(qa, tb) + ta, sa * sb)


def inv(a, dtype=np.float64):
    q, t, s = parts(a, dtype)
    qc = q * np.array([-1, -1, -1, 1], dtype)
    return normalized(pack(qc, qrot(qc, (-1 / s)[:, None] * t), 1 / s), dtype)


def _coef(theta, sigma, small_t, dtype):
    """A, B, C of W and their derivatives in theta and sigma, per branch: (A, B, C, A_th, B_th, A_s, B_s, C_s)."""
    one, zero = dtype(1), dtype(0)
    small_s = np.abs(sigma) < dtype(EPS)
    s = np.exp(sigma)
    sg, th = np.where(small_s, one, sigma), np.where(small_t, one, theta)  # safe denominators of the unused branches
    sn, cs, th2, sg2 = np.sin(th), np.cos(th), th * th, sg * sg
    # |sigma| < eps, theta general
    A1, B1 = (1 - cs) / th2, (th - sn) / (th2 * th)
    A1t, B1t = sn / th2 - 2 * (1 - cs) / (th2 * th), (1 - cs) / (th2 * th) - 3 * (th - sn) / (th2 * th2)
    # sigma general
    Cg = (s - 1) / sg
    Cgs = (s - Cg) / sg
    A3, B3 = ((sg - 1) * s + 1) / sg2, ((dtype(0.5) * sg2 - sg + 1) * s - 1) / (sg2 * sg)
    A3s, B3s = (s - 2 * A3) / sg, (dtype(0.5) * s - 3 * B3) / sg
    a, b, c = s * sn, s * cs, th2 + sg2
    A4 = (a * sg + (1 - b) * th) / (th * c)
    G = ((b - 1) * sg + a * th) / c
    B4 = (Cg - G) / th2
    A4t = (b * sg + a * th + (1 - b)) / (th * c) - A4 * (c + 2 * th2) / (th * c)
    A4s = (a + a * sg - b * th) / (th * c) - A4 * 2 * sg / c
    Gt = (-a * sg + b * th + a) / c - G * 2 * th / c
    Gs = (b * sg + (b - 1) + a * th) / c - G * 2 * sg / c
    B4t, B4s = -Gt / th2 - 2 * B4 / th, (Cgs - Gs) / th2

    def pick(ss_st, ss, st, gen):
        return np.where(small_s, np.where(small_t, ss_st, ss), np.where(small_t, st, gen))

    half, sixth = dtype(1) / 2, dtype(1) / 6
    return (pick(half, A1, A3, A4), pick(sixth, B1, B3, B4), np.where(small_s, one, Cg),
            pick(zero, A1t, zero, A4t), pick(zero, B1t, zero, B4t),
            pick(zero, zero, A3s, A4s), pick(zero, zero, B3s, B4s), np.where(small_s, zero, Cgs))


def exp(u, dtype=np.float64):
    """Sim3(Vector7): [n, 7] (omega, upsilon, sigma) -> records."""
    u = _a(u, dtype)
    om, ups, sigma = u[:, :3], u[:, 3:6], u[:, 6]
    theta = np.sqrt(np.sum(om * om, 1))
    small_t = theta < dtype(EPS)
    O = skew(om)
    O2 = O @ O
    eye = np.eye(3, dtype=dtype)
    th = np.where(small_t, dtype(1), theta)
    ra = np.where(small_t, dtype(1), np.sin(th) / th)[:, None, None]
    rb = np.where(small_t, dtype(1) / 2, (1 - np.cos(th)) / (th * th))[:, None, None]
    A, B, C = _coef(theta, sigma, small_t, dtype)[:3]
    W = A[:, None, None] * O + B[:, None, None] * O2 + C[:, None, None] * eye
    return pack(quat_of(eye + ra * O + rb * O2), _mv(W, ups), np.exp(sigma))


def inv3(M):
    """3x3 inverses by the adjugate (rows of the inverse are cross products of the columns)."""
    c0, c1, c2 = M[:, :, 0], M[:, :, 1], M[:, :, 2]
    r0, r1, r2 = np.cross(c1, c2), np.cross(c2, c0), np.cross(c0, c1)
    det = np.sum(c0 * r0, 1)
    return np.stack([r0, r1, r2], 1) / det[:, None, None]


def branch(S, dtype=np.float64):
    """(small sigma, small theta) of log's branch per record, and (|sigma|, d) for margins."""
    q, _, s = parts(S, dtype)
    R = rotm(q)
    d = (R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2] - 1) / 2
    sigma = np.log(s)
    return np.abs(sigma) < dtype(EPS), d > 1 - dtype(EPS), np.abs(sigma), d


def log(S, dtype=np.float64, jac=False):
    """Sim3::log: [n, 7]; with jac also M [n, 7, 7] = d log(exp(d) g) / d d at 0."""
    q, t, s = parts(S, dtype)
    n = len(s)
    R = rotm(q)
    tr = R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]
    d = (tr - 1) / 2
    sigma = np.log(s)
    dR = np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], 1)
    small_t = d > 1 - dtype(EPS)
    dd = np.where(small_t, dtype(0), d)
    theta = np.arccos(dd)
    sin = np.sqrt(1 - dd * dd)
    k = np.where(small_t, dtype(1) / 2, theta / (2 * sin))
    om = k[:, None] * dR
    A, B, C, At, Bt, As, Bs, Cs = _coef(theta, sigma, small_t, dtype)
    eye = np.eye(3, dtype=dtype)
    O = skew(om)
    W = A[:, None, None] * O + B[:, None, None] * (O @ O) + C[:, None, None] * eye
    Wi = inv3(W)
    ups = _mv(Wi, t)
    e = np.concatenate([om, ups, sigma[:, None]], 1)
    if not jac:
        return e
    kp = np.where(small_t, dtype(0), (dd * theta / sin - 1) / (2 * sin * sin))
    Jw = k[:, None, None] * (tr[:, None, None] * eye - R) - (kp / 2)[:, None, None] * dR[:, :, None] * dR[:, None, :]
    axis = np.where(small_t[:, None], dtype(0), om / np.where(small_t, dtype(1), theta)[:, None])
    Ou = _mv(O, ups)
    O2u = _mv(O, Ou)
    P = ((At[:, None] * Ou + Bt[:, None] * O2u)[:, :, None] * axis[:, None, :] - A[:, None, None] * skew(ups) -
         B[:, None, None] * (skew(Ou) + O @ skew(ups)))
    ps = As[:, None] * Ou + Bs[:, None] * O2u + Cs[:, None] * ups
    M = np.zeros((n, 7, 7), dtype)
    M[:, :3, :3] = Jw
    M[:, 3:6, :3] = Wi @ (-skew(t) - P @ Jw)
    M[:, 3:6, 3:6] = Wi
    M[:, 3:6, 6] = ups - _mv(Wi, ps)
    M[:, 6, 6] = 1
    return e, M


def adj(S, dtype=np.float64):
    q, t, s = parts(S, dtype)
    R = rotm(q)
    Ad = np.zeros((len(s), 7, 7), dtype)
    Ad[:, :3, :3] = R
    Ad[:, 3:6, :3] = skew(t) @ R
    Ad[:, 3:6, 3:6] = s[:, None, None] * R
    Ad[:, 3:6, 6] = -t
    Ad[:, 6, 6] = 1
    return Ad


def oplus(est, u, fix_scale=False, dtype=np.float64):
    u = np.array(_a(u, dtype))
    if fix_scale:
        u[:, 6] = 0
    return mul(exp(u, dtype), est, dtype)


def edge(xi, xj, z, dtype=np.float64, jac=True, fix_scale=False):
    """EdgeSim3: e [n, 7] and, with jac, Ji, Jj [n, 7, 7]. The measurement is normalised, the vertices are taken as
    given (the handle normalised them on entry; oplus does not)."""
    C = normalized(z, dtype)
    E = mul(mul(C, xi, dtype), inv(xj, dtype), dtype)
    if not jac:
        return log(E, dtype)
    e, M = log(E, dtype, True)
    Ji, Jj = M @ adj(C, dtype), -(M @ adj(E, dtype))
    if fix_scale:
        Ji[:, :, 6] = 0
        Jj[:, :, 6] = 0
    return e, Ji, Jj


def minimal(est, dtype=np.float64):
    """g2ohip_minimal_state of Sim3 vertices: log()."""
    return log(est, dtype)


# ---------------------------------------------------------------- the projection edges (host-J in the library)
def project_edge(p, S, obs, fl=(1.0, 1.0), pp=(0.0, 0.0), inverse=False, dtype=np.float64):
    """EdgeSim3ProjectXYZ (inverse: EdgeInverseSim3ProjectXYZ): obs - cam_map(project(S.map(p))), [n, 2]."""
    S = _a(S, dtype)
    g = inv(S, dtype) if inverse else S
    q, t, s = parts(g, dtype)
    x = s[:, None] * qrot(q, _a(p, dtype)) + t
    return _a(obs, dtype) - (x[:, :2] / x[:, 2:3] * np.asarray(fl, dtype) + np.asarray(pp, dtype))


def project_records(p, S, obs, fl=(1.0, 1.0), pp=(0.0, 0.0), inverse=False, fix_scale=False, h=1e-6):
    """[e | Ji (2 x 3) | Jj (2 x 7)] per edge as the reference's numeric linearizeOplus forms them (central differences
    through the vertices' oplus), here with h = 1e-6 in longdouble."""
    p, S = _a(p, LD), _a(S, LD)
    n = len(p)
    e = project_edge(p, S, obs, fl, pp, inverse, LD)
    Ji, Jj = np.zeros((n, 2, 3), LD), np.zeros((n, 2, 7), LD)
    for c in range(3):
        d = np.zeros((n, 3), LD)
        d[:, c] = h
        Ji[:, :, c] = (project_edge(p + d, S, obs, fl, pp, inverse, LD) - project_edge(p - d, S, obs, fl, pp, inverse, LD)) / (2 * h)
    for c in range(7):
        d = np.zeros((n, 7), LD)
        d[:, c] = h
        Jj[:, :, c] = (project_edge(p, oplus(S, d, fix_scale, LD), obs, fl, pp, inverse, LD) -
                       project_edge(p, oplus(S, -d, fix_scale, LD), obs, fl, pp, inverse, LD)) / (2 * h)
    return np.concatenate([e, Ji.reshape(n, -1), Jj.reshape(n, -1)], 1).astype(np.float64)


# ---------------------------------------------------------------- graphs
class Graph(unary_ref.Graph):
    """unary_ref.Graph with EdgeSim3 restated here; fix_scale as g2ohip_set_sim3_fix_scale."""

    def __init__(self, prob, fix_scale=False):
        super().__init__(prob)
        self.fix_scale = fix_scale

    def edge(self, es, k, est=None, binary=None):
        if es.etype == E_SIM3 and not (binary and es.etype in binary):
            i, j = int(es.v0[k]), int(es.v1[k])
            e, Ji, Jj = edge(self._est(est, i)[1], self._est(est, j)[1], es.meas[k], fix_scale=self.fix_scale)
            return e[0], [(i, Ji[0]), (j, Jj[0])]
        if es.v1 is not None and 32 < es.etype <= HOSTJ:  # a host-J set: the caller's [e | Ji | Jj] records
            i, j = int(es.v0[k]), int(es.v1[k])
            D, di, dj = es.etype - 32, unary_ref.V_DIM[self.row[i][0].vtype], unary_ref.V_DIM[self.row[j][0].vtype]
            rec = np.asarray(binary[es.etype]).reshape(len(es.v0), D * (1 + di + dj))[k]
            return rec[:D], [(i, rec[D:D + D * di].reshape(D, di)), (j, rec[D + D * di:].reshape(D, dj))]
        return super().edge(es, k, est, binary)

    def _rows(self, est, ids):
        vs = self.row[int(ids[0])][0]
        src = vs.est if est is None or vs.vtype not in est else np.asarray(est[vs.vtype])
        order = np.argsort(vs.ids)
        return src[order[np.searchsorted(vs.ids[order], ids)]]

    def _sets(self):
        return [es for es in self.prob.edges if es.etype == E_SIM3]

    def batch(self, es, est=None, dtype=np.float64, jac=True):
        return edge(self._rows(est, es.v0), self._rows(est, es.v1), es.meas, dtype, jac, self.fix_scale)

    def payload(self, est=None):
        """[e | Ji | Jj] row-major per EdgeSim3: the records of the G2OHIP_E_HOSTJ(7) set that holds them."""
        out = []
        for es in self._sets():
            e, Ji, Jj = self.batch(es, est)
            n = len(e)
            out.append(np.concatenate([e, Ji.reshape(n, -1), Jj.reshape(n, -1)], 1).ravel())
        return np.concatenate(out)

    def edge_chi2(self, est=None, dtype=np.float64):
        """e^T Omega e of every EdgeSim3, in order."""
        out = []
        for es in self._sets():
            e = self.batch(es, est, dtype, False)
            out.append(np.einsum("ni,nij,nj->n", e, np.asarray(es.info, dtype), e))
        return np.concatenate(out)

    def chi2_in(self, dtype, est=None):
        return np.sum(self.edge_chi2(est, dtype))


def numpy_stage(prob, lam=None, robust=None, est=None, fix_scale=False, binary=None):
    """The dense system and its solve; lam None: LM's own first lambda, 1e-5 max diag(H)."""
    g = Graph(prob, fix_scale)
    H, b = g.dense_system(est=est, robust=robust, binary=binary)
    if lam is None:
        lam = 1e-5 * float(np.max(np.diag(H)))
    Hs, bs, x = unary_ref.solve(H, b, g.npose, lam, prob.landmark_dim)
    return dict(b=b, x=x, Hschur=Hs, bschur=bs, np=g.npose, n=g.n, lam=lam, H=H)


def hostj_problem(prob):
    return synth.sim3_twin(prob)


# ---------------------------------------------------------------- optimizers over a dense system, in a dtype
def solve_spd(H, b):
    """Gaussian elimination without pivoting in H's dtype (numpy's solvers stop at float64): for a symmetric matrix the
    pivots are those of LDL^T, all positive exactly when it is positive definite; (x, positive pivots)."""
    A = np.concatenate([H, b[:, None]], 1).copy()
    n = len(b)
    ok = True
    for c in range(n):
        ok = ok and bool(A[c, c] > 0)
        if not ok:
            return np.zeros(n, H.dtype), False
        A[c + 1:] -= (A[c + 1:, c] / A[c, c])[:, None] * A[c]
    x = np.zeros(n, H.dtype)
    for c in range(n - 1, -1, -1):
        x[c] = (A[c, n] - A[c, c + 1:n] @ x[c + 1:]) / A[c, c]
    return x, ok


class Dense:
    """A pose-only Sim3 problem evaluated in a dtype, with the calls dogleg_ref.Dogleg and lm() make: chi2, stage,
    hessian_dense, push, update, pop, discard_top."""

    def __init__(self, prob, dtype=np.float64, robust=None, fix_scale=False):
        self.g, self.dtype, self.fix_scale = Graph(prob, fix_scale), dtype, fix_scale
        self.es = self.g._sets()
        assert len(self.es) == 1 and len(prob.edges) == 1
        vs = prob.vertices[0]
        self.vs, self.est = vs, normalized(vs.est, dtype)
        self.robust = robust  # (kind, delta) or None
        self.stack = []
        self.rowof = {int(i): k for k, i in enumerate(vs.ids)}

    def _edges(self, jac):
        return self.g.batch(self.es[0], {V_SIM3: self.est}, self.dtype, jac)

    def _rho(self, c):
        if not self.robust:
            return c, np.ones_like(c)
        r = [unary_ref.robustify(self.robust[0], self.dtype(self.robust[1]), x) for x in c]
        return np.array([a for a, _ in r], self.dtype), np.array([w for _, w in r], self.dtype)

    def chi2(self):
        e = self._edges(False)
        return self.dtype(np.sum(self._rho(np.einsum("ni,nij,nj->n", e, np.asarray(self.es[0].info, self.dtype), e))[0]))

    def system(self):
        es, g = self.es[0], self.g
        e, Ji, Jj = self._edges(True)
        Om = np.asarray(es.info, self.dtype)
        Om = Om * self._rho(np.einsum("ni,nij,nj->n", e, Om, e))[1][:, None, None]
        H, b = np.zeros((g.n, g.n), self.dtype), np.zeros(g.n, self.dtype)
        for k in range(len(e)):
            Js = [(g.off[int(v)], J[k]) for v, J in ((es.v0[k], Ji), (es.v1[k], Jj)) if int(v) in g.off]
            for oa, Ja in Js:
                b[oa:oa + 7] -= Ja.T @ Om[k] @ e[k]
                for ob, Jb in Js:
                    H[oa:oa + 7, ob:ob + 7] += Ja.T @ Om[k] @ Jb
        return H, b

    def stage(self, lam, cfg=None):
        H, b = self.system()
        self.H = H
        x, ok = solve_spd(H + self.dtype(lam) * np.eye(len(b), dtype=self.dtype), b)
        return dict(ok=ok, b=b, x=x, np=len(b), nl=0)

    def hessian_dense(self, npose, nl):
        return (self.H,)

    def push(self):
        self.stack.append(self.est.copy())

    def pop(self):
        self.est = self.stack.pop()

    def discard_top(self):
        self.stack.pop()

    def update(self, x):
        g = self.g
        for i, o in g.off.items():
            r = self.rowof[i]
            self.est[r] = oplus(self.est[r], x[o:o + 7], self.fix_scale, self.dtype)[0]

    def minimal_state(self):
        return minimal(self.est, self.dtype).ravel()


def lm(dense, iterations, max_trials=10):
    """OptimizationAlgorithmLevenberg::solve per iteration (optimization_algorithm_levenberg.cpp:58-150):
    [(chi2 after, trials, [rho of each trial])]."""
    dt = dense.dtype
    lam, ni, out = None, dt(2), []
    for it in range(iterations):
        chi = dense.chi2()
        H, b = dense.system()
        if it == 0:
            lam = dt(1e-5) * np.max(np.diag(H))
        rhos, rho, tries, new_chi = [], dt(0), 0, chi
        while True:
            dense.push()
            x, ok = solve_spd(H + lam * np.eye(len(b), dtype=dt), b)
            if ok:
                dense.update(x)
                t_chi = dense.chi2()
            else:
                t_chi = dt(np.inf)
            scale = x @ (lam * x + b) + dt(1e-3) if ok else dt(1)
            rho = (chi - t_chi) / scale if ok else dt(-1)
            rhos.append(float(rho))
            if rho > 0 and np.isfinite(t_chi):
                alpha = min(dt(1) - (2 * rho - 1) ** 3, dt(2) / 3)
                lam = lam * max(dt(1) / 3, alpha)
                ni = dt(2)
                new_chi = t_chi
                dense.discard_top()
            else:
                lam, ni = lam * ni, ni * 2
                dense.pop()
            tries += 1
            if rho > 0 or tries >= max_trials or not np.isfinite(float(lam)):
                break
        out.append((float(new_chi), tries, rhos))
        if rho <= 0:
            break
    return out


# ---------------------------------------------------------------- cases
def _unit(q):
    q = np.asarray(q, np.float64)
    return q / np.linalg.norm(q)


def _rand_sim3(rng, scale=(0.6, 1.7)):
    q = _unit(rng.standard_normal(4))
    return np.concatenate([rng.uniform(-1, 1, 3), q if q[3] >= 0 else -q, [rng.uniform(*scale)]])


# the four branches of exp and of log: (label, theta, sigma); a second general case with a large angle and s < 1
BRANCHES = [("small-theta small-sigma", 2e-6, 3e-6), ("theta small-sigma", 0.7, -4e-6), ("small-theta sigma", 3e-6, 0.3),
            ("theta sigma", 0.5, 0.25), ("large theta sigma<0", 1.9, -0.4)]
# log's small-angle branch reaches to d = 1 - 1e-5, theta ~ 4.5e-3, far beyond exp's theta < 1e-5
LOG_BRANCHES = BRANCHES + [("log small-theta small-sigma", 1e-3, -2e-6), ("log small-theta sigma", 1.5e-3, 0.05)]


def exp_cases():
    """[(label, u)]: updates in each branch of exp."""
    rng = np.random.default_rng(7101)
    out = []
    for label, theta, sigma in BRANCHES:
        ax = rng.standard_normal(3)
        out.append((label, np.concatenate([theta * ax / np.linalg.norm(ax), rng.uniform(-0.5, 0.5, 3), [sigma]])))
    return out


def log_cases():
    """[(label, xi, xj, z)]: the error E = C S0 S1^-1 of the edge is exp of a vector in the label's branch of log:
    S1 = E^-1 C S0, formed in longdouble. Each case is checked against the branch thresholds with a margin."""
    rng = np.random.default_rng(7102)
    out = []
    for label, theta, sigma in LOG_BRANCHES:
        ax = rng.standard_normal(3)
        xi_e = np.concatenate([theta * ax / np.linalg.norm(ax), rng.uniform(-0.4, 0.4, 3), [sigma]])
        xi, z = _rand_sim3(rng), _rand_sim3(rng)
        xj = mul(inv(exp(xi_e, LD), LD), mul(normalized(z, LD), xi, LD), LD)
        xj = normalized(xj.astype(np.float64))[0]
        ss, st, asg, d = branch(mul(mul(normalized(z), xi), inv(xj)))
        want_ss, want_st = abs(sigma) < EPS, np.cos(theta) > 1 - EPS
        assert (bool(ss[0]), bool(st[0])) == (want_ss, want_st), label
        assert abs(asg[0] - EPS) > 0.5 * EPS and abs(d[0] - (1 - EPS)) > 0.4 * EPS, label  # clear of both thresholds
        out.append((label, xi, xj, z))
    return out


def one_edge(case=None, seed=0, fixed=(0, 0)):
    """Two Sim3 vertices (ids 3, 8) and one EdgeSim3 with a non-diagonal information matrix."""
    _, xi, xj, z = case or log_cases()[3]
    info = _spd(np.random.default_rng(900 + seed), 7)
    return synth.Problem("sim3one", [_vs(V_SIM3, [3, 8], [xi, xj], fixed)], [_es(E_SIM3, [3], [8], z[None], info)], 7, 0)


def edge_case(ne, uniform=False):
    """Exactly ne edges: a chain of ne + 1 keyframes, every 8th fixed (ne = 1: both free), whose k-th edge has the
    error of log case k mod len(LOG_BRANCHES) (so every wave meets every branch): S_{k+1} = E_k^-1 C_k S_k. uniform: one
    information matrix for every edge (EdgeData::ue bit 0), else all distinct."""
    rng = np.random.default_rng(7200 + ne)
    est, meas = [_rand_sim3(rng)], []
    for k in range(ne):
        _, theta, sigma = LOG_BRANCHES[k % len(LOG_BRANCHES)]
        ax = rng.standard_normal(3)
        xi_e = np.concatenate([theta * ax / np.linalg.norm(ax), rng.uniform(-0.3, 0.3, 3), [sigma]])
        z = _rand_sim3(rng, (0.8, 1.25))
        nxt = mul(inv(exp(xi_e, LD), LD), mul(normalized(z, LD), est[-1], LD), LD)
        est.append(normalized(nxt.astype(np.float64))[0])
        meas.append(z)
    fx = np.zeros(ne + 1, np.int32)
    if ne > 1:
        fx[::8] = 1
    info = _spd(rng, 7, ne)
    if uniform:
        info = np.broadcast_to(info[:1], info.shape).copy()
    return synth.Problem(f"sim3chain{ne}u{int(uniform)}", [_vs(V_SIM3, np.arange(ne + 1), est, fx)],
                         [_es(E_SIM3, np.arange(ne), np.arange(1, ne + 1), meas, info)], 7, 0)


def projection_problem(n_points=24, inverse=False, seed=0):
    """OptimizeSim3's shape: n fixed points, one free Sim3 vertex, EdgeSim3ProjectXYZ (or the inverse edge) entered as
    G2OHIP_E_HOSTJ(2) between each point and the vertex. Returns (problem, records())."""
    rng = np.random.default_rng(7300 + seed + 10 * inverse)
    S = np.concatenate([rng.uniform(-0.2, 0.2, 3), _unit([0.05, -0.08, 0.03, 1.0]), [1.2]])
    pts_cam = np.stack([rng.uniform(-1, 1, n_points), rng.uniform(-1, 1, n_points), rng.uniform(3, 6, n_points)], 1)
    g = inv(S) if not inverse else S[None]
    q, t, s = parts(g)
    pts = s[:, None] * qrot(np.repeat(q, n_points, 0), pts_cam) + t  # the points in the frame the edge maps from
    fl, pp = (420.0, 415.0), (320.0, 240.0)
    Srep = np.repeat(S[None], n_points, 0)
    obs = -project_edge(pts, Srep, np.zeros((n_points, 2)), fl, pp, inverse) + rng.standard_normal((n_points, 2))
    start = oplus(S, np.concatenate([rng.standard_normal(6) * 0.01, [0.02]]))[0]
    ids = np.arange(n_points)
    prob = synth.Problem(f"sim3proj{int(inverse)}", [_vs(synth.V_XYZ, ids, pts, np.ones(n_points, np.int32)),
                                                     _vs(V_SIM3, [n_points], [start])],
                         [_es(32 + 2, ids, np.full(n_points, n_points), np.zeros((n_points, 0)),
                              _spd(rng, 2, n_points))], 7, 0)
    prob.edges[0].meas = None

    def records(est, fix_scale=False):
        return project_records(pts, np.repeat(np.asarray(est)[None], n_points, 0), obs, fl, pp, inverse, fix_scale)
    return prob, records


def arc_problem(first=26, last=40):
    """Keyframes first .. last - 1 of synth.sim3_pose_graph() with the edges among them, the first one fixed: an arc of
    the ring. The .g2o lines hold logs of cam2world transforms, and Sim3::log loses digits as eps / (pi - theta)^2 near
    a half turn (acos(d) and sqrt(1 - d^2) at d -> -1; keyframe 20 of the full ring sits 0.0099 rad from pi and comes
    back from its line with 7e-11). On this arc every rotation a line takes the log of is at least 0.7 rad clear of pi
    (asserted), so the text carries the state to rounding."""
    prob = synth.sim3_pose_graph()
    vs, es = prob.vertices[0], prob.edges[0]
    keep = (es.v0 >= first) & (es.v0 < last) & (es.v1 >= first) & (es.v1 < last)
    fx = np.zeros(last - first, np.int32)
    fx[0] = 1
    out = synth.Problem(f"sim3arc{first}_{last}", [_vs(V_SIM3, vs.ids[first:last], vs.est[first:last], fx)],
                        [_es(E_SIM3, es.v0[keep], es.v1[keep], es.meas[keep], es.info[keep])], 7, 0)
    for rec in (out.vertices[0].est, out.edges[0].meas):
        theta = np.linalg.norm(log(inv(normalized(rec)))[:, :3], axis=1)
        assert np.pi - theta.max() > 0.7
    return out


# ---------------------------------------------------------------- .g2o text (types_seven_dof_expmap.cpp:66-137)
def g2o_text(prob, intrinsics=(1.0, 1.0, 0.0, 0.0)):
    """The reference's lines for a Sim3 problem: VERTEX_SIM3:EXPMAP id log(estimate^-1) fx fy cx cy, EDGE_SIM3:EXPMAP
    v0 v1 log(measurement^-1) and the upper triangle of the information; FIX lines for the fixed vertices."""
    lines = []
    for vs in prob.vertices:
        assert vs.vtype == V_SIM3
        lv = log(inv(normalized(vs.est)))
        for i, v in zip(vs.ids, lv):
            lines.append("VERTEX_SIM3:EXPMAP %d " % i + " ".join(repr(float(x)) for x in v) + " " +
                         " ".join(repr(float(x)) for x in intrinsics))
        lines += ["FIX %d" % i for i, f in zip(vs.ids, vs.fixed) if f]
    for es in prob.edges:
        assert es.etype == E_SIM3
        lv = log(inv(normalized(es.meas)))
        for a, b, v, I in zip(es.v0, es.v1, lv, es.info):
            up = [I[r, c] for r in range(7) for c in range(r, 7)]
            lines.append("EDGE_SIM3:EXPMAP %d %d " % (a, b) + " ".join(repr(float(x)) for x in list(v) + up))
    return "\n".join(lines) + "\n"


def parse_g2o_text(text):
    """The reader's side: (ids, estimates, fixed ids, v0, v1, measurements, information) of the two tags."""
    ids, est, fix, v0, v1, meas, info = [], [], [], [], [], [], []
    for line in text.splitlines():
        w = line.split()
        if not w:
            continue
        if w[0] == "VERTEX_SIM3:EXPMAP":
            ids.append(int(w[1]))
            est.append(inv(exp(np.array(w[2:9], np.float64)))[0])
        elif w[0] == "FIX":
            fix += [int(x) for x in w[1:]]
        elif w[0] == "EDGE_SIM3:EXPMAP":
            v0.append(int(w[1]))
            v1.append(int(w[2]))
            meas.append(inv(exp(np.array(w[3:10], np.float64)))[0])
            up = np.array(w[10:38], np.float64)
            I = np.zeros((7, 7))
            I[np.triu_indices(7)] = up
            info.append(I + np.triu(I, 1).T)
    return np.array(ids), np.array(est), fix, np.array(v0), np.array(v1), np.array(meas), np.array(info)
