"""Plain-numpy restatement of the offset and bearing edges (test reference; written from the maths, nothing here comes
from the library, and none of it is a port of the device's skew / dq_dR code).

  EdgeSE3Offset          Ni = Xi Pi, Nj = Xj Pj, E = Z^-1 Ni^-1 Nj:  e = (t_E, q_v(R_E)), q_w >= 0
  EdgeSE2Offset          the same in SE2: e = (Rz^T (R_Ni^T (t_Nj - t_Ni) - tz), wrap(th_Nj - th_Ni - thz))
  EdgeSE2PointXYBearing  d = Ri^T (l - ti), e = wrap(z - atan2(d.y, d.x))

Jacobians. VertexSE3's oplus is X * (dt, dq): R <- R (I + 2 [dq]x), t <- t + R dt. With A = Z^-1 Pi^-1, B = Xi^-1 Xj,
C = Pj, E = A B C, q = (q_v, q_w) of R_E and Q = q_w I + [q_v]x (a right perturbation R_E (I + [w]x) moves q_v by Q w / 2):
  moving Xi: E = A (dt, dq)^-1 (B C):  d e_t / d t_i = -R_A,  d e_t / d q_i = 2 R_A [t_BC]x,  d e_q / d q_i = -Q R_BC^T
  moving Xj: E = (A B) (dt, dq) C:     d e_t / d t_j = R_AB,  d e_t / d q_j = -2 R_AB [t_C]x,  d e_q / d q_j = Q R_C^T
VertexSE2's oplus adds to x, y and to the angle. N = X * P has t_N = t + R(th) p, th_N = th + phi, so
d t_N / d th = R'(th) p with R'(th) = [[-s, -c], [c, -s]]:
  d e_t / d t_i = -Rz^T R_Ni^T          d e_t / d th_i = Rz^T (R_Ni'^T (t_Nj - t_Ni) - R_Ni^T R'(th_i) p_i)   d e_th / d th_i = -1
  d e_t / d t_j =  Rz^T R_Ni^T          d e_t / d th_j = Rz^T R_Ni^T R'(th_j) p_j                              d e_th / d th_j = 1
Bearing, with g = (-d.y, d.x) / |d|^2 the gradient of atan2:  Ji = [ g Ri^T | 1 ],  Jj = -g Ri^T  (d d / d th = (d.y, -d.x),
and g . (d.y, -d.x) = -1).

Every function takes batches and a dtype; np.longdouble is the high-precision mode. Graph plugs the edges into
unary_ref.Graph (dense system, chi2, robust kernels, priors, EdgeSE2, EdgeSE2PointXY; EdgeSE3 through pose_edges_ref);
Structure runs structure_only_ref over the bearing edges.
"""
import contextlib

import numpy as np

import pose_edges_ref as per
import structure_only_ref
import unary_ref
from g2o_amd import synth
from pose_edges_ref import LD, PI, SE2_ANGLES, _T, _a, _es, _mv, _qjac, _spd, _vs, quat, rot, rot2, skew, wrap

SE3O, SE2O, BEAR = synth.E_SE3_OFFSET, synth.E_SE2_OFFSET, synth.E_SE2_XY_BEARING
KINDS = (SE3O, SE2O, BEAR)
OFFSETS = (SE3O, SE2O)
TAGS = {SE3O: "EDGE_SE3_OFFSET", SE2O: "EDGE_SE2_OFFSET", BEAR: "EDGE_BEARING_SE2_XY"}
PTAGS = {SE3O: "PARAMS_SE3OFFSET", SE2O: "PARAMS_SE2OFFSET"}
HOSTJ = {SE3O: 32 + 6, SE2O: 32 + 3, BEAR: 32 + 1}
PLAIN = {SE3O: synth.E_SE3_QUAT, SE2O: synth.E_SE2}  # the edge an offset edge with identity offsets equals
VTYPE = {SE3O: synth.V_SE3_QUAT, SE2O: synth.V_SE2}
IDENT = {SE3O: np.array([0, 0, 0, 0, 0, 0, 1.0] * 2), SE2O: np.zeros(6)}


# ---------------------------------------------------------------- the three edges
def se3_offset_edge(xi, xj, z, P=None, dtype=np.float64, jac=True):
    """EdgeSE3Offset: e [n, 6] and, with jac, Ji, Jj [n, 6, 6]. P [n, 14]: the from vertex's offset, then the to
    vertex's (None: both the identity). The quaternions of the measurement and of the offsets are normalized, the
    vertices' are taken as given."""
    xi, xj, z = _a(xi, dtype), _a(xj, dtype), _a(z, dtype)
    P = _a(np.broadcast_to(IDENT[SE3O], (len(xi), 14)) if P is None else P, dtype)
    Ri, Rj, Rz = rot(xi[:, 3:], dtype, False), rot(xj[:, 3:], dtype, False), rot(z[:, 3:], dtype)
    Rpi, Rpj, tpi, tpj = rot(P[:, 3:7], dtype), rot(P[:, 10:14], dtype), P[:, 0:3], P[:, 7:10]
    Ra = _T(Rz) @ _T(Rpi)
    Rb, tb = _T(Ri) @ Rj, _mv(_T(Ri), xj[:, :3] - xi[:, :3])
    Rbc, tbc = Rb @ Rpj, tb + _mv(Rb, tpj)
    Rab = Ra @ Rb
    Re = Rab @ Rpj
    te = _mv(_T(Rz), _mv(_T(Rpi), tbc - tpi) - z[:, :3])
    q = quat(Re)
    e = np.concatenate([te, q[:, :3]], 1)
    if not jac:
        return e
    n = len(e)
    Ji, Jj = np.zeros((n, 6, 6), dtype), np.zeros((n, 6, 6), dtype)
    Q = _qjac(q)
    Ji[:, :3, :3], Ji[:, :3, 3:], Ji[:, 3:, 3:] = -Ra, 2 * Ra @ skew(tbc), -Q @ _T(Rbc)
    Jj[:, :3, :3], Jj[:, :3, 3:], Jj[:, 3:, 3:] = Rab, -2 * Rab @ skew(tpj), Q @ _T(Rpj)
    return e, Ji, Jj


def _drot2(th):
    c, s = np.cos(th), np.sin(th)
    return np.stack([np.stack([-s, -c], -1), np.stack([c, -s], -1)], -2)


def se2_offset_edge(xi, xj, z, P=None, dtype=np.float64, jac=True):
    """EdgeSE2Offset: e [n, 3], Ji, Jj [n, 3, 3]. P [n, 6]: the two offsets x y theta (None: the identity)."""
    xi, xj, z = _a(xi, dtype), _a(xj, dtype), _a(z, dtype)
    P = _a(np.zeros((len(xi), 6)) if P is None else P, dtype)
    pi, pj = P[:, 0:2], P[:, 3:5]
    tni, tnj = xi[:, :2] + _mv(rot2(xi[:, 2]), pi), xj[:, :2] + _mv(rot2(xj[:, 2]), pj)
    thni, thnj = xi[:, 2] + P[:, 2], xj[:, 2] + P[:, 5]
    RniT, RzT = _T(rot2(thni)), _T(rot2(z[:, 2]))
    d = tnj - tni
    e = np.concatenate([_mv(RzT, _mv(RniT, d) - z[:, :2]), wrap(thnj - thni - z[:, 2], dtype)[:, None]], 1)
    if not jac:
        return e
    n = len(e)
    Ji, Jj = np.zeros((n, 3, 3), dtype), np.zeros((n, 3, 3), dtype)
    Ji[:, :2, :2] = -RzT @ RniT
    Ji[:, :2, 2] = _mv(RzT, _mv(_T(_drot2(thni)), d) - _mv(RniT, _mv(_drot2(xi[:, 2]), pi)))
    Ji[:, 2, 2] = -1
    Jj[:, :2, :2] = RzT @ RniT
    Jj[:, :2, 2] = _mv(RzT @ RniT, _mv(_drot2(xj[:, 2]), pj))
    Jj[:, 2, 2] = 1
    return e, Ji, Jj


def bearing_edge(xi, l, z, dtype=np.float64, jac=True):
    """EdgeSE2PointXYBearing: e [n, 1], Ji [n, 1, 3], Jj [n, 1, 2]; z [n] or [n, 1]."""
    xi, l = _a(xi, dtype), _a(l, dtype)
    z = np.asarray(z, dtype).reshape(-1)
    RiT = _T(rot2(xi[:, 2]))
    d = _mv(RiT, l - xi[:, :2])
    e = wrap(z - np.arctan2(d[:, 1], d[:, 0]), dtype)[:, None]
    if not jac:
        return e
    g = np.stack([-d[:, 1], d[:, 0]], 1) / np.sum(d * d, 1, keepdims=True)
    gR = np.einsum("ni,nij->nj", g, RiT)
    Ji = np.concatenate([gR, np.ones((len(e), 1), dtype)], 1)[:, None, :]
    return e, Ji, -gR[:, None, :]


def batch(etype, xi, xj, meas, params=None, dtype=np.float64, jac=True):
    if etype == SE3O:
        return se3_offset_edge(xi, xj, meas, params, dtype, jac)
    if etype == SE2O:
        return se2_offset_edge(xi, xj, meas, params, dtype, jac)
    if etype == BEAR:
        return bearing_edge(xi, xj, meas, dtype, jac)
    raise KeyError(etype)


# ---------------------------------------------------------------- graphs
class Graph(unary_ref.Graph):
    """unary_ref.Graph with the three edges restated here and EdgeSE3 (pose_edges_ref.se3_edge)."""

    def edge(self, es, k, est=None, binary=None):
        if es.v1 is not None and (es.etype in KINDS or es.etype == synth.E_SE3_QUAT) and not (binary and es.etype in binary):
            i, j = int(es.v0[k]), int(es.v1[k])
            _, xi = self._est(est, i)
            _, xj = self._est(est, j)
            if es.etype == synth.E_SE3_QUAT:
                e, Ji, Jj = per.se3_edge(xi, xj, es.meas[k])
            else:
                e, Ji, Jj = batch(es.etype, xi, xj, es.meas[k], None if es.params is None else es.params[k])
            return e[0], [(i, Ji[0]), (j, Jj[0])]
        return super().edge(es, k, est, binary)

    def _rows(self, est, ids):
        vs = self.row[int(ids[0])][0]
        src = vs.est if est is None or vs.vtype not in est else np.asarray(est[vs.vtype])
        order = np.argsort(vs.ids)
        return src[order[np.searchsorted(vs.ids[order], ids)]]

    def payload(self, etype, est=None):
        """[e | Ji | Jj] row-major per edge of one of the three types: the records of the host-J set that holds them."""
        out = []
        for es in self.prob.edges:
            if es.etype == etype:
                e, Ji, Jj = batch(etype, self._rows(est, es.v0), self._rows(est, es.v1), es.meas, es.params)
                n = len(e)
                out.append(np.concatenate([e, Ji.reshape(n, -1), Jj.reshape(n, -1)], 1).ravel())
        return np.concatenate(out)

    def edge_chi2(self, etype, est=None, dtype=np.float64):
        """e^T Omega e of every edge of one type, in its order."""
        for es in self.prob.edges:
            if es.etype == etype:
                e = batch(etype, self._rows(est, es.v0), self._rows(est, es.v1), es.meas, es.params, dtype, False)
                return np.einsum("ni,nij,nj->n", e, np.asarray(es.info, dtype), e)
        raise KeyError(etype)

    def chi2_in(self, dtype, only=KINDS):
        """chi2 of the three types' edges at the problem's own estimates with every operation in dtype."""
        return sum((np.sum(self.edge_chi2(t, None, dtype)) for t in only
                    if any(es.etype == t for es in self.prob.edges)), dtype(0))


def numpy_stage(prob, lam=None, robust=None, est=None):
    """The dense system and its solve; lam None: LM's own first lambda, 1e-5 max diag(H) (a landmark seen through one
    or two bearings has a rank-deficient Hll: far under the scale of H the solve answers rounding with more than the
    stage tolerance)."""
    g = Graph(prob)
    H, b = g.dense_system(est=est, robust=robust)
    if lam is None:
        lam = 1e-5 * float(np.max(np.diag(H)))
    Hs, bs, x = unary_ref.solve(H, b, g.npose, lam, prob.landmark_dim)
    return dict(b=b, x=x, Hschur=Hs, bschur=bs, np=g.npose, n=g.n, lam=lam, H=H)


def hostj_problem(prob):
    return synth.offset_twin(prob)


# ---------------------------------------------------------------- structure-only over the bearing edges
def _edge_eval(ed, p, jac=True, dtype=np.float64):
    if ed.etype == BEAR:
        r = bearing_edge(ed.other, p, ed.meas, dtype, jac)
        if not jac:
            return r[0].astype(np.float64), None
        return r[0][0].astype(np.float64), r[2][0].astype(np.float64)
    return _edge_eval.base(ed, p, jac)


_edge_eval.base = structure_only_ref.edge_eval


@contextlib.contextmanager
def bearing_edges(dtype=np.float64):
    """structure_only_ref's calc with the bearing edge added to its edge table for the duration of a call."""
    structure_only_ref.edge_eval = lambda ed, p, jac=True: _edge_eval(ed, p, jac, dtype)
    try:
        yield
    finally:
        structure_only_ref.edge_eval = _edge_eval.base


class Structure(structure_only_ref.Structure):
    def calc(self, *a, dtype=np.float64, **kw):
        with bearing_edges(dtype):
            return super().calc(*a, **kw)

    def graph_chi2(self, est=None):
        return Graph(self.prob).chi2(est=est, robust=self.robust)


# ---------------------------------------------------------------- cases
def _iso_mul(Ra, ta, Rb, tb):
    return Ra @ Rb, ta + Ra @ tb


def _rand_pose(rng, scale=1.0):
    return per.axis_angle([rng.standard_normal(3)], [rng.uniform(0.3, 2.5)])[0], rng.uniform(-scale, scale, 3)


def _rand_offsets7(rng, n):
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return np.concatenate([rng.uniform(-0.5, 0.5, (n, 3)), q], 1)


def se3_branch_cases():
    """[(label, Xi, Xj, Z, P)]: the error rotation Z^-1 (Xi Pi)^-1 (Xj Pj) is pose_edges_ref's target of the label (the
    seven dq_dR labels, the pair at trace = +-1e-3, 'wneg': a measurement quaternion with w < 0 and norm 1.3), checked
    against its margins; both offsets are far from the identity."""
    rng = np.random.default_rng(5101)
    out = []
    for label, Te in per._targets():
        Ri, ti = _rand_pose(rng)
        qz = per.wneg_quat()[0] if label == "wneg" else per._unit(rng.standard_normal(4))
        Rz, tz = rot(qz)[0], rng.uniform(-1, 1, 3)
        P = _rand_offsets7(rng, 2)
        Rpi, Rpj = rot(P[:, 3:])
        te = rng.uniform(0.2, 0.5, 3) * np.array([1, -1, 1])
        Rn, tn = _iso_mul(Ri, ti, Rpi, P[0, :3])          # Ni
        Rn, tn = _iso_mul(Rn, tn, Rz, tz)                 # Ni Z
        Rn, tn = _iso_mul(Rn, tn, Te, te)                 # Nj = Ni Z E
        Rj, tj = _iso_mul(Rn, tn, Rpj.T, -Rpj.T @ P[1, :3])  # Xj = Nj Pj^-1
        per._check_margins(Te)
        out.append((label, per.pose_of(Ri, ti), per.pose_of(Rj, tj), np.concatenate([tz, qz]), P.ravel()))
    return out


def se2_wrap_cases():
    """[(label, xi, xj, z, P)]: vertex angles from SE2_ANGLES (on and outside the ends of [-pi, pi)), offset angles of
    either sign, the measurement angle such that the error angle is +-0.7 .. 1.2 after a wrap upward, downward or
    none."""
    rng = np.random.default_rng(5103)
    out = []
    pairs = [(0, 2), (2, 0), (1, 3), (3, 1), (2, 3), (3, 2)]
    for k, (a, b) in enumerate(pairs):
        thi, thj = SE2_ANGLES[a], SE2_ANGLES[b]
        P = np.array([*rng.uniform(-0.5, 0.5, 2), 2.0 * (-1) ** k, *rng.uniform(-0.5, 0.5, 2), -1.3 * (-1) ** (k // 2)])
        r = (0.7 + 0.1 * k) * (-1) ** k
        raw0 = (thj + P[5]) - (thi + P[2])
        thz = float(wrap(np.array(raw0 - r)))
        raw = raw0 - thz
        label = "up" if raw < -PI else ("down" if raw >= PI else "none")
        assert abs(float(wrap(np.array(raw)))) < PI - 0.3
        xi = np.array([*rng.uniform(-1, 1, 2), thi])
        xj = np.array([*(xi[:2] + rng.uniform(-1, 1, 2)), thj])
        out.append((label, xi, xj, np.array([*rng.uniform(-1, 1, 2), thz]), P))
    return out


def bearing_cut_cases():
    """[(label, xi, l, z)]: d = Ri^T (l - ti) in each quadrant, on the negative x axis on either side of the atan2 cut,
    and z - angle beyond +-pi (wrapped up / down); the pose angle cycles through SE2_ANGLES; |d| >= 1 everywhere."""
    rng = np.random.default_rng(5104)
    spec = [("q1", (2.0, 1.4), 0.3), ("q2", (-1.5, 2.0), -0.4), ("q3", (-2.0, -1.1), 0.5), ("q4", (1.2, -2.2), -0.25),
            ("cut+", (-2.0, 1e-3), -0.2), ("cut-", (-2.0, -1e-3), 0.2),
            ("up", (2 * np.cos(3.0), 2 * np.sin(3.0)), None), ("down", (2 * np.cos(-3.0), 2 * np.sin(-3.0)), None)]
    out = []
    for k, (label, d, dz) in enumerate(spec):
        d = np.array(d)
        assert np.linalg.norm(d) >= 1
        xi = np.array([*rng.uniform(-1, 1, 2), SE2_ANGLES[k % 4]])
        l = xi[:2] + rot2(xi[2]) @ d
        ang = np.arctan2(d[1], d[0])
        z = {"up": -3.0, "down": 3.0}.get(label, None)
        if z is None:
            z = float(wrap(np.array(ang + dz)))
        raw = z - ang
        if label == "up":
            assert raw < -PI
        if label == "down":
            assert raw >= PI
        out.append((label, xi, l, np.array([z])))
    return out


def one_edge(etype, case=None, seed=0):
    """Two free vertices and one edge of the type with a non-diagonal information matrix (bearing: one scalar), the
    landmark marginalized. case: an entry of the type's case table (default: its first)."""
    rng = np.random.default_rng(900 + etype + seed)
    if etype == SE3O:
        _, xi, xj, z, P = case or se3_branch_cases()[0]
        return synth.Problem("se3off_one", [_vs(synth.V_SE3_QUAT, [3, 8], [xi, xj])],
                             [_es(SE3O, [3], [8], z[None], _spd(rng, 6), P[None])], 6, 0)
    if etype == SE2O:
        _, xi, xj, z, P = case or se2_wrap_cases()[0]
        return synth.Problem("se2off_one", [_vs(synth.V_SE2, [2, 6], [xi, xj])],
                             [_es(SE2O, [2], [6], z[None], _spd(rng, 3), P[None])], 3, 0)
    _, xi, l, z = case or bearing_cut_cases()[0]
    return synth.Problem("bearing_one", [_vs(synth.V_SE2, [4], [xi]), _vs(synth.V_XY, [9], [l], marg=1)],
                         [_es(BEAR, [4], [9], z[None], np.array([[[37.0 + seed]]]))], 3, 2)


def edge_case(etype, ne, uniform=False):
    """Exactly ne edges of one type.
    Offset types: pose_edges_ref's anchored chain (ne + 1 poses, every 8th fixed, the SE3 errors cycling through the
    dq_dR branches, the SE2 angles through SE2_ANGLES) with each edge's measurement moved to the sensor frames,
    Z' = Pi^-1 Z Pj, so that the error keeps its size. uniform: one parameter record and one information matrix for
    every edge (EdgeData::ue bits 1 and 0), else all distinct.
    Bearing: min(ne, 9) poses on a circle of radius 6 around (ne + 2) // 3 landmarks within radius 2, each landmark seen
    from up to three neighbouring poses; EdgeSE2 odometry ties the poses, the first is fixed; landmarks marginalized.
    uniform: one information scalar for every bearing."""
    rng = np.random.default_rng(6000 + 10 * ne + etype)
    if etype in OFFSETS:
        base, _ = (per.se3_chain if etype == SE3O else per.se2_chain)(ne)
        es = base.edges[0]
        if etype == SE3O:
            P = _rand_offsets7(rng, 2 if uniform else 2 * ne).reshape(-1, 14)
            P = np.broadcast_to(P, (ne, 14)).copy()
            meas = []
            for k in range(ne):
                Rz, tz = rot(es.meas[k, 3:])[0], es.meas[k, :3]
                Rpi, Rpj = rot(P[k].reshape(2, 7)[:, 3:])
                R, t = _iso_mul(Rpi.T, -Rpi.T @ P[k, 0:3], Rz, tz)
                R, t = _iso_mul(R, t, Rpj, P[k, 7:10])
                meas.append(per.pose_of(R, t))
            meas = np.array(meas)
        else:
            P = np.concatenate([rng.uniform(-0.5, 0.5, (ne, 2)), rng.uniform(-2, 2, (ne, 1)),
                                rng.uniform(-0.5, 0.5, (ne, 2)), rng.uniform(-2, 2, (ne, 1))], 1)
            if uniform:
                P = np.broadcast_to(P[:1], (ne, 6)).copy()
            inv_i = np.array([unary_ref.se2_inv(p) for p in P[:, :3]])
            meas = np.array([unary_ref.se2_mul(unary_ref.se2_mul(a, z), pj) for a, z, pj in zip(inv_i, es.meas, P[:, 3:])])
        info = np.broadcast_to(es.info[:1], es.info.shape).copy() if uniform else es.info
        return synth.Problem(f"{base.name}/off{int(uniform)}", base.vertices, [_es(etype, es.v0, es.v1, meas, info, P)],
                             base.pose_dim, 0)
    npose = 1 if ne == 1 else min(max(ne, 3), 9)
    th = 2 * np.pi * np.arange(npose) / 9
    poses = np.stack([6 * np.cos(th), 6 * np.sin(th), [SE2_ANGLES[p % 4] for p in range(npose)]], 1)
    nl = (ne + 2) // 3
    rad, ang = 2 * np.sqrt(rng.random(nl)), 2 * np.pi * rng.random(nl)
    lms = np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
    v0 = np.array([(k + k // 3) % npose for k in range(ne)])
    v1 = npose + np.arange(ne) // 3
    z = wrap(-bearing_edge(poses[v0], lms[v1 - npose], np.zeros(ne), jac=False)[:, 0] + 0.05 * rng.standard_normal(ne))
    w = np.full(ne, 400.0) if uniform else 400.0 * (1 + rng.random(ne))
    fx = np.zeros(npose, np.int32)
    fx[0] = ne > 1
    edges = [_es(BEAR, v0, v1, z[:, None], w[:, None, None])]
    if npose > 1:
        a = np.arange(npose - 1)
        zo = per.se2_edge(poses[a], poses[a + 1], np.zeros((npose - 1, 3)), jac=False) + 0.02 * rng.standard_normal((npose - 1, 3))
        edges.append(_es(synth.E_SE2, a, a + 1, zo, _spd(rng, 3, npose - 1) * 100.0))
    return synth.Problem(f"bearing_fan{ne}u{int(uniform)}", [_vs(synth.V_SE2, np.arange(npose), poses, fx),
                                                             _vs(synth.V_XY, npose + np.arange(nl), lms, marg=1)],
                         edges, 3, 2)


def identity_chain(etype, ne=24):
    """(the chain entered as the offset type with params None, the same chain as EdgeSE3 / EdgeSE2)."""
    base, _ = (per.se3_chain if etype == SE3O else per.se2_chain)(ne)
    es = base.edges[0]
    off = synth.Problem(base.name + "/ident", base.vertices, [_es(etype, es.v0, es.v1, es.meas, es.info, None)],
                        base.pose_dim, 0)
    return off, base


def per_edge_scene():
    """synth.bearing_scene() for the per-edge chi2 comparison: a bearing's error is one scalar, the difference of two
    angles of order one, so a residual that happens to fall near zero has no relative precision in float64 (2 eps pi / |e|
    of its chi2). Measurements whose residual at the start is under 0.02 rad are moved so that it is +-0.02."""
    prob = synth.bearing_scene()
    poses, lms = prob.vertices
    es = prob.edges[1]
    e = bearing_edge(poses.est[es.v0], lms.est[es.v1 - lms.ids[0]], es.meas, jac=False)[:, 0]
    small = np.abs(e) < 0.02
    z = es.meas[:, 0].copy()
    z[small] = wrap(z[small] + np.where(e[small] < 0, -0.02, 0.02) - e[small])
    edges = [prob.edges[0], _es(BEAR, es.v0, es.v1, z[:, None], es.info)]
    return synth.Problem(prob.name + "/clear", prob.vertices, edges, 3, 2)


def tracks_problem(lengths=(2, 7, 8, 9, 65), prior=False, seed=5):
    """One landmark per track length, each seen by that many poses of a ring of max(lengths) poses of radius 6 around
    the landmarks (within radius 2), the poses of a track spread evenly over the ring (parallax); the first pose fixed;
    the landmarks start 0.1 to 0.25 off. prior: an EdgeXYPrior on every landmark beside its bearings. The structure-only
    kernel walks a landmark's edges with eight lanes."""
    rng = np.random.default_rng(seed + 77)
    C = max(lengths)
    th = 2 * np.pi * np.arange(C) / C
    poses = np.stack([6 * np.cos(th), 6 * np.sin(th), wrap(th + np.pi + 0.3 * rng.standard_normal(C))], 1)
    L = len(lengths)
    rad, ang = 2 * np.sqrt(rng.random(L)), 2 * np.pi * rng.random(L)
    truth = np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
    pose_ids, lm_ids = np.arange(C, dtype=np.int32), (1000 + np.arange(L)).astype(np.int32)
    v0 = np.concatenate([(rng.integers(0, C) + np.floor(np.arange(n) * C / n).astype(np.int64)) % C for n in lengths])
    v1 = np.concatenate([np.full(n, lm_ids[i]) for i, n in enumerate(lengths)])
    lidx = np.concatenate([np.full(n, i) for i, n in enumerate(lengths)])
    z = wrap(-bearing_edge(poses[v0], truth[lidx], np.zeros(len(v0)), jac=False)[:, 0] + 0.01 * rng.standard_normal(len(v0)))
    start = truth + rng.choice([-1.0, 1.0], truth.shape) * (0.1 + 0.15 * rng.random(truth.shape))
    edges = [_es(BEAR, v0, v1, z[:, None], np.full((len(v0), 1, 1), 100.0))]
    if prior:
        edges.append(_es(synth.E_XY_PRIOR, lm_ids, None, truth + 0.05 * rng.standard_normal(truth.shape),
                         np.broadcast_to(4.0 * np.eye(2), (L, 2, 2)).copy()))
    return synth.Problem(f"bearing_tracks{'p' if prior else ''}",
                         [_vs(synth.V_SE2, pose_ids, poses, (pose_ids == 0).astype(np.int32)),
                          _vs(synth.V_XY, lm_ids, start, marg=1)], edges, 3, 2)
