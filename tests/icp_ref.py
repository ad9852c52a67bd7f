"""Plain-numpy restatement of the types_icp edges (test reference; written from types_icp.h / types_icp.cpp and the
maths, nothing here comes from the library).

  Edge_V_V_GICP  e = R0^T (R1 pos1 + t1 - t0) - pos0                         (types_icp.h:177-227)
                 plane-to-plane: Omega = (cov0 + R01 cov1 R01^T)^-1, R01 = R0^T R1, at the current state
  Edge_XYZ_VSC   pc = R^T (pt - t); e = (fx x/z + cx - u, fy y/z + cy - v, fx (x - b)/z + cx - u_r)   (:340-402)

Jacobians. VertexSE3's oplus is X * (dt, dq): R <- R (I + 2 [dq]x), t <- t + R dt.
  GICP, moving T0: T0^-1 -> (dt, dq)^-1 T0^-1, so p -> (I - 2 [dq]x)(p - dt): Ji = [-I | 2 [p1t]x], p1t = T0^-1 T1 pos1.
  This is the reference's [-I | dRidx p1t, dRidy p1t, dRidz p1t]: dRid{x,y,z} (types_icp.cpp:49-57) are the columns
  of the map p -> 2 [p]x.
        moving T1: pos1 -> (I + 2 [dq]x) pos1 + dt: Jj = [R01 | -2 R01 [pos1]x] = [R01 | R01 dRid{x,y,z}^T pos1].
  VSC: with P = d proj / d pc, A = P R^T (the point) and B = P [-I | 2 [pc]x] (the camera, as Ji above). The reference
  has no analytic Jacobian for this edge (SCAM_ANALYTIC_JACOBIANS is commented out); these are the exact ones.

Every edge function takes batches and a dtype; np.longdouble is the high-precision mode. Graph plugs the two types
into unary_ref.Graph (hessian order, priors), with a vectorised chi2 / dense system over the two types' sets (the
graphs of tests/test_gpu_icp.py hold thousands of edges).
"""
import contextlib

import numpy as np

import structure_only_ref
import unary_ref
from g2o_amd import synth
from pose_edges_ref import _T, _a, _mv, rot, skew

GICP, VSC = synth.E_V_V_GICP, synth.E_XYZ_VSC
KINDS = (GICP, VSC)
HOSTJ3 = 32 + 3
KCAM = np.array([150.0, 150.0, 320.0, 240.0, 0.075])


def unpack(c, dtype=np.float64):
    """[n, 6] packed upper triangles 00 01 11 02 12 22 -> [n, 3, 3] symmetric."""
    c = _a(c, dtype)
    M = np.empty((len(c), 3, 3), dtype)
    M[:, 0, 0], M[:, 0, 1], M[:, 1, 1], M[:, 0, 2], M[:, 1, 2], M[:, 2, 2] = c.T
    M[:, 1, 0], M[:, 2, 0], M[:, 2, 1] = M[:, 0, 1], M[:, 0, 2], M[:, 1, 2]
    return M


def gicp_edge(x0, x1, meas, dtype=np.float64, jac=True, assoc=0):
    """Edge_V_V_GICP: e [n, 3] and, with jac, Ji, Jj [n, 3, 6]. x0, x1 [n, 7] (t, q as given), meas [n, 12].
    assoc: 0 the reference's T0^-1 (T1 pos1), 1 (T0^-1 T1) pos1, 2 R0^T ((R1 pos1 + t1) - t0)."""
    x0, x1, m = _a(x0, dtype), _a(x1, dtype), _a(meas, dtype)
    R0, R1 = rot(x0[:, 3:], dtype, False), rot(x1[:, 3:], dtype, False)
    t0, t1, p0, p1 = x0[:, :3], x1[:, :3], m[:, 0:3], m[:, 6:9]
    R01, t01 = _T(R0) @ R1, _mv(_T(R0), t1 - t0)
    if assoc == 0:
        pt = _mv(_T(R0), _mv(R1, p1) + t1) + (-_mv(_T(R0), t0))
    elif assoc == 1:
        pt = _mv(R01, p1) + t01
    else:
        pt = _mv(_T(R0), (_mv(R1, p1) + t1) - t0)
    e = pt - p0
    if not jac:
        return e
    n = len(e)
    Ji, Jj = np.zeros((n, 3, 6), dtype), np.zeros((n, 3, 6), dtype)
    p1t = _mv(R01, p1) + t01
    Ji[:, :, :3], Ji[:, :, 3:] = -np.eye(3, dtype=dtype), 2 * skew(p1t)
    Jj[:, :, :3], Jj[:, :, 3:] = R01, -2 * R01 @ skew(p1)
    return e, Ji, Jj


def gicp_omega(x0, x1, info, params, dtype=np.float64):
    """The information of each edge [n, 3, 3]: the caller's (params None), or (cov0 + R01 cov1 R01^T)^-1."""
    if params is None:
        return _a(info, dtype)
    x0, x1 = _a(x0, dtype), _a(x1, dtype)
    R01 = _T(rot(x0[:, 3:], dtype, False)) @ rot(x1[:, 3:], dtype, False)
    P = _a(params, dtype)
    S = unpack(P[:, :6], dtype) + R01 @ unpack(P[:, 6:], dtype) @ _T(R01)
    if dtype == np.longdouble:  # numpy's inv has no long double: adjugate over determinant
        out = np.empty_like(S)
        for r in range(3):
            for c in range(3):
                i, j = [k for k in range(3) if k != c], [k for k in range(3) if k != r]  # cofactor (c, r)
                out[:, r, c] = (-1) ** (r + c) * (S[:, i[0], j[0]] * S[:, i[1], j[1]] - S[:, i[0], j[1]] * S[:, i[1], j[0]])
        det = S[:, 0, 0] * out[:, 0, 0] + S[:, 0, 1] * out[:, 1, 0] + S[:, 0, 2] * out[:, 2, 0]
        return out / det[:, None, None]
    return np.linalg.inv(S)


def vsc_edge(pt, x, meas, K, dtype=np.float64, jac=True):
    """Edge_XYZ_VSC: e [n, 3], Ji [n, 3, 3] (the point), Jj [n, 3, 6] (the camera). K [n, 5] fx fy cx cy baseline."""
    pt, x, m, K = _a(pt, dtype), _a(x, dtype), _a(meas, dtype), _a(K, dtype)
    R = rot(x[:, 3:], dtype, False)
    pc = _mv(_T(R), pt - x[:, :3])
    fx, fy, cx, cy, bl = K.T
    X, Y, Z = pc.T
    e = np.stack([fx * X / Z + cx, fy * Y / Z + cy, fx * (X - bl) / Z + cx], 1) - m
    if not jac:
        return e
    n = len(e)
    P = np.zeros((n, 3, 3), dtype)
    P[:, 0, 0], P[:, 0, 2] = fx / Z, -fx * X / Z ** 2
    P[:, 1, 1], P[:, 1, 2] = fy / Z, -fy * Y / Z ** 2
    P[:, 2, 0], P[:, 2, 2] = fx / Z, -fx * (X - bl) / Z ** 2
    Jj = np.zeros((n, 3, 6), dtype)
    Jj[:, :, :3], Jj[:, :, 3:] = -P, 2 * P @ skew(pc)
    return e, P @ _T(R), Jj


def _rho(kind, delta, e2):
    """Vectorised unary_ref.robustify: (rho, rho') of squared errors e2 [n]."""
    out = [unary_ref.robustify(kind, delta, float(v)) for v in e2]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


# ---------------------------------------------------------------- graphs
class Graph(unary_ref.Graph):
    """unary_ref.Graph with the two edges restated here. levels: {edge type: int array}, edges off level 0 are left
    out (a handle initialised at level 0)."""

    def __init__(self, prob, levels=None):
        super().__init__(prob)
        self.levels = levels or {}
        if levels:  # the hessian order holds the vertices that have an edge at the level
            has = set()
            for es in prob.edges:
                on = self._on(es)
                has.update(int(i) for i in es.v0[on])
                if es.v1 is not None:
                    has.update(int(i) for i in es.v1[on])
            free = [(int(vs.marginalized[k]), i) for i, (vs, k) in self.row.items() if i in has and not vs.fixed[k]]
            self.order = [i for _, i in sorted(free)]
            self.off, o = {}, 0
            for i in self.order:
                self.off[i] = o
                o += unary_ref.V_DIM[self.row[i][0].vtype]
            self.n = o
            self.npose = sum(unary_ref.V_DIM[self.row[i][0].vtype] for i in self.order
                             if not self.row[i][0].marginalized[self.row[i][1]])

    def _on(self, es):
        lv = self.levels.get(es.etype)
        return np.ones(len(es.v0), bool) if lv is None else np.asarray(lv) == 0

    def _rows(self, est, ids):
        vs = self.row[int(ids[0])][0]
        src = vs.est if est is None or vs.vtype not in est else np.asarray(est[vs.vtype])
        order = np.argsort(vs.ids)
        return src[order[np.searchsorted(vs.ids[order], ids)]]

    def terms(self, es, est=None, dtype=np.float64, jac=True):
        """(e, Ji, Jj, Omega) of every edge of a GICP or VSC set."""
        xi, xj = self._rows(est, es.v0), self._rows(est, es.v1)
        if es.etype == GICP:
            r = gicp_edge(xi, xj, es.meas, dtype, jac)
            Om = gicp_omega(xi, xj, es.info, es.params, dtype)
        else:
            r = vsc_edge(xi, xj, es.meas, es.params, dtype, jac)
            Om = _a(es.info, dtype)
        return (r + (Om,)) if jac else (r, None, None, Om)

    def edge_chi2(self, etype, est=None, dtype=np.float64):
        """e^T Omega e of every edge of one type, in the order of its sets."""
        out = []
        for es in self.prob.edges:
            if es.etype == etype:
                e, _, _, Om = self.terms(es, est, dtype, False)
                out.append(np.einsum("ni,nij,nj->n", e, Om, e))
        return np.concatenate(out)

    def chi2(self, est=None, robust=None, binary=None, only=None):
        c = 0.0
        for es in self.prob.edges:
            if only is not None and es.etype not in only:
                continue
            if es.etype not in KINDS:
                sub = synth.Problem("one", self.prob.vertices, [es], self.prob.pose_dim, self.prob.landmark_dim)
                c += unary_ref.Graph(sub).chi2(est, robust, binary)
                continue
            e, _, _, Om = self.terms(es, est, jac=False)
            e2 = np.einsum("ni,nij,nj->n", e, Om, e)[self._on(es)]
            kind, delta = (robust or {}).get(es.etype, (None, 1.0))
            c += float(np.sum(e2 if kind in (None, "none") else _rho(kind, delta, e2)[0]))
        return c

    def dense_system(self, est=None, robust=None, binary=None):
        H, b = np.zeros((self.n, self.n)), np.zeros(self.n)
        rest = [es for es in self.prob.edges if es.etype not in KINDS]
        if rest:  # the other sets through unary_ref, in this graph's hessian order
            g = unary_ref.Graph(synth.Problem("rest", self.prob.vertices, rest, self.prob.pose_dim, self.prob.landmark_dim))
            g.order, g.off, g.n, g.npose = self.order, self.off, self.n, self.npose
            H, b = g.dense_system(est, robust, binary)
        for es in self.prob.edges:
            if es.etype not in KINDS:
                continue
            e, Ji, Jj, Om = self.terms(es, est)
            kind, delta = (robust or {}).get(es.etype, (None, 1.0))
            if kind not in (None, "none"):
                Om = Om * _rho(kind, delta, np.einsum("ni,nij,nj->n", e, Om, e))[1][:, None, None]
            on = self._on(es)
            sides = [(es.v0, Ji), (es.v1, Jj)]
            for ia, Ja in sides:
                oa = np.array([self.off.get(int(i), -1) for i in ia])
                ba = -np.einsum("nia,nij,nj->na", Ja, Om, e)
                for ib, Jb in sides:
                    ob = np.array([self.off.get(int(i), -1) for i in ib])
                    Hab = np.einsum("nia,nij,njb->nab", Ja, Om, Jb)
                    for u in {(x, y) for x, y, k in zip(oa, ob, on) if x >= 0 and y >= 0 and k}:
                        sel = (oa == u[0]) & (ob == u[1]) & on
                        da, db = Hab.shape[1], Hab.shape[2]
                        H[u[0]:u[0] + da, u[1]:u[1] + db] += Hab[sel].sum(0)
                for u in {x for x, k in zip(oa, on) if x >= 0 and k}:
                    b[u:u + ba.shape[1]] += ba[(oa == u) & on].sum(0)
        return H, b

    def payload(self, est=None):
        """The records of the twin's E_HOSTJ(3) set, every GICP / VSC set in the problem's order: [e | Ji | Jj]
        row-major per edge; a plane-to-plane set whitened, [L^T e | L^T Ji | L^T Jj] with Omega = L L^T."""
        out = []
        for es in self.prob.edges:
            if es.etype in KINDS:
                e, Ji, Jj, Om = self.terms(es, est)
                if es.etype == GICP and es.params is not None:
                    Lt = _T(np.linalg.cholesky(Om))
                    e, Ji, Jj = _mv(Lt, e), Lt @ Ji, Lt @ Jj
                n = len(e)
                out.append(np.concatenate([e, Ji.reshape(n, -1), Jj.reshape(n, -1)], 1).ravel())
        return np.concatenate(out)


def numpy_stage(prob, lam=None, robust=None, est=None, levels=None):
    """The dense system and its solve; lam None: LM's own first lambda, 1e-5 max diag(H)."""
    g = Graph(prob, levels)
    H, b = g.dense_system(est=est, robust=robust)
    if lam is None:
        lam = 1e-5 * float(np.max(np.diag(H)))
    Hs, bs, x = unary_ref.solve(H, b, g.npose, lam, prob.landmark_dim)
    return dict(b=b, x=x, Hschur=Hs, bschur=bs, np=g.npose, n=g.n, lam=lam, H=H)


def hostj_problem(prob):
    return synth.icp_twin(prob)


# ---------------------------------------------------------------- structure-only over the VSC edges
def _edge_eval(ed, p, jac=True):
    if ed.etype == VSC:
        r = vsc_edge(np.asarray(p)[None], ed.other[None], ed.meas[None], ed.params[None], jac=jac)
        return (r[0][0], r[1][0]) if jac else (r[0], None)
    return _edge_eval.base(ed, p, jac)


_edge_eval.base = structure_only_ref.edge_eval


@contextlib.contextmanager
def vsc_edges():
    """structure_only_ref's calc with Edge_XYZ_VSC added to its edge table for the duration of a call."""
    structure_only_ref.edge_eval = _edge_eval
    try:
        yield
    finally:
        structure_only_ref.edge_eval = _edge_eval.base


class Structure(structure_only_ref.Structure):
    def calc(self, *a, **kw):
        with vsc_edges():
            return super().calc(*a, **kw)

    def graph_chi2(self, est=None):
        return Graph(self.prob).chi2(est=est, robust=self.robust)


# ---------------------------------------------------------------- small cases
def _rand_pose(rng, scale=1.0):
    q = rng.standard_normal(4)
    q /= np.linalg.norm(q)
    return np.concatenate([rng.standard_normal(3) * scale, q if q[3] >= 0 else -q])


def _spd3(rng, n):
    A = np.eye(3) + 0.3 * rng.standard_normal((n, 3, 3))
    return np.einsum("nij,nkj->nik", A, A)


def gicp_case(n, pl_pl=False, seed=0):
    """n random Edge_V_V_GICP edges between two random poses, as the edge functions' inputs: (x0, x1, meas, info, params)."""
    rng = np.random.default_rng(100 + seed)
    x0, x1 = np.tile(_rand_pose(rng), (n, 1)), np.tile(_rand_pose(rng), (n, 1))
    nm = rng.standard_normal((n, 2, 3))
    nm /= np.linalg.norm(nm, axis=2, keepdims=True)
    meas = np.concatenate([rng.standard_normal((n, 3)), nm[:, 0], rng.standard_normal((n, 3)), nm[:, 1]], 1)
    info = np.stack([synth.gicp_prec(v, 0.01) for v in nm[:, 0]])
    params = None
    if pl_pl:
        params = np.concatenate([synth.gicp_pack([synth.gicp_cov(v, 0.01) for v in nm[:, 0]]),
                                 synth.gicp_pack([synth.gicp_cov(v, 0.01) for v in nm[:, 1]])], 1)
    return x0, x1, meas, info, params


def vsc_case(n, seed=0):
    """n random Edge_XYZ_VSC edges: points 8..12 in front of a slightly rotated camera: (pt, x, meas, K, info)."""
    rng = np.random.default_rng(200 + seed)
    q = np.concatenate([0.1 * rng.standard_normal(3), [1.0]])
    x = np.tile(np.concatenate([0.2 * rng.standard_normal(3), q / np.linalg.norm(q)]), (n, 1))
    pt = np.stack([(rng.random(n) - 0.5) * 3, rng.random(n) - 0.5, 8 + 4 * rng.random(n)], 1)
    K = np.tile(KCAM, (n, 1))
    meas = vsc_edge(pt, x, np.zeros((n, 3)), K, jac=False) + rng.standard_normal((n, 3))
    return pt, x, meas, K, _spd3(rng, n)


def one_edge(etype, pl_pl=False, seed=0, free="cam"):
    """A one-edge problem: GICP between a fixed and a free pose; VSC between a point and a camera of which ``free``
    ("cam" or "point") is free and the other fixed (the engine takes one pose block size per graph)."""
    if etype == GICP:
        x0, x1, meas, info, params = gicp_case(1, pl_pl, seed)
        verts = synth.VertexSet(synth.V_SE3_QUAT, np.array([0, 1], np.int32), np.stack([x0[0], x1[0]]),
                                np.array([1, 0], np.int32), np.zeros(2, np.int32))
        es = synth.EdgeSet(GICP, np.array([0], np.int32), np.array([1], np.int32), meas, None if pl_pl else info, params)
        return synth.Problem("one_gicp", [verts], [es], 6, 0)
    pt, x, meas, K, info = vsc_case(1, seed)
    fc, fp = np.array([int(free != "cam")], np.int32), np.array([int(free != "point")], np.int32)
    cams = synth.VertexSet(synth.V_SE3_QUAT, np.array([0], np.int32), x[:1], fc, np.zeros(1, np.int32))
    pts = synth.VertexSet(synth.V_XYZ, np.array([1], np.int32), pt[:1], fp, np.zeros(1, np.int32))
    es = synth.EdgeSet(VSC, np.array([1], np.int32), np.array([0], np.int32), meas, info, K)
    return synth.Problem("one_vsc_" + free, [cams, pts], [es], 6 if free == "cam" else 3, 0)
