"""Plain-numpy restatement of the "Bundle Adjustment in the Large" types of examples/bal/bal_example.cpp (test
reference; nothing here is taken from the library).

  VertexCameraBAL     9 doubles rx ry rz tx ty tz f k1 k2 (angle-axis, world to camera), oplus +=  (:59-95)
  VertexPointBAL      3 doubles, oplus +=                                                          (:102-132)
  EdgeObservationBAL  v0 the camera, v1 the point, measurement u v                                 (:156-281)

  error     with w = cam[0:3], th = sqrt(w.w): P = X cos th + (v x X) sin th + v (v.X)(1 - cos th), v = w / th, for
            th > 0; P = X + w x X for th == 0 exactly; P += t; p = -P.xy / P.z; r2 = p.p; rp = 1 + k1 r2 + k2 r2 r2;
            e = f rp p - z, in the reference's operation order (:191-244).
  Jacobians the reference differentiates that function with ceres autodiff (:254-280): the exact first derivatives of
            the expression as written, per branch. Here by hand: dE = f (rp I + (2 k1 + 4 k2 r2) p p^T),
            dp/dP = [[-1/Pz, 0, Px/Pz^2], [0, -1/Pz, Py/Pz^2]], M = dE dp/dP,
              Ji = [ M dP/dw | M | rp p | f r2 p | f r2^2 p ],   Jj = M dP/dX,
            dP/dX the Rodrigues matrix of the branch (th == 0: I + [w]x), dP/dw = -[X]x at th == 0 and for th > 0 the
            sum of the derivatives of the three terms through th, v, sin and cos: dth/dw_k = v_k,
            dv/dw_k = (e_k - v v_k) / th. What makes this a reference is tests/test_bal_host.py, which pins it against
            central differences in longdouble.

Graph plugs the type into unary_ref.Graph's dense system; Dense evaluates a problem in a dtype for lm() / gn() and
dogleg_ref.Dogleg; bal_text / parse_bal are the text format of bal_example.cpp:336-406.
"""
import numpy as np

import sim3_ref
import unary_ref
from pose_edges_ref import LD, _a, _es, _spd, _vs
from g2o_amd import synth

V_CAM, V_XYZ, E = 8, synth.V_XYZ, 30  # G2OHIP_V_CAM_BAL, G2OHIP_V_XYZ, G2OHIP_E_OBSERVATION_BAL
unary_ref.V_DIM.setdefault(V_CAM, 9)
HUBER = ("Huber", 4.0)  # delta^2 = 16: between the 3 - 6 px residuals' squares (9 .. 36) under identity information


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def _skew(v):
    z = np.zeros(len(v), v.dtype)
    return np.stack([np.stack([z, -v[:, 2], v[:, 1]], 1), np.stack([v[:, 2], z, -v[:, 0]], 1),
                     np.stack([-v[:, 1], v[:, 0], z], 1)], 1)


def rotate(w, X, dtype=np.float64, jac=False):
    """P [n, 3] before the translation; with jac also dP/dw and dP/dX [n, 3, 3]. Each row takes its own branch."""
    w, X = _a(w, dtype), _a(X, dtype)
    n = len(w)
    th = np.sqrt(w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1] + w[:, 2] * w[:, 2])
    big = th > 0
    P = np.zeros((n, 3), dtype)
    dPw, dPX = np.zeros((n, 3, 3), dtype), np.zeros((n, 3, 3), dtype)
    if big.any():
        wb, Xb, t = w[big], X[big], th[big][:, None]
        v = wb / t
        c, s = np.cos(t), np.sin(t)
        vX = _cross(v, Xb)
        vd = np.sum(v * Xb, 1)[:, None]
        omc = 1 - c
        P[big] = Xb * c + vX * s + v * vd * omc
        if jac:
            d = np.zeros((len(wb), 3, 3), dtype)
            for k in range(3):
                ek = np.zeros(3, dtype)
                ek[k] = 1
                vk = v[:, k:k + 1]
                dv = (ek[None] - v * vk) / t
                dvX = _cross(dv, Xb)
                dvd = np.sum(dv * Xb, 1)[:, None]
                dc, ds = -s * vk, c * vk
                d[:, :, k] = Xb * dc + dvX * s + vX * ds + dv * vd * omc + v * dvd * omc - v * vd * dc
            dPw[big] = d
            eye = np.eye(3, dtype=dtype)[None]
            dPX[big] = c[:, :, None] * eye + s[:, :, None] * _skew(v) + omc[:, :, None] * (v[:, :, None] * v[:, None, :])
    if (~big).any():
        wz, Xz = w[~big], X[~big]
        P[~big] = Xz + _cross(wz, Xz)
        if jac:
            dPw[~big] = -_skew(Xz)
            dPX[~big] = np.eye(3, dtype=dtype)[None] + _skew(wz)
    return (P, dPw, dPX) if jac else P


def error(cam, X, z, dtype=np.float64):
    """[n, 2] from cameras [n, 9], points [n, 3] and observations [n, 2]."""
    cam, X, z = _a(cam, dtype), _a(X, dtype), _a(z, dtype)
    P = rotate(cam[:, :3], X, dtype) + cam[:, 3:6]
    p = -P[:, :2] / P[:, 2:3]
    r2 = p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]
    rp = 1 + cam[:, 7] * r2 + cam[:, 8] * r2 * r2
    return (cam[:, 6] * rp)[:, None] * p - z


def jacobians(cam, X, dtype=np.float64):
    """The analytic Ji [n, 2, 9] and Jj [n, 2, 3] of the docstring."""
    cam, X = _a(cam, dtype), _a(X, dtype)
    n = len(cam)
    P, dPw, dPX = rotate(cam[:, :3], X, dtype, True)
    P = P + cam[:, 3:6]
    p = -P[:, :2] / P[:, 2:3]
    r2 = p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]
    f, k1, k2 = cam[:, 6], cam[:, 7], cam[:, 8]
    rp = 1 + k1 * r2 + k2 * r2 * r2
    g = 2 * k1 + 4 * k2 * r2
    dE = f[:, None, None] * (rp[:, None, None] * np.eye(2, dtype=dtype)[None] + g[:, None, None] * (p[:, :, None] * p[:, None, :]))
    iz = 1 / P[:, 2]
    dp = np.zeros((n, 2, 3), dtype)
    dp[:, 0, 0] = dp[:, 1, 1] = -iz
    dp[:, 0, 2], dp[:, 1, 2] = P[:, 0] * iz * iz, P[:, 1] * iz * iz
    M = dE @ dp
    Ji = np.concatenate([M @ dPw, M, (rp[:, None] * p)[:, :, None], ((f * r2)[:, None] * p)[:, :, None],
                         ((f * r2 * r2)[:, None] * p)[:, :, None]], 2)
    return Ji, M @ dPX


def records(cam, X, z, dtype=np.float64):
    """[e | Ji | Jj] row-major per edge."""
    e = error(cam, X, z, dtype)
    Ji, Jj = jacobians(cam, X, dtype)
    return np.concatenate([e, Ji.reshape(len(e), -1), Jj.reshape(len(e), -1)], 1)


# ---------------------------------------------------------------- graphs
class Graph(unary_ref.Graph):
    """unary_ref.Graph with EdgeObservationBAL restated here."""

    def edge(self, es, k, est=None, binary=None):
        if es.etype == E:
            i, j = int(es.v0[k]), int(es.v1[k])
            rec = records(self._est(est, i)[1][None], self._est(est, j)[1][None], es.meas[k][None])[0]
            return rec[:2], [(i, rec[2:20].reshape(2, 9)), (j, rec[20:].reshape(2, 3))]
        return super().edge(es, k, est, binary)

    def _rows(self, est, ids):
        vs = self.row[int(ids[0])][0]
        src = vs.est if est is None or vs.vtype not in est else np.asarray(est[vs.vtype])
        order = np.argsort(vs.ids)
        return src[order[np.searchsorted(vs.ids[order], ids)]]

    def sets(self):
        return [es for es in self.prob.edges if es.etype == E]

    def edge_chi2(self, est=None, dtype=np.float64):
        """e^T Omega e of every EdgeObservationBAL, in order."""
        out = []
        for es in self.sets():
            e = error(self._rows(est, es.v0), self._rows(est, es.v1), es.meas, dtype)
            out.append(np.einsum("ni,nij,nj->n", e, np.asarray(es.info, dtype), e))
        return np.concatenate(out)

    def chi2_in(self, dtype, est=None, robust=None):
        """The (robustified) chi2 in a dtype; robust (kind, delta)."""
        c = self.edge_chi2(est, dtype)
        if robust:
            c = np.array([unary_ref.robustify(robust[0], dtype(robust[1]), x)[0] for x in c], dtype)
        return np.sum(c)


def numpy_stage(prob, lam=None, robust=None, est=None):
    """The dense system and its solve; lam None: LM's own first lambda, 1e-5 max diag(H). robust (kind, delta)."""
    g = Graph(prob)
    H, b = g.dense_system(est=est, robust={E: robust} if robust else None)
    if lam is None:
        lam = 1e-5 * float(np.max(np.diag(H)))
    Hs, bs, x = unary_ref.solve(H, b, g.npose, lam, prob.landmark_dim)
    return dict(b=b, x=x, Hschur=Hs, bschur=bs, np=g.npose, n=g.n, lam=lam, H=H)


def without(prob, drop):
    """The problem without the observations drop[k] != 0: what a level leaves active."""
    (es,) = prob.edges
    keep = np.asarray(drop) == 0
    return synth.Problem(prob.name + "/kept", list(prob.vertices),
                         [_es(E, es.v0[keep], es.v1[keep], es.meas[keep], es.info[keep])], prob.pose_dim, prob.landmark_dim)


# ---------------------------------------------------------------- optimizers over the dense system, in a dtype
class Dense:
    """A BAL problem (one camera set, one point set, one observation set) evaluated in a dtype, with the calls lm(), gn()
    and dogleg_ref.Dogleg make. The full system (poses, then landmarks) is solved without forming the Schur complement:
    the same x. robust: (kind, delta) or None."""

    def __init__(self, prob, dtype=np.float64, robust=None, est=None):
        self.prob, self.g, self.dtype, self.robust, self.stack = prob, Graph(prob), dtype, robust, []
        (self.es,) = prob.edges
        self.vs = {v.vtype: v for v in prob.vertices}
        self.est = {t: np.array((est or {}).get(t, v.est), dtype) for t, v in self.vs.items()}
        self.rowc = np.searchsorted(self.vs[V_CAM].ids, self.es.v0)
        self.rowp = np.searchsorted(self.vs[V_XYZ].ids, self.es.v1)
        assert np.array_equal(self.vs[V_CAM].ids[self.rowc], self.es.v0) and np.array_equal(self.vs[V_XYZ].ids[self.rowp], self.es.v1)

    _rho = sim3_ref.Dense._rho

    def _records(self):
        return records(self.est[V_CAM][self.rowc], self.est[V_XYZ][self.rowp], self.es.meas, self.dtype)

    def edge_chi2(self):
        r = self._records()
        return np.einsum("ni,nij,nj->n", r[:, :2], np.asarray(self.es.info, self.dtype), r[:, :2])

    def chi2(self):
        return self.dtype(np.sum(self._rho(self.edge_chi2())[0]))

    def system(self):
        g, es, dt = self.g, self.es, self.dtype
        r = self._records()
        e, Ji, Jj = r[:, :2], r[:, 2:20].reshape(-1, 2, 9), r[:, 20:].reshape(-1, 2, 3)
        Om = np.asarray(es.info, dt)
        Om = Om * self._rho(np.einsum("ni,nij,nj->n", e, Om, e))[1][:, None, None]
        H, b = np.zeros((g.n, g.n), dt), np.zeros(g.n, dt)
        for k in range(len(e)):
            Js = [(g.off[int(v)], J[k]) for v, J in ((es.v0[k], Ji), (es.v1[k], Jj)) if int(v) in g.off]
            for oa, Ja in Js:
                b[oa:oa + Ja.shape[1]] -= Ja.T @ Om[k] @ e[k]
                for ob, Jb in Js:
                    H[oa:oa + Ja.shape[1], ob:ob + Jb.shape[1]] += Ja.T @ Om[k] @ Jb
        return H, b

    def stage(self, lam, cfg=None):
        H, b = self.system()
        self.H = H
        x, ok = sim3_ref.solve_spd(H + self.dtype(lam) * np.eye(len(b), dtype=self.dtype), b)
        return dict(ok=ok, b=b, x=x, np=self.g.npose, nl=(self.g.n - self.g.npose) // 3)

    def hessian_dense(self, npose, nl):
        return (self.H[:npose, :npose],)

    def push(self):
        self.stack.append({t: v.copy() for t, v in self.est.items()})

    def pop(self):
        self.est = self.stack.pop()

    def discard_top(self):
        self.stack.pop()

    def update(self, x):
        for i, o in self.g.off.items():
            vs, r = self.g.row[i]
            self.est[vs.vtype][r] += x[o:o + unary_ref.V_DIM[vs.vtype]]  # both vertex types: estimate += update

    def minimal_state(self):
        """Every vertex's values in id order, as g2ohip_minimal_state gives them."""
        ids = sorted(self.g.row)
        return np.concatenate([self.est[self.g.row[i][0].vtype][self.g.row[i][1]] for i in ids])


lm = sim3_ref.lm


def gn(dense, iterations):
    """OptimizationAlgorithmGaussNewton::solve per iteration (optimization_algorithm_gauss_newton.cpp:53-95): build,
    solve without damping, update; [chi2 after]. Stops where the solve is not positive definite."""
    out = []
    for _ in range(iterations):
        H, b = dense.system()
        x, ok = sim3_ref.solve_spd(H, b)
        if not ok:
            break
        dense.update(x)
        out.append(float(dense.chi2()))
    return out


# ---------------------------------------------------------------- the BAL text format (bal_example.cpp:336-406)
def bal_text(prob, sep="\n"):
    """ncams npts nobs | cam pt x y per observation | 9 values per camera | 3 per point, with repr()'s 17 digits. The
    cameras' ids must be 0 .. ncams-1 and the points' ncams .. ncams+npts-1."""
    vs = {v.vtype: v for v in prob.vertices}
    (es,) = prob.edges
    nc, npt = len(vs[V_CAM].ids), len(vs[V_XYZ].ids)
    assert np.array_equal(vs[V_CAM].ids, np.arange(nc)) and np.array_equal(vs[V_XYZ].ids, nc + np.arange(npt))
    lines = ["%d %d %d" % (nc, npt, len(es.v0))]
    lines += ["%d %d %r %r" % (a, b - nc, float(m[0]), float(m[1])) for a, b, m in zip(es.v0, es.v1, es.meas)]
    lines += [repr(float(x)) for x in vs[V_CAM].est.ravel()]
    lines += [repr(float(x)) for x in vs[V_XYZ].est.ravel()]
    return sep.join(lines) + "\n"


def parse_bal(text):
    """(cameras [nc, 9], points [np, 3], cam index [no], point index [no], observations [no, 2]) of a BAL text."""
    w = text.split()
    nc, npt, no = int(w[0]), int(w[1]), int(w[2])
    assert len(w) == 3 + 4 * no + 9 * nc + 3 * npt, (len(w), nc, npt, no)
    ob = np.array(w[3:3 + 4 * no]).reshape(no, 4)
    o = 3 + 4 * no
    cams = np.array([float(x) for x in w[o:o + 9 * nc]]).reshape(nc, 9)
    pts = np.array([float(x) for x in w[o + 9 * nc:]]).reshape(npt, 3)
    return cams, pts, ob[:, 0].astype(np.int64), ob[:, 1].astype(np.int64), ob[:, 2:].astype(np.float64)


def problem_of(cams, pts, ci, pi, obs, marginalize=True, name="balfile"):
    """The graph g2ohip_load_bal builds from parse_bal's arrays."""
    nc, npt = len(cams), len(pts)
    info = np.broadcast_to(np.eye(2), (len(ci), 2, 2)).copy()
    return synth.Problem(name, [_vs(V_CAM, np.arange(nc), cams), _vs(V_XYZ, nc + np.arange(npt), pts, marg=int(marginalize))],
                         [_es(E, ci, nc + pi, obs, info)], 9, 3 if marginalize else 0)


# ---------------------------------------------------------------- generators
def _rand_cams(rng, n, theta=None):
    """Cameras looking down -z, as BAL's do: rotations of 0.1 to 0.6 rad about a random axis (theta: that angle), small
    translations, f 400 - 600, |k1| <= 0.05, |k2| <= 0.01 with both signs: both distortion terms move the pixels."""
    ax = rng.standard_normal((n, 3))
    ax /= np.linalg.norm(ax, axis=1)[:, None]
    ang = rng.uniform(0.1, 0.6, n) if theta is None else np.full(n, float(theta))
    k1 = rng.uniform(0.01, 0.05, n) * rng.choice([-1.0, 1.0], n)
    k2 = rng.uniform(0.002, 0.01, n) * rng.choice([-1.0, 1.0], n)
    return np.concatenate([ax * ang[:, None], rng.uniform(-0.3, 0.3, (n, 3)), rng.uniform(400, 600, (n, 1)), k1[:, None],
                           k2[:, None]], 1)


def _points_seen_by(rng, cam, n, depth=(3.0, 6.0)):
    """n world points whose camera-frame image lies at depth 3 - 6 in front of the camera (z < 0), |x|, |y| <= 1."""
    Pc = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), -rng.uniform(*depth, n)], 1) - cam[3:6]
    return rotate(np.repeat(-cam[None, :3], n, 0), Pc, LD).astype(np.float64)  # R(-w) = R(w)^T


def _observe(rng, cams, pts):
    """The projections moved by 3 to 6 px in a random direction: no residual comes near zero, for the reason
    sim3_project_ref._observe gives (a small residual between large coordinates holds the chi2's digits in their
    last bits)."""
    n = len(pts)
    ang, mag = rng.uniform(0, 2 * np.pi, n), rng.uniform(3.0, 6.0, n)
    return error(cams, pts, np.zeros((n, 2))) + mag[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)


def one_edge(free_camera, theta=None, seed=0):
    """One camera (id 3) and one point (id 7) with one observation and a non-diagonal information: the camera free and
    the point fixed, or the camera fixed and the point free and marginalised. theta: the camera's rotation angle."""
    rng = np.random.default_rng(9000 + seed + 10 * free_camera)
    cam = _rand_cams(rng, 1, theta)
    pts = _points_seen_by(rng, cam[0], 1)
    obs = _observe(rng, cam, pts)
    verts = [_vs(V_CAM, [3], cam, [0 if free_camera else 1]), _vs(V_XYZ, [7], pts, [1 if free_camera else 0], marg=0 if free_camera else 1)]
    if not free_camera:  # BlockSolver needs a free non-marginalised vertex: a second, free camera sees the point too
        cam2 = _rand_cams(rng, 1)
        cam2[0, :6] = cam[0, :6] + 0.01 * rng.standard_normal(6)
        verts[0] = _vs(V_CAM, [3, 4], np.concatenate([cam, cam2]), [1, 0])
        obs = np.concatenate([obs, _observe(rng, cam2, pts)])
        return synth.Problem("bal1p", verts, [_es(E, [3, 4], [7, 7], obs, _spd(rng, 2, 2))], 9, 3)
    return synth.Problem("bal1c", verts, [_es(E, [3], [7], obs, _spd(rng, 2))], 9, 0)


def scene(nc, npt, per_point, seed, fixed_cams=(), fixed_pts=(), uniform=True, marginalize=True, perturb=True, name=None):
    """nc cameras around one pose (ids 0 .. nc-1) and npt points (ids nc ..) in front of all of them; point k is seen
    by per_point cameras (k, k + 1, ... mod nc; per_point >= nc: by all). uniform: one information record (the
    identity), else per-edge ones. perturb: the start is moved off the generating state by a fraction of a pixel's
    worth, so the residuals stay the observations' 3 - 6 px offsets."""
    rng = np.random.default_rng(seed)
    base = _rand_cams(rng, 1)[0]
    cams = _rand_cams(rng, nc)
    cams[:, :6] = base[:6] + np.array([0.05] * 3 + [0.4] * 3) * rng.standard_normal((nc, 6))  # a baseline to triangulate over
    pts = _points_seen_by(rng, base, npt)
    pp = min(per_point, nc)
    ci = ((np.arange(npt)[:, None] + np.arange(pp)[None]) % nc).ravel()
    pi = np.repeat(np.arange(npt), pp)
    obs = _observe(rng, cams[ci], pts[pi])
    info = np.broadcast_to(np.eye(2), (len(ci), 2, 2)).copy() if uniform else _spd(rng, 2, len(ci))
    if perturb:
        cams = cams + np.array([1e-4] * 6 + [5e-2, 1e-5, 1e-6]) * rng.standard_normal((nc, 9))
        pts = pts + 1e-3 * rng.standard_normal((npt, 3))
    fc, fp = np.zeros(nc, np.int32), np.zeros(npt, np.int32)
    fc[list(fixed_cams)] = 1
    fp[list(fixed_pts)] = 1
    return synth.Problem(name or f"bal{nc}x{npt}", [_vs(V_CAM, np.arange(nc), cams, fc), _vs(V_XYZ, nc + np.arange(npt), pts, fp, marg=int(marginalize))],
                         [_es(E, ci, nc + pi, obs, info)], 9, 3 if marginalize else 0)


def kernel_case(ne, uniform):
    """ne observations: 4 cameras (camera 2 fixed) see ceil(ne / 4) points (point 1 fixed), cut to ne edges. ne = 1:
    the one edge joins free camera 0 and the point, which is the fixed one (a single observation of a free point leaves
    the Schur complement as the difference of two nearly equal blocks: tests of the 9/3 Schur kernels have that row)."""
    npt = (ne + 3) // 4
    p = scene(4, npt, 4, 9100 + ne, fixed_cams=(2,) if ne > 1 else (), fixed_pts=(1,) if npt > 1 else (0,), uniform=uniform,
              name=f"balk{ne}_{int(uniform)}")
    (es,) = p.edges
    p.edges[0] = _es(E, es.v0[:ne], es.v1[:ne], es.meas[:ne], es.info[:ne])
    return p


def degree_case(which):
    """Graphs whose average camera degree falls in each lane class of the vertex reduction: under 6, 6 - 15, 16 - 127
    and >= 128 (two cameras x 260 common points)."""
    nc, npt, pp = {"lt6": (6, 8, 3), "6to15": (4, 10, 4), "16to127": (3, 40, 3), "ge128": (2, 260, 2)}[which]
    return scene(nc, npt, pp, 9200 + npt, name=f"baldeg_{which}")


def schur_case(which):
    """Camera rows for k_schur_diag's wave loop (1, 64, 65, 257 observations of camera 0 beside a second camera that
    sees them all), one camera with more than 64 off-diagonal neighbours (70 cameras, every point seen by camera 0 and
    one other), a row whose staged blocks exceed one 128-block batch (two cameras x 260 common points)."""
    if which == "neighbours":
        nc, npt = 70, 138
        rng = np.random.default_rng(9350)
        p = scene(nc, npt, 1, 9300, name="balschur_nb")
        (es,) = p.edges
        other = 1 + np.arange(npt) % (nc - 1)
        cams = p.vertices[0].est
        pts = p.vertices[1].est
        ci = np.concatenate([np.zeros(npt, np.int64), other])
        pi = np.concatenate([np.arange(npt), np.arange(npt)])
        obs = _observe(rng, cams[ci], pts[pi])
        p.edges[0] = _es(E, ci, nc + pi, obs, np.broadcast_to(np.eye(2), (len(ci), 2, 2)).copy())
        return p
    n = int(which)
    return scene(2, n, 2, 9300 + n, name=f"balschur_{n}")


def trajectory_case(fixed):
    """6 cameras x 40 points, every point seen by every camera. fixed: the cameras held (() as bal_example leaves them, (0,)
    or the pair (0, 1) that holds the gauge for Gauss-Newton and dogleg). The start is 1 - 2 px off the generating state,
    so that LM has something to do and every trial's rho stays clear of 0."""
    rng = np.random.default_rng(9400)
    p = scene(6, 40, 6, 9400, fixed_cams=fixed, perturb=False, name=f"baltraj_{len(fixed)}")
    p.vertices[0].est += np.array([2e-4] * 6 + [0.5, 1e-4, 1e-5]) * rng.standard_normal((6, 9))
    p.vertices[1].est += 2e-3 * rng.standard_normal((40, 3))
    return p


# (algorithm, fixed cameras): LM as bal_example runs it and with camera 0 fixed; Gauss-Newton and dogleg solve without
# damping and need the gauge held: two fixed cameras (one leaves the scale free and H singular)
TRAJECTORIES = [("lm", ()), ("lm", (0,)), ("gn", (0, 1)), ("dl", (0, 1))]

# The float64 floor of a staged system's x (numpy float64 against longdouble, relative) where it is above 1e-11: the
# graph of one point under two observations, whose H + lambda I has the condition of 1 / 1e-5 and more. Its x is compared
# at 64 x the floor (the factor of tests/test_gpu_cholesky_edges.py), every other case at 1e-9; tests/test_bal_host.py measures both.
X_FLOOR = {"bal1p": 3.4e-10}


def x_tolerance(prob):
    return 64 * X_FLOOR[prob.name] if prob.name in X_FLOOR else 1e-9


def solve_in(prob, dtype, lam=None, robust=None):
    """x of the staged system in a dtype, by the Schur complement where the graph has landmarks; lam None: LM's first."""
    d = Dense(prob, dtype, robust)
    H, b = d.system()
    lam = dtype(1e-5) * np.max(np.diag(H)) if lam is None else dtype(lam)
    n, npz = d.g.n, d.g.npose
    Hd = H + lam * np.eye(n, dtype=dtype)
    if n == npz:
        return sim3_ref.solve_spd(Hd, b)[0]
    Hpp, Hpl, Hll = Hd[:npz, :npz], Hd[:npz, npz:], Hd[npz:, npz:]
    W, Dinv = np.zeros_like(Hpl), []
    for o in range(0, n - npz, 3):
        Di = np.stack([sim3_ref.solve_spd(Hll[o:o + 3, o:o + 3], np.eye(3, dtype=dtype)[c])[0] for c in range(3)], 1)
        Dinv.append(Di)
        W[:, o:o + 3] = Hpl[:, o:o + 3] @ Di
    xp = sim3_ref.solve_spd(Hpp - W @ Hpl.T, b[:npz] - W @ b[npz:])[0]
    r = b[npz:] - Hpl.T @ xp
    return np.concatenate([xp] + [Di @ r[3 * k:3 * k + 3] for k, Di in enumerate(Dinv)])


def staged_cases():
    """[problem]: every graph whose staged system a GPU test compares with numpy."""
    out = [one_edge(True), one_edge(False), one_edge(True, 0.0)]
    out += [kernel_case(ne, u) for ne in (1, 63, 64, 65, 257) for u in (True, False)]
    out += [degree_case(w) for w in ("lt6", "6to15", "16to127", "ge128")]
    out += [schur_case(w) for w in ("1", "64", "65", "257", "neighbours", "260")]
    return out + [trajectory_case(f) for f in ((), (0,), (0, 1))]


def outlier_case():
    """trajectory_case((0,))'s shape with 40 observations of which 4 are moved by 50 px: (problem, the moved ones)."""
    rng = np.random.default_rng(9500)
    p = scene(4, 10, 4, 9500, fixed_cams=(0,), name="balout")
    bad = np.zeros(40, bool)
    bad[rng.choice(40, 4, replace=False)] = True
    ang = rng.uniform(0, 2 * np.pi, 4)
    p.edges[0].meas[bad] += 50.0 * np.stack([np.cos(ang), np.sin(ang)], 1)
    return p, bad


def pin_huber(prob):
    """Huber with every edge on the linear branch: delta half of the smallest sqrt(chi2)."""
    return ("Huber", 0.5 * float(np.sqrt(Graph(prob).edge_chi2().min())))


def median_huber(prob):
    """Huber with half of the edges on the linear branch."""
    return ("Huber", float(np.sqrt(np.median(Graph(prob).edge_chi2()))))


def chi2_cases():
    """[(problem, robust or None)]: every graph at whose start a GPU test compares chi2 (in total or per edge) at 1e-12:
    each staged system, the outlier graph, and the Huber-robustified chi2 of the pins and of the 65-edge kernel case."""
    out = [(p, None) for p in staged_cases()] + [(outlier_case()[0], None)]
    out += [(p, pin_huber(p)) for p in (one_edge(True), one_edge(False))]
    return out + [(kernel_case(65, False), median_huber(kernel_case(65, False)))]
