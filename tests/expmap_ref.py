"""Plain-numpy restatement of the edges on VertexSE3Expmap besides the two BA projections (test reference; nothing here
comes from the oracle or the library).

  EdgeSE3Expmap                    types_six_dof_expmap.h:117-124, .cpp:278-293
      e = log(Tj^-1 * C * Ti),  Ji = adj(Tj^-1 * C),  Jj = -adj(Ti^-1 * C^-1)
  EdgeSE3ProjectXYZOnlyPose        types_six_dof_expmap.h:242-246, .cpp:569-599
      e = obs - (x/z fx + cx, y/z fy + cy) of T.map(Xw); J in invz / invz_2 products
  EdgeStereoSE3ProjectXYZOnlyPose  types_six_dof_expmap.h:303-307, .cpp:601-665
      the same with u_r = u - bf invz; the error's invz is a float (np.float32), the Jacobian's a double

and of SE3Quat (types/slam3d/se3quat.h): operator* (normalises the rotation, w >= 0), inverse, log (both branches),
exp, adj.  A transform is a 7-vector tx ty tz qx qy qz qw, as the vertex estimate.  Every function takes a dtype, so
the chi2 of a graph can be evaluated in np.longdouble too (the acos band tolerance, test_expmap_host.py).

Graphs: `Graph` extends unary_ref.Graph (dense_system, chi2, solve come from there) with the three types; the BA
projections of a mixed graph are restated from stereo_ref / the monocular formulas of the same file.
"""
import numpy as np

import stereo_ref
import unary_ref
from g2o_amd import synth

E_EXPMAP = synth.E_SE3_EXPMAP
E_MONO = synth.E_SE3_PROJECT_XYZ_ONLYPOSE
E_STEREO = synth.E_STEREO_SE3_PROJECT_XYZ_ONLYPOSE
POSE_ONLY = (E_MONO, E_STEREO)


# ---------------------------------------------------------------- quaternions (x, y, z, w), SE3Quat
def _a(v, dtype):
    return np.asarray(v, dtype)


def quat_to_R(q):
    """Eigen toRotationMatrix."""
    x, y, z, w = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1 - (txx + tyy)]], dtype=q.dtype)


def qrot(q, v):
    """Eigen's Quaternion * Vector3."""
    u = q[:3]
    uv = 2 * np.cross(u, v)
    return v + q[3] * uv + np.cross(u, uv)


def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz], dtype=a.dtype)


def normalize_rotation(q):
    """SE3Quat::normalizeRotation: w >= 0, unit norm."""
    if q[3] < 0:
        q = -q
    return q / np.sqrt(q @ q)


def from_vector(v, dtype=np.float64):
    """SE3Quat(Vector7) (se3quat.h:81-88): the rotation normalised."""
    v = _a(v, dtype)
    return np.concatenate([v[:3], normalize_rotation(v[3:7])])


def inv(T):
    """SE3Quat::inverse (se3quat.h:118-123)."""
    qc = np.concatenate([-T[3:6], T[6:7]])
    return np.concatenate([qrot(qc, -T[:3]), qc])


def mul(A, B, raw=False):
    """SE3Quat::operator* (se3quat.h:99-105). raw: also return w of the quaternion product before normalisation."""
    q = qmul(A[3:7], B[3:7])
    T = np.concatenate([A[:3] + qrot(A[3:7], B[:3]), normalize_rotation(q)])
    return (T, q[3]) if raw else T


def skew(v):
    z = v.dtype.type(0)
    return np.array([[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]], dtype=v.dtype)


def log(T):
    """SE3Quat::log (se3quat.h:173-210): (omega, upsilon)."""
    dt = T.dtype.type
    R = quat_to_R(T[3:7])
    d = dt(0.5) * (R[0, 0] + R[1, 1] + R[2, 2] - 1)
    dR = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]], dtype=T.dtype)
    eye = np.eye(3, dtype=T.dtype)
    if d > dt(0.99999):
        omega = dt(0.5) * dR
        Om = skew(omega)
        Vinv = eye - dt(0.5) * Om + (dt(1) / dt(12)) * (Om @ Om)
    else:
        theta = np.arccos(d)
        omega = theta / (2 * np.sqrt(1 - d * d)) * dR
        Om = skew(omega)
        Vinv = eye - dt(0.5) * Om + (1 - theta / (2 * np.tan(theta / 2))) / (theta * theta) * (Om @ Om)
    return np.concatenate([omega, Vinv @ T[:3]])


def exp(u):
    """SE3Quat::exp (se3quat.h:217-257) of (omega, upsilon), float64."""
    u = _a(u, np.float64)
    dt = u.dtype.type
    om, ups = u[:3], u[3:]
    theta = np.sqrt(om @ om)
    Om = skew(om)
    Om2 = Om @ Om
    eye = np.eye(3, dtype=u.dtype)
    if theta < dt(0.00001):
        R = eye + Om + dt(0.5) * Om2
        V = eye + dt(0.5) * Om + dt(1) / dt(6) * Om2
    else:
        R = eye + np.sin(theta) / theta * Om + (1 - np.cos(theta)) / (theta * theta) * Om2
        V = eye + (1 - np.cos(theta)) / (theta * theta) * Om + (theta - np.sin(theta)) / theta ** 3 * Om2
    return np.concatenate([V @ ups, normalize_rotation(synth.rot_to_quat(R[None])[0])])


def adj(T):
    """SE3Quat::adj (se3quat.h:259-268): [[R, 0], [skew(t) R, R]]."""
    R = quat_to_R(T[3:7])
    J = np.zeros((6, 6), dtype=T.dtype)
    J[:3, :3] = R
    J[3:, 3:] = R
    J[3:, :3] = skew(T[:3]) @ R
    return J


# ---------------------------------------------------------------- EdgeSE3Expmap
def expmap_error(Ti, Tj, C, dtype=np.float64, raw=False):
    """log(Tj^-1 * C * Ti). raw: also (w before normalisation of Tj^-1 * C, of the whole product)."""
    Ti, Tj, C = _a(Ti, dtype), _a(Tj, dtype), from_vector(C, dtype)
    A, w1 = mul(inv(Tj), C, raw=True)
    E, w2 = mul(A, Ti, raw=True)
    e = log(E)
    return (e, (w1, w2)) if raw else e


def expmap_jacobians(Ti, Tj, C, dtype=np.float64):
    Ti, Tj, C = _a(Ti, dtype), _a(Tj, dtype), from_vector(C, dtype)
    return adj(mul(inv(Tj), C)), -adj(mul(inv(Ti), inv(C)))


def residual_angle(Ti, Tj, C):
    """|omega| of the edge's error: the rotation angle of Tj^-1 * C * Ti."""
    return float(np.linalg.norm(expmap_error(Ti, Tj, C)[:3]))


# ---------------------------------------------------------------- the pose-only projections
def _map_n(T, xw):
    """SE3Quat::map of points [n, 3] by transforms [n, 7]."""
    u = T[:, 3:6]
    uv = 2 * np.cross(u, xw)
    return xw + T[:, 6:7] * uv + np.cross(u, uv) + T[:, :3]


def pose_only_error(etype, T, par, obs, dtype=np.float64, float_invz=True):
    """obs - cam_project(T.map(Xw)); par = Xw fx fy cx cy (bf). float_invz: the stereo type's float 1/z. One edge
    (1-D arguments) or n edges ([n, .] arguments)."""
    T, par, obs = _a(T, dtype), _a(par, dtype), _a(obs, dtype)
    if T.ndim == 1:
        return pose_only_error(etype, T[None], par[None], obs[None], dtype, float_invz)[0]
    pc = _map_n(T, par[:, :3])
    fx, fy, cx, cy = par[:, 3], par[:, 4], par[:, 5], par[:, 6]
    if etype == E_MONO:
        return obs - np.stack([pc[:, 0] / pc[:, 2] * fx + cx, pc[:, 1] / pc[:, 2] * fy + cy], axis=1)
    invz = 1 / pc[:, 2]
    if float_invz:
        invz = invz.astype(np.float32).astype(pc.dtype)
    u = pc[:, 0] * invz * fx + cx
    v = pc[:, 1] * invz * fy + cy
    return obs - np.stack([u, v, u - par[:, 7] * invz], axis=1)


def pose_only_jacobian(etype, T, par):
    """[D, 6] of one edge, [n, D, 6] of n."""
    T, par = _a(T, np.float64), _a(par, np.float64)
    if T.ndim == 1:
        return pose_only_jacobian(etype, T[None], par[None])[0]
    pc = _map_n(T, par[:, :3])
    x, y, z = pc[:, 0], pc[:, 1], pc[:, 2]
    fx, fy = par[:, 3], par[:, 4]
    invz = 1.0 / z
    invz_2 = invz * invz
    zero = np.zeros(len(T))
    r0 = [x * y * invz_2 * fx, -(1 + (x * x * invz_2)) * fx, y * invz * fx, -invz * fx, zero, x * invz_2 * fx]
    r1 = [(1 + y * y * invz_2) * fy, -x * y * invz_2 * fy, -x * invz * fy, zero, -invz * fy, y * invz_2 * fy]
    rows = [np.stack(r0, axis=1), np.stack(r1, axis=1)]
    if etype == E_STEREO:
        bf = par[:, 7]
        rows.append(np.stack([r0[0] - bf * y * invz_2, r0[1] + bf * x * invz_2, r0[2], r0[3], zero,
                              r0[5] - bf * invz_2], axis=1))
    return np.stack(rows, axis=1)


def ba_edge(etype, pt, cam, meas, K):
    """The binary projections of a mixed graph: (e, J_point, J_camera). Monocular: types_six_dof_expmap.cpp:395-455."""
    if etype == synth.E_STEREO_SE3_PROJECT_XYZ:
        Ji, Jj = stereo_ref.edge_jacobians(cam, pt, K)
        return stereo_ref.edge_error(cam, pt, meas, K)[0], Ji[0], Jj[0]
    K5 = np.concatenate([K, [0.0]])
    Ji, Jj = stereo_ref.edge_jacobians(cam, pt, K5)
    return stereo_ref.edge_error(cam, pt, np.concatenate([meas, [0.0]]), K5, float_bf=False)[0][:2], Ji[0][:2], Jj[0][:2]


# ---------------------------------------------------------------- graphs
class Graph(unary_ref.Graph):
    """unary_ref.Graph with EdgeSE3Expmap, the pose-only projections and the BA projections restated here (binary
    records, where given for a type, still take precedence)."""

    def edge(self, es, k, est=None, binary=None):
        if binary and es.etype in binary:
            return super().edge(es, k, est, binary)
        i = int(es.v0[k])
        _, xi = self._est(est, i)
        if es.etype in POSE_ONLY:
            return (pose_only_error(es.etype, xi, es.params[k], es.meas[k]),
                    [(i, pose_only_jacobian(es.etype, xi, es.params[k]))])
        if es.etype == E_EXPMAP:
            j = int(es.v1[k])
            _, xj = self._est(est, j)
            Ji, Jj = expmap_jacobians(xi, xj, es.meas[k])
            return expmap_error(xi, xj, es.meas[k]), [(i, Ji), (j, Jj)]
        if es.etype in (synth.E_SE3_PROJECT_XYZ, synth.E_STEREO_SE3_PROJECT_XYZ):
            j = int(es.v1[k])
            _, xj = self._est(est, j)
            e, Ji, Jj = ba_edge(es.etype, xi, xj, es.meas[k], es.params[k])
            return e, [(i, Ji), (j, Jj)]
        return super().edge(es, k, est, binary)

    def payload(self, etype, est=None):
        """Host-J records of one edge type, in edge order: [e | Ji] per unary edge, [e | Ji | Jj] per binary one."""
        out = []
        for es in self.prob.edges:
            if es.etype == etype and etype in POSE_ONLY:  # all edges at once
                vs = self.row[int(es.v0[0])][0]
                src = vs.est if est is None or vs.vtype not in est else np.asarray(est[vs.vtype])
                order = np.argsort(vs.ids)
                T = src[order[np.searchsorted(vs.ids[order], es.v0)]]
                e, J = pose_only_error(etype, T, es.params, es.meas), pose_only_jacobian(etype, T, es.params)
                out.append(np.concatenate([e, J.reshape(len(e), -1)], axis=1).ravel())
            elif es.etype == etype:
                for k in range(len(es.v0)):
                    e, Js = self.edge(es, k, est)
                    out += [e] + [J.ravel() for _, J in Js]
        return np.concatenate(out)

    def chi2_in(self, dtype, only=(E_EXPMAP, E_MONO, E_STEREO)):
        """chi2 of the three types' edges at the problem's own estimates with every operation in dtype."""
        c = dtype(0)
        for es in self.prob.edges:
            if es.etype in only:
                for k in range(len(es.v0)):
                    xi = self._est(None, es.v0[k])[1]
                    if es.etype == E_EXPMAP:
                        e = expmap_error(xi, self._est(None, es.v1[k])[1], es.meas[k], dtype)
                    else:
                        e = pose_only_error(es.etype, xi, es.params[k], es.meas[k], dtype)
                    c += e @ _a(es.info[k], dtype) @ e
        return c

    def residual_angles(self, est=None):
        out = []
        for es in self.prob.edges:
            if es.etype == E_EXPMAP:
                for k in range(len(es.v0)):
                    out.append(residual_angle(self._est(est, es.v0[k])[1], self._est(est, es.v1[k])[1], es.meas[k]))
        return np.array(out)


def hostj_version(prob, types=(E_EXPMAP, E_MONO, E_STEREO)):
    """The same graph with the edge sets of the given types entered as host-J sets: E_HOSTJ(6) for EdgeSE3Expmap,
    E_HOSTJ_UNARY(D) for the pose-only types. Returns (problem, {host-J type: original type})."""
    import g2o_amd
    edges, back = [], {}
    for es in prob.edges:
        if es.etype in types:
            D = synth.ERR_DIM[es.etype]
            ht = g2o_amd.E_HOSTJ(D) if es.v1 is not None else g2o_amd.E_HOSTJ_UNARY(D)
            assert ht not in back, "one set per host-J type"
            back[ht] = es.etype
            edges.append(synth.EdgeSet(ht, es.v0, es.v1, None, es.info, None))
        else:
            edges.append(es)
    return synth.Problem(prob.name + "/hostj", prob.vertices, edges, prob.pose_dim, prob.landmark_dim), back


def set_residuals(prob, r):
    """Rewrite the measurements of the problem's EdgeSE3Expmap set so that edge k's error at the problem's own
    estimates is r[k] (omega, upsilon), up to rounding: C = Tj * exp(r) * Ti^-1."""
    es = next(e for e in prob.edges if e.etype == E_EXPMAP)
    row = {}
    for vs in prob.vertices:
        for k, i in enumerate(vs.ids):
            row[int(i)] = vs.est[k]
    for k in range(len(es.v0)):
        Ti, Tj = from_vector(row[int(es.v0[k])]), from_vector(row[int(es.v1[k])])
        es.meas[k] = mul(mul(Tj, exp(r[k])), inv(Ti))
    return prob


# ---------------------------------------------------------------- the cases both test files use
# acos near 1: relative difference of the band case's chi2 (band_case below) between float64 and np.longdouble as
# measured by test_expmap_host.py::test_band_tolerance (x86-64 glibc, 80-bit long double), rounded up to two digits; the
# GPU test's tolerance for that case is 4 times it (a second implementation's independent rounding plus the acos / tan
# ulp differences between glibc and the device math library).
BAND_MEASURED = 3.8e-15  # measured 3.75e-15
BAND_TOL = 4 * BAND_MEASURED


def _spd(rng, D):
    A = np.eye(D) + 0.3 * rng.standard_normal((D, D))
    return A @ A.T


def one_pose_only(etype):
    """One free camera, one pose-only edge of the type: non-diagonal information, fx != fy. The point sits at
    (0.4, -0.3, 3.7) in the camera frame (1/z is no float), the principal point is small (160, 120) and the observation is off by 6 to 8 px:
    the error is at least 1/30 of the quantities it is the difference of."""
    rng = np.random.default_rng(300 + etype)
    T = np.array([0.3, -1.2, 2.0, 0.1, -0.2, 0.3, 0.9])
    T[3:] /= np.linalg.norm(T[3:])
    pc = np.array([0.4, -0.3, 3.7])
    xw = qrot(inv(T)[3:7], pc - T[:3])
    fx, fy, cx, cy, bf = 260.0, 250.0, 160.0, 120.0, 30.0
    u, v = fx * pc[0] / pc[2] + cx, fy * pc[1] / pc[2] + cy
    if etype == E_MONO:
        obs, par = np.array([u + 8.0, v - 6.0]), np.concatenate([xw, [fx, fy, cx, cy]])
    else:
        obs, par = np.array([u + 8.0, v - 6.0, u - bf / pc[2] + 7.0]), np.concatenate([xw, [fx, fy, cx, cy, bf]])
    cams = synth.VertexSet(synth.V_SE3_EXPMAP, np.array([4], np.int32), T[None], np.zeros(1, np.int32), np.zeros(1, np.int32))
    es = synth.EdgeSet(etype, np.array([4], np.int32), None, obs[None], _spd(rng, len(obs))[None], par[None])
    return synth.Problem(f"one{etype}", [cams], [es], 6, 0)


def one_expmap(kind):
    """Two free cameras and one EdgeSE3Expmap, non-diagonal information. kind: "small" (residual angle 0.003: the
    series branch of log), "regular" (0.7 rad), "wneg" (Tj turns by -2 rad and Ti by 2.28 rad about nearly the same
    axis, so Tj^-1 and C each turn by ~2 rad and the quaternion of Tj^-1 * C has w = cos(2) < 0 before
    SE3Quat::operator* normalises it; residual 0.5 rad)."""
    rng = np.random.default_rng({"small": 1, "regular": 2, "wneg": 3}[kind] + 400)
    Ti = exp([0.1, -0.1, 2.28, 1.0, -2.0, 0.5] if kind == "wneg" else [0.4, -0.3, 0.2, 1.0, -2.0, 0.5])
    ang = {"small": 0.003, "regular": 0.7, "wneg": 0.5}[kind]
    r = np.concatenate([ang * np.array([0.6, -0.64, 0.48]), [0.3, -0.2, 0.25]])
    if kind == "wneg":
        Tj = exp([0.05, 0.1, -2.0, 0.5, 1.0, -1.5])
    else:
        Tj = exp([-0.2, 0.5, 0.3, 2.0, 1.0, -1.5])
    C = mul(mul(Tj, exp(r)), inv(Ti))  # error = r at these estimates
    est = np.stack([Ti, Tj])
    cams = synth.VertexSet(synth.V_SE3_EXPMAP, np.array([2, 5], np.int32), est, np.zeros(2, np.int32), np.zeros(2, np.int32))
    es = synth.EdgeSet(E_EXPMAP, np.array([2], np.int32), np.array([5], np.int32), C[None], _spd(rng, 6)[None], None)
    return synth.Problem(f"expmap_{kind}", [cams], [es], 6, 0)


def residuals_outside_band(n, seed, small_fraction=0.5):
    """n residuals (omega, upsilon): rotation angles 0.001 to 0.003 (the series branch) for a fraction, 0.1 to 1.0
    otherwise; upsilon up to 0.3 per component."""
    rng = np.random.default_rng(seed)
    axis = rng.standard_normal((n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    small = rng.random(n) < small_fraction
    ang = np.where(small, rng.uniform(0.001, 0.003, n), rng.uniform(0.1, 1.0, n))
    return np.concatenate([axis * ang[:, None], rng.uniform(-0.3, 0.3, (n, 3))], axis=1)


def assert_outside_band(angles):
    """Every residual angle below 0.004 rad or inside [0.05, 2.5]: clear of acos' ill-conditioned band and of pi."""
    angles = np.asarray(angles)
    ok = (angles < 0.004) | ((angles >= 0.05) & (angles <= 2.5))
    assert ok.all(), angles[~ok]


def expmap_case(num_poses, loops, seed, inside_band=False):
    """expmap_pose_graph at its true poses with the residual of every edge set: outside the acos band
    (residuals_outside_band), or every one inside it (angles 0.006 to 0.04)."""
    prob = synth.expmap_pose_graph(num_poses, loops, init="truth", seed=seed)
    n = prob.num_edges
    if inside_band:
        rng = np.random.default_rng(seed)
        axis = rng.standard_normal((n, 3))
        axis /= np.linalg.norm(axis, axis=1, keepdims=True)
        r = np.concatenate([axis * rng.uniform(0.006, 0.04, (n, 1)), rng.uniform(-0.01, 0.01, (n, 3))], axis=1)
    else:
        r = residuals_outside_band(n, seed)
    return set_residuals(prob, r)


def band_case():
    """The one pinned case inside the band: 24 poses, 3 loop closures, residual angles 0.006 to 0.04 rad and small
    translational residuals, so that omega carries the chi2."""
    return expmap_case(24, 3, 77, inside_band=True)
