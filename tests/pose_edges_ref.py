"""Plain-numpy reference of the pose-graph edges and the vertex oplus maps, written from the maths (test reference;
nothing here comes from the oracle or the library, and none of it is a port of the device's branch code).

Every function takes batches ([n, ...] arrays) and a `dtype`; np.longdouble is the high-precision mode.

Conventions. A 3D pose is (t, q) = x y z qx qy qz qw, an isometry X = (R, t). VertexSE3's oplus is X * (dt, dq): R <- R
(I + 2 [dq]x) to first order, t <- t + R dt. With q_e = (q_v, q_w), q_w >= 0, the quaternion of a rotation Re, a right
perturbation Re (I + [w]x) moves q_v by (q_w w + q_v x w) / 2. This one identity gives every rotation Jacobian below in a
form that is valid wherever q_w > 0, whichever entry of Re is largest:

  EdgeSE3       E = Z^-1 Xi^-1 Xj, A = Z^-1, B = Xi^-1 Xj:  e = (t_E, q_v(R_E))
                d e_t / d t_j = R_E              d e_q / d q_j = q_w I + [q_v]x
                d e_t / d t_i = -R_A             d e_t / d q_i = 2 R_A [t_B]x         d e_q / d q_i = -(q_w I + [q_v]x) R_B^T
  EdgeSE3Prior  E = Z^-1 X P, A = Z^-1 X, B = P:
                d e_t / d t = R_A                d e_t / d q = -2 R_A [t_P]x           d e_q / d q = (q_w I + [q_v]x) R_P^T
  EdgeSE2       e = Z^-1 (Xi^-1 Xj): e_t = Rz^T (Ri^T (tj - ti) - tz), e_th = wrap(thj - thi - thz); VertexSE2's oplus
                adds to x, y (world frame) and to the angle
  EdgeSE2PointXY  e = Ri^T (l - ti) - z

The quaternion of a rotation matrix is taken with the largest of the four squares 1 + tr, 1 + 2 r_kk - tr (Shepperd's
choice, not the trace-then-diagonal rule of the device code), then signed to q_w >= 0 and normalized.

The oplus maps follow the reference's rules, because these are rules and not maths: fromCompactQuaternion returns the
identity rotation when |dq|^2 > 1; VertexSE3 replaces R by R - R (R^T R - I) / 2 on every 1001st call; SE3Quat::exp uses
the series I + W + W^2 / 2, V = I + W / 2 + W^2 / 6 below theta = 1e-5; angles are wrapped into [-pi, pi) with the double
constant pi, only when they lie outside.

Case generators (deterministic, every input constructed for the branch it names): se3_branch_cases, prior_branch_cases,
se2_wrap_cases, se2xy_wrap_cases; the graphs made of them: single-edge problems, anchored chains, degree-ragged graphs.
"""
import numpy as np

from g2o_amd import synth

LD = np.longdouble
LABELS = ("tr+", "x+", "x-", "y+", "y-", "z+", "z-")
PI = float(np.pi)
# float64 against longdouble over oplus_cases, |difference| / max(1, |value|): measured by tests/test_pose_edges_host.py,
# which explains the first figure
OPLUS_FLOOR = {synth.V_SE3_EXPMAP: 4.6e-13, synth.V_XYZ: 2.8e-17, synth.V_SE3_QUAT: 1.8e-16, synth.V_SE2: 9.5e-17,
               synth.V_XY: 4.9e-17}


# ---------------------------------------------------------------- small algebra
def _a(x, dtype):
    return np.atleast_2d(np.asarray(x, dtype))


def skew(v):
    """[n, 3] -> [n, 3, 3], [v]x."""
    S = np.zeros(v.shape[:-1] + (3, 3), v.dtype)
    S[..., 0, 1], S[..., 0, 2], S[..., 1, 0] = -v[..., 2], v[..., 1], v[..., 2]
    S[..., 1, 2], S[..., 2, 0], S[..., 2, 1] = -v[..., 0], -v[..., 1], v[..., 0]
    return S


def rot(q, dtype=np.float64, normalize=True):
    """Rotation matrices [n, 3, 3] of quaternions (x, y, z, w) [n, 4]: I + 2 w [v]x + 2 [v]x^2. normalize=False is the
    vertex estimate's rule (fromVectorQT does not normalize), True the measurement's."""
    q = _a(q, dtype)
    if normalize:
        q = q / np.sqrt(np.sum(q * q, axis=-1, keepdims=True))
    S = skew(q[:, :3])
    return np.eye(3, dtype=dtype) + 2 * q[:, 3, None, None] * S + 2 * (S @ S)


def quat(R):
    """[n, 3, 3] -> the unit quaternions (x, y, z, w) with w >= 0, from the largest of the four squares."""
    R = np.asarray(R)
    dt = R.dtype
    tr = R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]
    sq = np.stack([1 + 2 * R[:, 0, 0] - tr, 1 + 2 * R[:, 1, 1] - tr, 1 + 2 * R[:, 2, 2] - tr, 1 + tr], 1)  # 4 q_k^2
    # the symmetric / antisymmetric parts hold the products 4 q_a q_b
    pr = np.zeros((len(R), 4, 4), dt)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        pr[:, a, b] = pr[:, b, a] = R[:, a, b] + R[:, b, a]
    pr[:, 0, 3] = pr[:, 3, 0] = R[:, 2, 1] - R[:, 1, 2]
    pr[:, 1, 3] = pr[:, 3, 1] = R[:, 0, 2] - R[:, 2, 0]
    pr[:, 2, 3] = pr[:, 3, 2] = R[:, 1, 0] - R[:, 0, 1]
    m = np.argmax(sq, axis=1)
    rows = np.arange(len(R))
    big = np.sqrt(sq[rows, m])  # 2 |q_m|
    q = pr[rows, m] / (2 * big[:, None])
    q[rows, m] = big / 2
    q = q / np.sqrt(np.sum(q * q, axis=1, keepdims=True))
    return np.where(q[:, 3:4] < 0, -q, q)


def qmul(a, b):
    """Hamilton product of (x, y, z, w) quaternions."""
    av, aw, bv, bw = a[:, :3], a[:, 3:4], b[:, :3], b[:, 3:4]
    return np.concatenate([aw * bv + bw * av + np.cross(av, bv), aw * bw - np.sum(av * bv, 1, keepdims=True)], 1)


def axis_angle(axis, angle, dtype=np.float64):
    """Rodrigues: [n, 3] axes (normalized here), [n] angles -> [n, 3, 3]."""
    k = _a(axis, dtype)
    k = k / np.sqrt(np.sum(k * k, axis=-1, keepdims=True))
    th = np.asarray(angle, dtype).reshape(-1, 1, 1)
    K = skew(k)
    return np.eye(3, dtype=dtype) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def wrap(th, dtype=np.float64):
    """normalize_theta: unchanged inside [-pi, pi), else brought there; pi is the double constant in every dtype."""
    th = np.asarray(th, dtype)
    pi = dtype(PI)
    w = th - np.floor(th / (2 * pi)) * (2 * pi)
    w = np.where(w >= pi, w - 2 * pi, w)
    w = np.where(w < -pi, w + 2 * pi, w)
    return np.where((th >= -pi) & (th < pi), th, w)


def rot2(th):
    c, s = np.cos(th), np.sin(th)
    return np.stack([np.stack([c, -s], -1), np.stack([s, c], -1)], -2)


def _mv(M, v):
    return np.einsum("nij,nj->ni", M, v)


def _T(M):
    return np.transpose(M, (0, 2, 1))


def _qjac(q):
    """q_w I + [q_v]x."""
    return q[:, 3, None, None] * np.eye(3, dtype=q.dtype) + skew(q[:, :3])


# ---------------------------------------------------------------- the four edges
def se3_edge(xi, xj, z, dtype=np.float64, jac=True):
    """EdgeSE3: e [n, 6] and, with jac, Ji, Jj [n, 6, 6]. The measurement's quaternion is normalized (any sign, any
    norm), the vertices' are taken as given."""
    xi, xj, z = _a(xi, dtype), _a(xj, dtype), _a(z, dtype)
    Ri, Rj, Rz = rot(xi[:, 3:], dtype, False), rot(xj[:, 3:], dtype, False), rot(z[:, 3:], dtype)
    Ra = _T(Rz)
    Rb, tb = _T(Ri) @ Rj, _mv(_T(Ri), xj[:, :3] - xi[:, :3])
    Re, te = Ra @ Rb, _mv(Ra, tb - z[:, :3])
    q = quat(Re)
    e = np.concatenate([te, q[:, :3]], 1)
    if not jac:
        return e
    n = len(e)
    Ji, Jj = np.zeros((n, 6, 6), dtype), np.zeros((n, 6, 6), dtype)
    Q = _qjac(q)
    Ji[:, :3, :3], Ji[:, :3, 3:], Ji[:, 3:, 3:] = -Ra, 2 * Ra @ skew(tb), -Q @ _T(Rb)
    Jj[:, :3, :3], Jj[:, 3:, 3:] = Re, Q
    return e, Ji, Jj


def se3_prior(x, z, offset=None, dtype=np.float64, jac=True):
    """EdgeSE3Prior with the sensor offset P [n, 7] (None: the identity): e [n, 6], J [n, 6, 6]."""
    x, z = _a(x, dtype), _a(z, dtype)
    P = _a(np.broadcast_to([0, 0, 0, 0, 0, 0, 1.0], x.shape) if offset is None else offset, dtype)
    Rx, Rz, Rp = rot(x[:, 3:], dtype, False), rot(z[:, 3:], dtype), rot(P[:, 3:], dtype)
    Ra = _T(Rz) @ Rx
    Re = Ra @ Rp
    te = _mv(_T(Rz), _mv(Rx, P[:, :3]) + x[:, :3] - z[:, :3])
    q = quat(Re)
    e = np.concatenate([te, q[:, :3]], 1)
    if not jac:
        return e
    J = np.zeros((len(e), 6, 6), dtype)
    J[:, :3, :3], J[:, :3, 3:], J[:, 3:, 3:] = Ra, -2 * Ra @ skew(P[:, :3]), _qjac(q) @ _T(Rp)
    return e, J


def se2_edge(xi, xj, z, dtype=np.float64, jac=True):
    """EdgeSE2: e [n, 3], Ji, Jj [n, 3, 3]."""
    xi, xj, z = _a(xi, dtype), _a(xj, dtype), _a(z, dtype)
    RiT, RzT = _T(rot2(xi[:, 2])), _T(rot2(z[:, 2]))
    d = xj[:, :2] - xi[:, :2]
    e = np.concatenate([_mv(RzT, _mv(RiT, d) - z[:, :2]), wrap(xj[:, 2] - xi[:, 2] - z[:, 2], dtype)[:, None]], 1)
    if not jac:
        return e
    n = len(e)
    c, s = np.cos(xi[:, 2]), np.sin(xi[:, 2])
    dRiT = np.stack([np.stack([-s, c], -1), np.stack([-c, -s], -1)], -2)  # d Ri^T / d theta
    Ji, Jj = np.zeros((n, 3, 3), dtype), np.zeros((n, 3, 3), dtype)
    Ji[:, :2, :2], Ji[:, :2, 2], Ji[:, 2, 2] = -RzT @ RiT, _mv(RzT, _mv(dRiT, d)), -1
    Jj[:, :2, :2], Jj[:, 2, 2] = RzT @ RiT, 1
    return e, Ji, Jj


def se2xy_edge(xi, l, z, dtype=np.float64, jac=True):
    """EdgeSE2PointXY: e [n, 2], Ji [n, 2, 3], Jj [n, 2, 2]."""
    xi, l, z = _a(xi, dtype), _a(l, dtype), _a(z, dtype)
    RiT = _T(rot2(xi[:, 2]))
    d = l - xi[:, :2]
    e = _mv(RiT, d) - z
    if not jac:
        return e
    c, s = np.cos(xi[:, 2]), np.sin(xi[:, 2])
    dRiT = np.stack([np.stack([-s, c], -1), np.stack([-c, -s], -1)], -2)
    Ji = np.concatenate([-RiT, _mv(dRiT, d)[:, :, None]], 2)
    return e, Ji, RiT.copy()


# ---------------------------------------------------------------- the five oplus maps
def oplus_xyz(est, u, dtype=np.float64):
    return _a(est, dtype) + _a(u, dtype)


oplus_xy = oplus_xyz


def oplus_se2(est, u, dtype=np.float64):
    est, u = _a(est, dtype), _a(u, dtype)
    return np.concatenate([est[:, :2] + u[:, :2], wrap(est[:, 2] + u[:, 2], dtype)[:, None]], 1)


def reorthogonalize(R):
    """approximateNearestOrthogonalMatrix: one step R - R (R^T R - I) / 2."""
    return R - (R @ (_T(R) @ R - np.eye(3, dtype=R.dtype))) / 2


def oplus_se3quat(R, t, u, dtype=np.float64, calls=0):
    """VertexSE3's oplus on the isometry (R [n, 3, 3], t [n, 3]): X * fromVectorMQT(u); `calls` is the number of
    oplus calls this vertex has had since its last re-orthogonalisation. Returns (R, t, calls)."""
    R, t, u = np.asarray(R, dtype), _a(t, dtype), _a(u, dtype)
    w2 = 1 - np.sum(u[:, 3:] * u[:, 3:], axis=1)
    qi = np.concatenate([u[:, 3:], np.sqrt(np.maximum(w2, 0))[:, None]], 1)
    inc = np.where((w2 < 0)[:, None, None], np.eye(3, dtype=dtype), rot(qi, dtype, False))
    Rn, tn = R @ inc, t + _mv(R, u[:, :3])
    calls += 1
    if calls > 1000:
        Rn, calls = reorthogonalize(Rn), 0
    return Rn, tn, calls


def se3_exp(u, dtype=np.float64):
    """SE3Quat::exp of u = (omega, upsilon): (R [n, 3, 3], t [n, 3])."""
    u = _a(u, dtype)
    th = np.sqrt(np.sum(u[:, :3] * u[:, :3], axis=1))
    W = skew(u[:, :3])
    small = th < 1e-5
    ths = np.where(small, 1, th)
    a = np.where(small, 1, np.sin(ths) / ths)
    b = np.where(small, dtype(1) / 2, (1 - np.cos(ths)) / (ths * ths))
    d = np.where(small, dtype(1) / 6, (ths - np.sin(ths)) / (ths * ths * ths))
    I = np.eye(3, dtype=dtype)
    R = I + a[:, None, None] * W + b[:, None, None] * (W @ W)
    V = I + b[:, None, None] * W + d[:, None, None] * (W @ W)
    return R, _mv(V, u[:, 3:])


def oplus_se3expmap(est, u, dtype=np.float64):
    """VertexSE3Expmap's oplus on est = (t, q): exp(u) * T, the quaternion normalized to w >= 0."""
    est = _a(est, dtype)
    R, t = se3_exp(u, dtype)
    q = qmul(quat(R), est[:, 3:])
    q = q / np.sqrt(np.sum(q * q, axis=1, keepdims=True))
    q = np.where(q[:, 3:4] < 0, -q, q)
    return np.concatenate([t + _mv(R, est[:, :3]), q], 1)


def oplus(vtype, est, u, dtype=np.float64):
    """One oplus of estimates in the external form (SE3 poses as t, q); V_SE3_QUAT without the call counter."""
    if vtype in (synth.V_XYZ, synth.V_XY):
        return oplus_xyz(est, u, dtype)
    if vtype == synth.V_SE2:
        return oplus_se2(est, u, dtype)
    if vtype == synth.V_SE3_EXPMAP:
        return oplus_se3expmap(est, u, dtype)
    if vtype == synth.V_SE3_QUAT:
        est = _a(est, dtype)
        R, t, _ = oplus_se3quat(rot(est[:, 3:], dtype, False), est[:, :3], u, dtype)
        return np.concatenate([t, quat(R)], 1)
    raise KeyError(vtype)


# ---------------------------------------------------------------- oplus cases
def oplus_cases(vtype):
    """(labels, est [m, .], u [m, .]): one free vertex per adversarial increment of the type."""
    rng = np.random.default_rng(4700 + vtype)
    if vtype in (synth.V_XYZ, synth.V_XY):
        d = 3 if vtype == synth.V_XYZ else 2
        est = rng.uniform(-5, 5, (3, d))
        u = np.array([[0.0] * d, [1e-9, -2.5, 1e6][:d], [-1e3, 3e-7, 0.125][:d]])
        return ["zero", "mixed", "large"], est, u
    if vtype == synth.V_SE2:
        th = np.array([[-PI / 2, -PI / 2], [PI / 2, PI / 2 - 1e-12], [3.0, 20.0], [-3.0, -17.5], [0.3, 0.4]])
        assert th[0].sum() == -PI  # lands on -pi exactly, in every precision
        t, ut = rng.uniform(-3, 3, (5, 2)), rng.uniform(-1, 1, (5, 2))
        return (["at -pi", "under pi", "turns+", "turns-", "inside"], np.concatenate([t, th[:, :1]], 1),
                np.concatenate([ut, th[:, 1:]], 1))
    if vtype == synth.V_SE3_QUAT:
        s = [0.0, 0.5, 0.98, 1.02, 4.0, 1e-4]
        dirs = rng.standard_normal((len(s), 3))
        dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
        u = np.concatenate([rng.uniform(-1, 1, (len(s), 3)), np.sqrt(s)[:, None] * dirs], 1)
        q = rng.standard_normal((len(s), 4))
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        return [f"|dq|^2={x:g}" for x in s], np.concatenate([rng.uniform(-2, 2, (len(s), 3)), q], 1), u
    if vtype == synth.V_SE3_EXPMAP:
        d0 = np.array([0.6, -0.48, 0.64])
        om = [0 * d0, 5e-6 * d0, 2e-5 * d0, 1.0 * d0]
        labels = ["th=0", "th=5e-6", "th=2e-5", "th=1"]
        for i, ax in enumerate("xyz"):
            for sg in (1.0, -1.0):
                a = np.full(3, 0.05)
                a[i] = sg
                om.append(2.6 * a / np.linalg.norm(a))
                labels.append(f"2.6 {'+' if sg > 0 else '-'}{ax}")
        om.append(np.array([0.1, -0.1, 2.0]))
        labels.append("w<0")
        m = len(om)
        u = np.concatenate([np.array(om), rng.uniform(-1, 1, (m, 3))], 1)
        R = axis_angle(rng.standard_normal((m, 3)), rng.uniform(0.2, 0.9, m))
        R[-1] = axis_angle([[0.0, 0.1, 1.0]], [2.0])[0]  # 2 rad about ~z, then 2 rad more: w = cos(2) < 0
        est = np.concatenate([rng.uniform(-2, 2, (m, 3)), quat(R)], 1)
        # the sign rule jumps where w = 0: every case stays clear of it, and the last one has w < 0
        Re, _ = se3_exp(u, LD)
        w = qmul(quat(Re), np.asarray(est[:, 3:], LD))[:, 3]
        assert np.all(np.abs(w) >= 0.02) and w[-1] < 0, w
        return labels, est, u
    raise KeyError(vtype)


# ---------------------------------------------------------------- pose helpers for the generators (float64)
def _unit(q):
    q = np.asarray(q, np.float64)
    return q / np.linalg.norm(q)


def pose_of(R, t):
    return np.concatenate([np.asarray(t, np.float64), quat(np.asarray(R, np.float64)[None])[0]])


def _spd(rng, D, n=1):
    A = np.eye(D) + 0.3 * rng.standard_normal((n, D, D))
    return A @ _T(A)


def branch_of(Re):
    """The label of an error rotation [3, 3]: 'tr+' when its trace is positive, else the axis of its largest diagonal
    entry with the sign of q_w as the diagonal formula yields it (the sign of w * q_axis, q the w >= 0 quaternion)."""
    Re = np.asarray(Re)
    if Re[0, 0] + Re[1, 1] + Re[2, 2] > 0:
        return "tr+"
    i = int(np.argmax(np.diag(Re)))
    q = quat(Re[None].astype(LD))[0]
    return "xyz"[i] + ("+" if q[i] > 0 else "-")


def _targets():
    """(label, error rotation) of the branch cases: 0.8 rad for 'tr+'; 2.6 rad about +-x, +-y, +-z tilted 0.2 rad off
    the axis; a pair at trace = +-1e-3; the last entry is the rotation of the 'wneg' case."""
    out = [("tr+", axis_angle([[0.3, -0.5, 0.8]], [0.8])[0])]
    for i, ax in enumerate("xyz"):
        for sg, name in ((1.0, "+"), (-1.0, "-")):
            a = np.zeros(3)
            a[i] = sg * np.cos(0.2)
            a[(i + 1) % 3], a[(i + 2) % 3] = np.sin(0.2) * 0.8, -np.sin(0.2) * 0.6
            out.append((ax + name, axis_angle([a], [2.6])[0]))
    for sg, name in ((1.0, "tr0+"), (-1.0, "tr0-")):
        out.append((name, axis_angle([[0.5, 0.4, -0.77]], [np.arccos((sg * 1e-3 - 1) / 2)])[0]))
    out.append(("wneg", axis_angle([[-0.6, 0.3, 0.5]], [1.1])[0]))
    return out


def _check_margins(Re):
    q = quat(np.asarray(Re, LD)[None])[0]
    ang = 2 * np.arccos(q[3])
    assert q[3] >= 0.02 and ang <= np.pi - 0.05, (q, ang)


def wneg_quat(k=0):
    """The 'wneg' measurement quaternion: w < 0, norm 1.3 (to rounding). Chosen so that q / |q|, evaluated in the
    order the loader and add_edges evaluate it, is a fixed point of that normalization: the three ways of entering the
    measurement then hand bit-identical matrices to the device. Returns (raw, normalized with w > 0)."""
    for j in range(k, 64):
        q = -1.3 * _unit([0.21 + 0.01 * j, -0.33, 0.4, 0.82])
        qn = -(q / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]))
        if np.sqrt(qn[0] * qn[0] + qn[1] * qn[1] + qn[2] * qn[2] + qn[3] * qn[3]) == 1.0:
            return q, qn
    raise AssertionError("no fixed point")


def se3_branch_cases():
    """[(label, Xi, Xj, Z)]: the seven LABELS first, then 'tr0+', 'tr0-' and 'wneg'. Xj = Xi Z E with E the wanted
    error (rotation from _targets, a translation of a few tenths)."""
    rng = np.random.default_rng(4101)
    out = []
    for k, (label, Te) in enumerate(_targets()):
        Ri = axis_angle([rng.standard_normal(3)], [0.4 + 0.3 * k])[0]
        ti = rng.uniform(-1, 1, 3)
        qz = wneg_quat()[0] if label == "wneg" else _unit(rng.standard_normal(4))
        Rz, tz = rot(qz)[0], rng.uniform(-1, 1, 3)
        te = rng.uniform(0.2, 0.5, 3) * np.array([1, -1, 1])
        Rj, tj = Ri @ Rz @ Te, ti + Ri @ (tz + Rz @ te)
        _check_margins(Te)
        out.append((label, pose_of(Ri, ti), pose_of(Rj, tj), np.concatenate([tz, qz])))
    return out


def prior_branch_cases():
    """[(label, X, Z, P)] for EdgeSE3Prior: error rotation Z^-1 X P = the targets, P a non-identity sensor offset."""
    rng = np.random.default_rng(4102)
    out = []
    for k, (label, Te) in enumerate(_targets()):
        qz = wneg_quat()[0] if label == "wneg" else _unit(rng.standard_normal(4))
        Rz, tz = rot(qz)[0], rng.uniform(-1, 1, 3)
        qp = _unit(rng.standard_normal(4))
        Rp, tp = rot(qp)[0], rng.uniform(-0.5, 0.5, 3)
        te = rng.uniform(0.2, 0.5, 3) * np.array([-1, 1, 1])
        Rx = Rz @ Te @ Rp.T
        tx = tz + Rz @ te - Rx @ tp
        _check_margins(Te)
        out.append((label, pose_of(Rx, tx), np.concatenate([tz, qz]), np.concatenate([tp, qp])))
    return out


SE2_ANGLES = (-PI, PI - 1e-12, 7.0, -9.5)


def se2_wrap_cases():
    """[(label, xi, xj, z)]: theta_i, theta_j from SE2_ANGLES, the measurement angle inside [-pi, pi) such that the
    error angle is +-0.7 .. 1.2 after a wrap upward ('up': thj - thi - thz < -pi) or downward ('down')."""
    rng = np.random.default_rng(4103)
    out = []
    pairs = [(0, 2), (2, 0), (1, 3), (3, 1), (2, 3), (3, 2)]
    for k, (a, b) in enumerate(pairs):
        thi, thj = SE2_ANGLES[a], SE2_ANGLES[b]
        r = (0.7 + 0.1 * k) * (-1) ** k
        thz = float(wrap(np.array(thj - thi - r)))
        raw = thj - thi - thz
        label = "up" if raw < -PI else ("down" if raw >= PI else "none")
        assert abs(float(wrap(np.array(raw)))) < PI - 0.3
        xi = np.array([*rng.uniform(-1, 1, 2), thi])
        xj = np.array([*(xi[:2] + rng.uniform(-1, 1, 2)), thj])
        out.append((label, xi, xj, np.array([*rng.uniform(-1, 1, 2), thz])))
    return out


def se2xy_wrap_cases():
    """[(label, xi, l, z)]: the pose angle on or outside the ends of [-pi, pi)."""
    rng = np.random.default_rng(4104)
    out = []
    for th in SE2_ANGLES:
        label = "outside" if not (-PI <= th < PI) else "edge"
        xi = np.array([*rng.uniform(-1, 1, 2), th])
        out.append((label, xi, xi[:2] + rng.uniform(-2, 2, 2), rng.uniform(-1, 1, 2)))
    return out


# ---------------------------------------------------------------- problems
def _vs(vtype, ids, est, fixed=None, marg=0):
    n = len(ids)
    fx = np.zeros(n, np.int32) if fixed is None else np.asarray(fixed, np.int32)
    return synth.VertexSet(vtype, np.asarray(ids, np.int32), np.asarray(est, np.float64).reshape(n, -1), fx,
                           np.full(n, marg, np.int32))


def _es(etype, v0, v1, meas, info, params=None):
    return synth.EdgeSet(etype, np.asarray(v0, np.int32), None if v1 is None else np.asarray(v1, np.int32),
                         np.asarray(meas, np.float64), np.asarray(info, np.float64),
                         None if params is None else np.asarray(params, np.float64))


def se3_problem(case, seed=0):
    """Two free VertexSE3 (ids 3, 8) and one EdgeSE3 with a non-diagonal information matrix."""
    _, xi, xj, z = case
    info = _spd(np.random.default_rng(500 + seed), 6)
    return synth.Problem("se3one", [_vs(synth.V_SE3_QUAT, [3, 8], [xi, xj])],
                         [_es(synth.E_SE3_QUAT, [3], [8], z[None], info)], 6, 0)


def prior_problem(case, seed=0):
    """One free VertexSE3 (id 5) and one EdgeSE3Prior with a sensor offset."""
    _, x, z, P = case
    info = _spd(np.random.default_rng(600 + seed), 6)
    return synth.Problem("priorone", [_vs(synth.V_SE3_QUAT, [5], [x])],
                         [_es(synth.E_SE3_PRIOR, [5], None, z[None], info, P[None])], 6, 0)


def se2_problem(case, seed=0):
    _, xi, xj, z = case
    info = _spd(np.random.default_rng(700 + seed), 3)
    return synth.Problem("se2one", [_vs(synth.V_SE2, [2, 6], [xi, xj])], [_es(synth.E_SE2, [2], [6], z[None], info)], 3, 0)


def se2xy_problem(case, seed=0):
    _, xi, l, z = case
    info = _spd(np.random.default_rng(800 + seed), 2)
    return synth.Problem("se2xyone", [_vs(synth.V_SE2, [4], [xi]), _vs(synth.V_XY, [9], [l], marg=1)],
                         [_es(synth.E_SE2_XY, [4], [9], z[None], info)], 3, 2)


def _anchors(nv):
    """Every 8th vertex of a chain is fixed: the solve stays well conditioned at every length, and the branch cases
    (a cycle of 7) meet a fixed vertex at both ends in turn."""
    fx = np.zeros(nv, np.int32)
    fx[::8] = 1
    return fx


def se3_chain(ne):
    """ne + 1 VertexSE3 in a chain whose k-th edge repeats se3 branch case k mod 7 (the seven LABELS): X_{k+1} =
    X_k Z_k E_k. ne = 1 keeps both vertices free."""
    cases = se3_branch_cases()[:7]
    rng = np.random.default_rng(4200 + ne)
    R, t = np.eye(3), np.zeros(3)
    est, meas, labels = [pose_of(R, t)], [], []
    for k in range(ne):
        label, xi, xj, z = cases[k % 7]
        e = se3_edge(xi, xj, z, LD, jac=False)[0].astype(np.float64)
        Re = rot(np.concatenate([e[3:], [np.sqrt(1 - e[3:] @ e[3:])]]))[0]
        tz = rng.uniform(-0.5, 0.5, 3)
        Rz = rot(z[3:])[0]
        R, t = R @ Rz @ Re, t + R @ (tz + Rz @ e[:3])
        est.append(pose_of(R, t))
        meas.append(np.concatenate([tz, z[3:]]))
        labels.append(label)
    fx = _anchors(ne + 1) if ne > 1 else None
    prob = synth.Problem(f"se3chain{ne}", [_vs(synth.V_SE3_QUAT, np.arange(ne + 1), est, fx)],
                         [_es(synth.E_SE3_QUAT, np.arange(ne), np.arange(1, ne + 1), meas, _spd(rng, 6, ne))], 6, 0)
    return prob, labels


def se2_chain(ne):
    """ne + 1 VertexSE2 in a chain; the vertex angles cycle through SE2_ANGLES in the order -pi, 7.0, -9.5, pi - 1e-12
    and stay as given (unwrapped); the measurement angles are made as in se2_wrap_cases, so that the error angles are
    +-0.7 .. 1.2 after a wrap. Returns (problem, wrap label per edge)."""
    rng = np.random.default_rng(4300 + ne)
    cyc = (0, 2, 3, 1)
    th = np.array([SE2_ANGLES[cyc[k % 4]] for k in range(ne + 1)])
    est = np.concatenate([np.cumsum(rng.uniform(-1, 1, (ne + 1, 2)), 0), th[:, None]], 1)
    i, j = np.arange(ne), np.arange(1, ne + 1)
    r = (0.7 + 0.1 * (i % 6)) * (-1.0) ** i
    thz = wrap(th[j] - th[i] - r)
    raw = th[j] - th[i] - thz
    labels = ["up" if x < -PI else ("down" if x >= PI else "none") for x in raw]
    assert np.all(np.abs(wrap(raw)) < PI - 0.3)
    z0 = np.concatenate([np.zeros((ne, 2)), thz[:, None]], 1)
    tz = se2_edge(est[i], est[j], z0, jac=False)[:, :2]  # Rz^T (Ri^T (tj - ti)): the translation error at tz = 0
    meas = np.concatenate([_mv(rot2(thz), tz) + 0.1 * rng.standard_normal((ne, 2)), thz[:, None]], 1)
    fx = _anchors(ne + 1) if ne > 1 else None
    prob = synth.Problem(f"se2chain{ne}", [_vs(synth.V_SE2, np.arange(ne + 1), est, fx)],
                         [_es(synth.E_SE2, i, j, meas, _spd(rng, 3, ne))], 3, 0)
    return prob, labels


def se2xy_fan(ne):
    """ne EdgeSE2PointXY: min(ne, 9) poses whose angles cycle through SE2_ANGLES (the first fixed when ne > 1), each
    landmark seen by up to three of them; landmarks marginalized (the 3/2 Schur path)."""
    rng = np.random.default_rng(4400 + ne)
    P = min(ne, 9)
    poses = np.array([[*rng.uniform(-2, 2, 2), SE2_ANGLES[p % 4]] for p in range(P)])
    nl = (ne + 2) // 3
    lms = rng.uniform(-3, 3, (nl, 2))
    v0 = np.array([(k + k // 3) % P for k in range(ne)])
    v1 = P + np.arange(ne) // 3
    e = se2xy_edge(poses[v0], lms[v1 - P], np.zeros((ne, 2)), jac=False)
    meas = e + 0.1 * rng.standard_normal((ne, 2))
    fx = np.zeros(P, np.int32)
    fx[0] = ne > 1
    return synth.Problem(f"se2xyfan{ne}", [_vs(synth.V_SE2, np.arange(P), poses, fx),
                                          _vs(synth.V_XY, P + np.arange(nl), lms, marg=1)],
                         [_es(synth.E_SE2_XY, v0, v1, meas, _spd(rng, 2, ne))], 3, 2)


# ---------------------------------------------------------------- dense normal equations
_VDIM = {synth.V_SE3_QUAT: 6, synth.V_SE2: 3, synth.V_XY: 2}


class Graph:
    """The dense system of a problem of the four edge types at its own estimates, in the hessian order: free
    non-marginalized vertices by id, then the free marginalized ones by id, only vertices that have an edge; a prior
    on a fixed vertex is inactive."""

    def __init__(self, prob):
        self.prob = prob
        self.est, self.dim, fixed, marg = {}, {}, {}, {}
        for vs in prob.vertices:
            for k, i in enumerate(vs.ids):
                self.est[int(i)], self.dim[int(i)] = vs.est[k], _VDIM[vs.vtype]
                fixed[int(i)], marg[int(i)] = int(vs.fixed[k]), int(vs.marginalized[k])
        has = set()
        for es in prob.edges:
            has.update(int(i) for i in es.v0)
            if es.v1 is not None:
                has.update(int(i) for i in es.v1)
        order = sorted((marg[i], i) for i in has if not fixed[i])
        self.off, o = {}, 0
        for m, i in order:
            self.off[i] = o
            o += self.dim[i]
        self.n = o
        self.npose = sum(self.dim[i] for m, i in order if not m)
        self.fixed = fixed

    def edges(self, es, dtype=np.float64):
        """(e, [(vertex ids, J), ...]) of an edge set."""
        xi = np.array([self.est[int(i)] for i in es.v0])
        if es.etype == synth.E_SE3_PRIOR:
            e, J = se3_prior(xi, es.meas, es.params, dtype)
            return e, [(es.v0, J)]
        xj = np.array([self.est[int(i)] for i in es.v1])
        f = {synth.E_SE3_QUAT: se3_edge, synth.E_SE2: se2_edge, synth.E_SE2_XY: se2xy_edge}[es.etype]
        e, Ji, Jj = f(xi, xj, es.meas, dtype)
        return e, [(es.v0, Ji), (es.v1, Jj)]

    def chi2(self, dtype=np.float64):
        c = dtype(0)
        for es in self.prob.edges:
            e, Js = self.edges(es, dtype)
            act = np.array([es.v1 is not None or not self.fixed[int(i)] for i in es.v0])
            c += np.einsum("ni,nij,nj->", e[act], np.asarray(es.info, dtype)[act], e[act])
        return c

    def dense_system(self, dtype=np.float64):
        H, b = np.zeros((self.n, self.n), dtype), np.zeros(self.n, dtype)
        for es in self.prob.edges:
            e, Js = self.edges(es, dtype)
            Om = np.asarray(es.info, dtype)
            We = np.einsum("nij,nj->ni", Om, e)
            for ia, Ja in Js:
                ga = np.einsum("nri,nr->ni", Ja, We)
                for ib, Jb in Js:
                    Hab = np.einsum("nri,nrs,nsj->nij", Ja, Om, Jb)
                    for k in range(len(e)):
                        a, c = int(ia[k]), int(ib[k])
                        if a in self.off and c in self.off:
                            oa, oc = self.off[a], self.off[c]
                            H[oa:oa + Hab.shape[1], oc:oc + Hab.shape[2]] += Hab[k]
                for k in range(len(e)):
                    a = int(ia[k])
                    if a in self.off:
                        b[self.off[a]:self.off[a] + ga.shape[1]] -= ga[k]
        return H, b


def solve(H, b, npose, lam, ld=0):
    """The solve at lambda: (Hschur, bschur, x); without landmarks Hschur = H + lam I and bschur = b."""
    n = len(b)
    Hd = H + lam * np.eye(n, dtype=H.dtype)
    if n == npose:
        return Hd, b.copy(), np.linalg.solve(Hd.astype(np.float64), b.astype(np.float64))
    Hpp, Hpl, Hll = Hd[:npose, :npose], Hd[:npose, npose:], Hd[npose:, npose:]
    Dinv = np.zeros_like(Hll)
    for o in range(0, n - npose, ld):
        Dinv[o:o + ld, o:o + ld] = np.linalg.inv(Hll[o:o + ld, o:o + ld].astype(np.float64))
    W = Hpl @ Dinv
    Hs, bs = Hpp - W @ Hpl.T, b[:npose] - W @ b[npose:]
    xp = np.linalg.solve(Hs.astype(np.float64), bs.astype(np.float64))
    return Hs, bs, np.concatenate([xp, Dinv @ (b[npose:] - Hpl.T @ xp)])


def numpy_stage(prob, lam):
    g = Graph(prob)
    H, b = g.dense_system()
    Hs, bs, x = solve(H, b, g.npose, lam, prob.landmark_dim)
    return dict(b=b, x=x, Hschur=Hs, bschur=bs, np=g.npose, n=g.n)


# ---------------------------------------------------------------- degree-ragged graphs (the vertex reduction)
def ragged_edges(nv, k, lanes, wide=False, hub=3):
    """Edge list (v0, v1) over vertices 0 .. nv-1: the circulant in which every vertex is joined to its next k
    neighbours (degree 2k), then vertex 1 cut down to degree 1, vertex 3 to lanes - 1 (if that is at least 1), vertex
    5 to lanes + 1, for the wide class vertex 7 to degree 7 and vertex 9 to 65; vertex 11 becomes a hub with `hub`
    times the base degree through parallel edges. Returns the int arrays and the degree of every vertex."""
    pairs = [(i, (i + d) % nv) for d in range(1, k + 1) for i in range(nv)]
    special = {1: 1, 5: lanes + 1}
    if lanes > 1:
        special[3] = lanes - 1
    if wide:
        special.update({7: 7, 9: 65})
    assert nv > 12
    for v, want in special.items():
        have = [p for p in pairs if v in p]
        # keep the first `want` edges of v that do not touch another special vertex or the hub
        keep, rest = [], []
        for p in have:
            o = p[0] if p[1] == v else p[1]
            (keep if len(keep) < want and o not in special and o != 11 else rest).append(p)
        if len(keep) < want:  # sparse base (k = 1): parallel edges to a plain neighbour make up the count
            keep += [(v, (v + nv // 2) % nv)] * (want - len(keep))
        pairs = [p for p in pairs if v not in p] + keep
    extra = hub * 2 * k - sum(11 in p for p in pairs)
    others = [v for v in range(nv) if v != 11 and v not in special]
    pairs += [(11, others[j % len(others)]) for j in range(max(extra, 0))]
    v0, v1 = np.array([p[0] for p in pairs], np.int32), np.array([p[1] for p in pairs], np.int32)
    deg = np.bincount(np.concatenate([v0, v1]), minlength=nv)
    return v0, v1, deg


def ragged_pose_graph(vtype, nv, k, lanes, wide=False, seed=0):
    """VertexSE3 / EdgeSE3 (dim 6) or VertexSE2 / EdgeSE2 (dim 3) over ragged_edges; the last vertex is fixed. Returns
    (problem, degrees of the free vertices)."""
    rng = np.random.default_rng(4500 + seed)
    v0, v1, deg = ragged_edges(nv, k, lanes, wide)
    ne = len(v0)
    if vtype == synth.V_SE3_QUAT:
        q = rng.standard_normal((nv, 4))
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        est = np.concatenate([rng.uniform(-3, 3, (nv, 3)), q], 1)
        e = se3_edge(est[v0], est[v1], np.broadcast_to([0, 0, 0, 0, 0, 0, 1.0], (ne, 7)), jac=False)
        # measurement = the relative pose times a small error: Z = D N^-1 with N = (0.1 t-noise, 0.05 q-noise)
        nq = np.concatenate([0.05 * rng.standard_normal((ne, 3)), np.ones((ne, 1))], 1)
        qd = np.concatenate([e[:, 3:], np.sqrt(1 - np.sum(e[:, 3:] ** 2, 1))[:, None]], 1)
        meas = np.concatenate([e[:, :3] + 0.1 * rng.standard_normal((ne, 3)), qmul(qd, nq)], 1)
        etype, D = synth.E_SE3_QUAT, 6
    else:
        est = np.concatenate([rng.uniform(-3, 3, (nv, 2)), rng.uniform(-np.pi, np.pi, (nv, 1))], 1)
        meas = se2_edge(est[v0], est[v1], np.zeros((ne, 3)), jac=False) + 0.05 * rng.standard_normal((ne, 3))
        etype, D = synth.E_SE2, 3
    fx = np.zeros(nv, np.int32)
    fx[-1] = 1
    prob = synth.Problem(f"ragged{D}_{lanes}", [_vs(vtype, np.arange(nv), est, fx)],
                         [_es(etype, v0, v1, meas, _spd(rng, D, ne))], D, 0)
    return prob, deg[:-1]


def ragged_landmark_graph(degrees, npose, seed=0):
    """XY landmarks under EdgeSE2PointXY with the given number of observing poses each (more than npose - 1: parallel
    edges); pose 0 is fixed, every pose is joined to the next by an EdgeSE2. Returns the problem."""
    rng = np.random.default_rng(4600 + seed)
    poses = np.concatenate([rng.uniform(-4, 4, (npose, 2)), rng.uniform(-np.pi, np.pi, (npose, 1))], 1)
    lms = rng.uniform(-4, 4, (len(degrees), 2))
    v0 = np.concatenate([(np.arange(d) + 3 * j) % npose for j, d in enumerate(degrees)])
    v1 = np.concatenate([np.full(d, npose + j) for j, d in enumerate(degrees)])
    ne = len(v0)
    meas = se2xy_edge(poses[v0], lms[v1 - npose], np.zeros((ne, 2)), jac=False) + 0.1 * rng.standard_normal((ne, 2))
    o0, o1 = np.arange(npose - 1), np.arange(1, npose)
    odo = se2_edge(poses[o0], poses[o1], np.zeros((npose - 1, 3)), jac=False) + 0.05 * rng.standard_normal((npose - 1, 3))
    fx = np.zeros(npose, np.int32)
    fx[0] = 1
    return synth.Problem(f"raggedxy{len(degrees)}", [_vs(synth.V_SE2, np.arange(npose), poses, fx),
                                                    _vs(synth.V_XY, npose + np.arange(len(degrees)), lms, marg=1)],
                         [_es(synth.E_SE2, o0, o1, odo, _spd(rng, 3, npose - 1)),
                          _es(synth.E_SE2_XY, v0, v1, meas, _spd(rng, 2, ne))], 3, 2)
