"""Synthetic problem generators for the BASELINE configs.

All generators are seeded with a counter-based RNG (numpy Philox), so the
oracle, the CPU baseline and the HIP backend see byte-identical inputs.  They
return a :class:`Problem` holding plain arrays in the C-ABI layout of
``include/g2o_hip.h`` (the same layout ``oracle/oracle.h`` accepts).

Recipes:
  * ``sphere``  - ``g2o/examples/sphere/create_sphere.cpp:40-231`` (SE3 pose graph,
    EDGE_SE3:QUAT), optionally with the extra lap f-2 loop closures of config C3.
  * ``se2_grid`` - SE2 lattice random walk with odometry plus up to 3 spatially
    local loop closures per pose (config C2).
  * ``slam2d``  - 2D landmark SLAM for BlockSolver_3_2 (VERTEX_SE2 poses, VERTEX_XY landmarks, EDGE_SE2
    odometry, EDGE_SE2_XY range-limited point observations), the shape of g2o/examples/tutorial_slam2d.
  * ``ba``      - BAL-style bundle adjustment after ``g2o/examples/ba/ba_demo.cpp:86-300``
    (VERTEX_SE3:EXPMAP cameras, VERTEX_XYZ points, EDGE_SE3_PROJECT_XYZ:EXPMAP),
    each point observed by exactly k cameras of a window of W consecutive ones.
  * ``ba_stereo`` - the same scene observed by a stereo rig (EdgeStereoSE3ProjectXYZ: u_l v u_r),
    all observations or a fraction of them (a mixed monocular + stereo graph).
  * ``expmap_pose_graph`` - a pose graph on the BA camera parameterisation (VERTEX_SE3:EXPMAP cameras joined by
    EDGE_SE3:EXPMAP odometry and loop closures).
  * ``pose_only`` / ``with_pose_only`` - pose optimisation: cameras observing points held in the edges
    (EdgeSE3ProjectXYZOnlyPose, EdgeStereoSE3ProjectXYZOnlyPose), alone or beside a BA problem's edges.
  * ``sba``     - the scene of ``ba`` in the sba vocabulary of ``g2o/examples/sba/sba_demo.cpp`` (VERTEX_CAM cameras
    holding their intrinsics, VERTEX_XYZ points, EDGE_PROJECT_P2MC or EDGE_PROJECT_P2SC).
  * ``slam3d_landmarks`` - 3D SLAM with landmarks (VERTEX_SE3:QUAT poses with EDGE_SE3:QUAT odometry, VERTEX_TRACKXYZ
    points seen through EDGE_SE3_TRACKXYZ / EDGE_PROJECT_DEPTH / EDGE_PROJECT_DISPARITY), the shape of
    g2o_simulator3d's output.
  * ``se3_offset_graph`` / ``se2_offset_graph`` - pose graphs measured between sensor frames (EDGE_SE3_OFFSET /
    EDGE_SE2_OFFSET with one or two distinct sensor offsets), the shape of g2o_simulator3d's pose sensor.
  * ``bearing_scene`` - bearing-only 2D landmark SLAM (EDGE_BEARING_SE2_XY; every landmark seen from several poses
    with parallax), the shape of g2o_simulator2d's bearing sensor.
  * ``gicp_pair`` / ``gicp_scans`` / ``gicp_sba`` - scan registration in the types_icp vocabulary (EDGE_V_V_GICP
    correspondences between VERTEX_SE3:QUAT scans, point-to-plane or plane-to-plane; Edge_XYZ_VSC stereo
    observations of marginalised points): the scenes of gicp_demo.cpp and gicp_sba_demo.cpp, and a ring of scans
    with many correspondences per scan pair.
  * ``sim3_pose_graph`` - a 7-DoF pose graph in the types/sim3 vocabulary (VERTEX_SIM3:EXPMAP keyframes joined by
    EDGE_SIM3:EXPMAP odometry and loop closures), the shape of a monocular essential graph with scale drift.
"""
from __future__ import annotations

import dataclasses
import math
from typing import List

import numpy as np

SEED = 20261015

# vertex / edge type codes (include/g2o_hip.h)
V_SE3_EXPMAP, V_XYZ, V_SE3_QUAT, V_SE2, V_XY = 1, 2, 3, 4, 5
# VertexCam (types_sba): x y z qx qy qz qw (camera-to-world) fx fy cx cy baseline
V_CAM = 6
E_SE3_PROJECT_XYZ, E_SE3_QUAT, E_SE2, E_SE2_XY = 1, 2, 3, 5
E_STEREO_SE3_PROJECT_XYZ = 6
# slam3d landmark edges: v0 a V_SE3_QUAT pose, v1 a V_XYZ point
E_SE3_XYZ, E_SE3_XYZ_DEPTH, E_SE3_XYZ_DISPARITY = 7, 8, 9
# unary edge types (priors): EdgeSet.v1 is None
E_SE2_PRIOR, E_SE2_XY_PRIOR, E_XY_PRIOR, E_SE3_PRIOR, E_XYZ_PRIOR = 16, 17, 18, 19, 20
# EdgeSE3Expmap between two V_SE3_EXPMAP cameras; the pose-only projections (unary, on a V_SE3_EXPMAP camera; params
# Xw fx fy cx cy, stereo + bf)
E_SE3_EXPMAP = 10
E_SE3_PROJECT_XYZ_ONLYPOSE, E_STEREO_SE3_PROJECT_XYZ_ONLYPOSE = 21, 22
# the sba types: v0 a V_XYZ point, v1 a V_CAM camera; no params (the intrinsics live in the vertex)
E_PROJECT_P2MC, E_PROJECT_P2SC = 11, 12
# EdgeSE3Offset / EdgeSE2Offset between two poses (params: the from vertex's sensor offset, then the to vertex's),
# EdgeSE2PointXYBearing from a V_SE2 pose to a V_XY point (one angle, no params)
E_SE3_OFFSET, E_SE2_OFFSET, E_SE2_XY_BEARING = 13, 14, 15
# g2o's own BA edges on a CameraParameters parameter: EdgeProjectXYZ2UV (u v), EdgeProjectXYZ2UVU (u v u_r); v0 a V_XYZ
# point, v1 a V_SE3_EXPMAP camera; params focal_length cx cy baseline
E_PROJECT_XYZ2UV, E_PROJECT_XYZ2UVU = 23, 24
# types_icp: Edge_V_V_GICP between two V_SE3_QUAT (meas pos0 normal0 pos1 normal1; params None = point-to-plane, or
# cov0 | cov1 packed upper = plane-to-plane), Edge_XYZ_VSC from a V_XYZ point to a V_SE3_QUAT camera (params fx fy cx
# cy baseline)
E_V_V_GICP, E_XYZ_VSC = 25, 26
# types/sim3: VertexSim3Expmap, estimate tx ty tz qx qy qz qw s (world->camera); EdgeSim3 between two of them, meas a
# Sim3 in the same layout, info 7x7 in (omega, upsilon, sigma) order
V_SIM3 = 7
E_SIM3 = 27
# EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ from a fixed V_XYZ point to a V_SIM3 (meas u v, info 2x2, no params: the
# intrinsics are camera 1 / camera 2 of the Sim3 vertex)
E_SIM3_PROJECT, E_SIM3_PROJECT_INVERSE = 28, 29
# examples/bal: VertexCameraBAL, estimate rx ry rz tx ty tz f k1 k2 (angle-axis, world->camera), dimension 9;
# EdgeObservationBAL from it (v0) to a V_XYZ point (v1), meas u v, info 2x2, no params
V_CAM_BAL = 8
E_OBSERVATION_BAL = 30
EST_DIM = {V_SE3_EXPMAP: 7, V_XYZ: 3, V_SE3_QUAT: 7, V_SE2: 3, V_XY: 2, V_CAM: 12, V_SIM3: 8, V_CAM_BAL: 9}
MEAS_DIM = {E_SE3_PROJECT_XYZ: 2, E_SE3_QUAT: 7, E_SE2: 3, E_SE2_XY: 2, E_STEREO_SE3_PROJECT_XYZ: 3,
            E_SE2_PRIOR: 3, E_SE2_XY_PRIOR: 2, E_XY_PRIOR: 2, E_SE3_PRIOR: 7, E_XYZ_PRIOR: 3,
            E_SE3_XYZ: 3, E_SE3_XYZ_DEPTH: 3, E_SE3_XYZ_DISPARITY: 3,
            E_SE3_EXPMAP: 7, E_SE3_PROJECT_XYZ_ONLYPOSE: 2, E_STEREO_SE3_PROJECT_XYZ_ONLYPOSE: 3,
            E_PROJECT_P2MC: 2, E_PROJECT_P2SC: 3, E_SE3_OFFSET: 7, E_SE2_OFFSET: 3, E_SE2_XY_BEARING: 1,
            E_PROJECT_XYZ2UV: 2, E_PROJECT_XYZ2UVU: 3, E_V_V_GICP: 12, E_XYZ_VSC: 3, E_SIM3: 8,
            E_SIM3_PROJECT: 2, E_SIM3_PROJECT_INVERSE: 2, E_OBSERVATION_BAL: 2}
ERR_DIM = {E_SE3_PROJECT_XYZ: 2, E_SE3_QUAT: 6, E_SE2: 3, E_SE2_XY: 2, E_STEREO_SE3_PROJECT_XYZ: 3,
           E_SE2_PRIOR: 3, E_SE2_XY_PRIOR: 2, E_XY_PRIOR: 2, E_SE3_PRIOR: 6, E_XYZ_PRIOR: 3,
           E_SE3_XYZ: 3, E_SE3_XYZ_DEPTH: 3, E_SE3_XYZ_DISPARITY: 3,
           E_SE3_EXPMAP: 6, E_SE3_PROJECT_XYZ_ONLYPOSE: 2, E_STEREO_SE3_PROJECT_XYZ_ONLYPOSE: 3,
           E_PROJECT_P2MC: 2, E_PROJECT_P2SC: 3, E_SE3_OFFSET: 6, E_SE2_OFFSET: 3, E_SE2_XY_BEARING: 1,
           E_PROJECT_XYZ2UV: 2, E_PROJECT_XYZ2UVU: 3, E_V_V_GICP: 3, E_XYZ_VSC: 3, E_SIM3: 7,
           E_SIM3_PROJECT: 2, E_SIM3_PROJECT_INVERSE: 2, E_OBSERVATION_BAL: 2}
# parameter values per edge of the types that take a record (EdgeSet.params; where None is allowed it is the identity)
PARAM_DIM = {E_SE3_PROJECT_XYZ: 4, E_STEREO_SE3_PROJECT_XYZ: 5, E_SE3_PRIOR: 7, E_SE3_XYZ: 7, E_SE3_XYZ_DEPTH: 11,
             E_SE3_XYZ_DISPARITY: 11, E_SE3_PROJECT_XYZ_ONLYPOSE: 7, E_STEREO_SE3_PROJECT_XYZ_ONLYPOSE: 8,
             E_SE3_OFFSET: 14, E_SE2_OFFSET: 6, E_PROJECT_XYZ2UV: 4, E_PROJECT_XYZ2UVU: 4, E_V_V_GICP: 12, E_XYZ_VSC: 5}
# the vertex type a unary edge type attaches to
PRIOR_VERTEX = {E_SE2_PRIOR: V_SE2, E_SE2_XY_PRIOR: V_SE2, E_XY_PRIOR: V_XY, E_SE3_PRIOR: V_SE3_QUAT, E_XYZ_PRIOR: V_XYZ}
# the same for the pose-only projections, and the binary projection each of them is the pose-only form of
POSE_ONLY_VERTEX = {E_SE3_PROJECT_XYZ_ONLYPOSE: V_SE3_EXPMAP, E_STEREO_SE3_PROJECT_XYZ_ONLYPOSE: V_SE3_EXPMAP}
POSE_ONLY_BINARY = {E_SE3_PROJECT_XYZ_ONLYPOSE: E_SE3_PROJECT_XYZ,
                    E_STEREO_SE3_PROJECT_XYZ_ONLYPOSE: E_STEREO_SE3_PROJECT_XYZ}


@dataclasses.dataclass
class VertexSet:
    vtype: int
    ids: np.ndarray          # int32 [n]
    est: np.ndarray          # float64 [n, EST_DIM]
    fixed: np.ndarray        # int32 [n]
    marginalized: np.ndarray  # int32 [n]


@dataclasses.dataclass
class EdgeSet:
    etype: int
    v0: np.ndarray      # int32 [n] vertex ids
    v1: np.ndarray | None  # int32 [n]; None for a unary edge type (a prior)
    meas: np.ndarray    # float64 [n, MEAS_DIM]
    info: np.ndarray    # float64 [n, D, D]
    # float64 [n, 4] (fx fy cx cy) for projection edges, [n, 5] (+ bf) for stereo, [n, 7] (offset x y z qx qy qz qw)
    # or None (identity) for SE3 priors and E_SE3_XYZ, [n, 11] (offset, fx fy cx cy) for E_SE3_XYZ_DEPTH / _DISPARITY,
    # [n, 7] (Xw fx fy cx cy) / [n, 8] (+ bf) for the pose-only projections, [n, 14] / [n, 6] (the from vertex's offset,
    # then the to vertex's; or None, both the identity) for E_SE3_OFFSET / E_SE2_OFFSET, [n, 4] (focal_length cx cy
    # baseline) for E_PROJECT_XYZ2UV / E_PROJECT_XYZ2UVU, [n, 12] (cov0 | cov1, packed upper triangles) or None
    # (point-to-plane) for E_V_V_GICP (info may be None when params is given), [n, 5] (fx fy cx cy baseline) for E_XYZ_VSC
    params: np.ndarray | None = None


@dataclasses.dataclass
class Problem:
    name: str
    vertices: List[VertexSet]
    edges: List[EdgeSet]
    pose_dim: int
    landmark_dim: int  # 0 when there is no Schur complement

    @property
    def num_vertices(self) -> int:
        return sum(len(v.ids) for v in self.vertices)

    @property
    def num_edges(self) -> int:
        return sum(len(e.v0) for e in self.edges)


def _rng(seed: int, stream: int) -> np.random.Generator:
    return np.random.Generator(np.random.Philox(key=seed + (stream << 32)))


# ---------------------------------------------------------------- rotations
def _axis_angle(axis: np.ndarray, angle: np.ndarray) -> np.ndarray:
    """Rotation matrices for unit axes [n,3] and angles [n] (Rodrigues)."""
    angle = np.asarray(angle, dtype=np.float64)
    k = axis / np.linalg.norm(axis, axis=-1, keepdims=True)
    K = np.zeros(k.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2] = -k[..., 2], k[..., 1]
    K[..., 1, 0], K[..., 1, 2] = k[..., 2], -k[..., 0]
    K[..., 2, 0], K[..., 2, 1] = -k[..., 1], k[..., 0]
    s, c = np.sin(angle)[..., None, None], np.cos(angle)[..., None, None]
    eye = np.broadcast_to(np.eye(3), K.shape)
    return eye + s * K + (1 - c) * (K @ K)


def rot_to_quat(R: np.ndarray) -> np.ndarray:
    """Rotation matrices [n,3,3] -> quaternions [n,4] as (x, y, z, w), w >= 0."""
    R = np.asarray(R)
    n = R.shape[0]
    q = np.zeros((n, 4))
    tr = R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]
    m0 = tr > 0
    t = np.sqrt(np.maximum(tr[m0] + 1.0, 0.0))
    w = 0.5 * t
    f = 0.5 / t
    q[m0, 0] = (R[m0, 2, 1] - R[m0, 1, 2]) * f
    q[m0, 1] = (R[m0, 0, 2] - R[m0, 2, 0]) * f
    q[m0, 2] = (R[m0, 1, 0] - R[m0, 0, 1]) * f
    q[m0, 3] = w
    for idx in np.nonzero(~m0)[0]:
        M = R[idx]
        i = 0
        if M[1, 1] > M[0, 0]:
            i = 1
        if M[2, 2] > M[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        tt = math.sqrt(M[i, i] - M[j, j] - M[k, k] + 1.0)
        c = [0.0, 0.0, 0.0]
        c[i] = 0.5 * tt
        tt = 0.5 / tt
        ww = (M[k, j] - M[j, k]) * tt
        c[j] = (M[j, i] + M[i, j]) * tt
        c[k] = (M[k, i] + M[i, k]) * tt
        q[idx] = [c[0], c[1], c[2], ww]
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[q[:, 3] < 0] *= -1
    return q


def quat_to_rot(q: np.ndarray) -> np.ndarray:
    """(x, y, z, w) [n,4] -> [n,3,3] (Eigen toRotationMatrix formula)."""
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    R = np.empty((q.shape[0], 3, 3))
    R[:, 0, 0] = 1 - (ty * y + tz * z)
    R[:, 0, 1] = tx * y - tz * w
    R[:, 0, 2] = tx * z + ty * w
    R[:, 1, 0] = tx * y + tz * w
    R[:, 1, 1] = 1 - (tx * x + tz * z)
    R[:, 1, 2] = ty * z - tx * w
    R[:, 2, 0] = tx * z - ty * w
    R[:, 2, 1] = ty * z + tx * w
    R[:, 2, 2] = 1 - (tx * x + ty * y)
    return R


def _iso_vec(R: np.ndarray, t: np.ndarray) -> np.ndarray:
    q = rot_to_quat(R)
    return np.concatenate([t, q], axis=1)


# ---------------------------------------------------------------- SE3 sphere
def sphere(nodes_per_level: int = 50, laps: int = 50, radius: float = 100.0, extra_lap2: bool = False,
           noise_t=(0.01, 0.01, 0.01), noise_q=(0.005, 0.005, 0.005), seed: int = SEED) -> Problem:
    """create_sphere.cpp:40-231; ``extra_lap2`` adds lap f-2 offset-0 closures (config C3)."""
    npl = nodes_per_level
    N = npl * laps
    ids = np.arange(N)
    f = ids // npl
    n = ids % npl
    idp1 = ids + 1  # create_sphere uses the post-incremented id in roty (:104-106)
    rz = _axis_angle(np.tile([0.0, 0.0, 1.0], (N, 1)), -math.pi + 2 * n * math.pi / npl)
    ry = _axis_angle(np.tile([0.0, 1.0, 0.0], (N, 1)), -0.5 * math.pi + idp1 * math.pi / (laps * npl))
    Rt = rz @ ry
    tt = Rt @ np.array([radius, 0.0, 0.0])
    e_from: list = [np.arange(0, N - 1)]
    e_to: list = [np.arange(1, N)]
    for ff in range(1, laps):
        nn = np.arange(npl)
        for off in (-1, 0, 1):
            if ff == laps - 1 and off == 1:
                continue
            e_from.append((ff - 1) * npl + nn)
            e_to.append(ff * npl + nn + off)
    if extra_lap2:
        for ff in range(2, laps):
            nn = np.arange(npl)
            e_from.append((ff - 2) * npl + nn)
            e_to.append(ff * npl + nn)
    a = np.concatenate(e_from)
    b = np.concatenate(e_to)
    # ground-truth relative transforms prev^-1 * cur
    Rrel = np.transpose(Rt[a], (0, 2, 1)) @ Rt[b]
    trel = np.einsum("nji,nj->ni", Rt[a], tt[b] - tt[a])
    # noise (create_sphere.cpp:161-182)
    rng = _rng(seed, 1)
    m = len(a)
    qn = rng.standard_normal((m, 3)) * np.asarray(noise_q)
    qw = 1.0 - np.linalg.norm(qn, axis=1)
    qw = np.maximum(qw, 0.0)
    qnoise = np.concatenate([qn, qw[:, None]], axis=1)
    qnoise /= np.linalg.norm(qnoise, axis=1, keepdims=True)
    gtq = rot_to_quat(Rrel)
    # gtQuat * noise
    x1, y1, z1, w1 = gtq.T
    x2, y2, z2, w2 = qnoise.T
    qm = np.stack([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                   w1 * y2 + y1 * w2 + z1 * x2 - x1 * z2,
                   w1 * z2 + z1 * w2 + x1 * y2 - y1 * x2,
                   w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2], axis=1)
    qm /= np.linalg.norm(qm, axis=1, keepdims=True)
    qm[qm[:, 3] < 0] *= -1
    tm = trel + rng.standard_normal((m, 3)) * np.asarray(noise_t)
    meas = np.concatenate([tm, qm], axis=1)
    info = np.zeros((6, 6))
    info[0:3, 0:3] = np.diag(1.0 / np.square(noise_t))
    info[3:6, 3:6] = np.diag(1.0 / np.square(noise_q))
    # initial estimate: chain the (noisy) odometry from vertex 0 (:184-191)
    Rm = quat_to_rot(qm[: N - 1])
    Rc = np.empty((N, 3, 3))
    tc = np.empty((N, 3))
    Rc[0], tc[0] = Rt[0], tt[0]
    for i in range(1, N):
        Rc[i] = Rc[i - 1] @ Rm[i - 1]
        tc[i] = Rc[i - 1] @ tm[i - 1] + tc[i - 1]
    est = _iso_vec(Rc, tc)
    fixed = np.zeros(N, np.int32)
    fixed[0] = 1
    verts = VertexSet(V_SE3_QUAT, ids.astype(np.int32), est, fixed, np.zeros(N, np.int32))
    edges = EdgeSet(E_SE3_QUAT, a.astype(np.int32), b.astype(np.int32), meas, np.broadcast_to(info, (m, 6, 6)).copy())
    name = f"sphere{npl}x{laps}" + ("_lap2" if extra_lap2 else "")
    return Problem(name, [verts], [edges], 6, 0)


# ---------------------------------------------------------------- SE2 grid
def _se2_compose(a, b):
    c, s = np.cos(a[..., 2]), np.sin(a[..., 2])
    x = a[..., 0] + c * b[..., 0] - s * b[..., 1]
    y = a[..., 1] + s * b[..., 0] + c * b[..., 1]
    th = np.mod(a[..., 2] + b[..., 2] + np.pi, 2 * np.pi) - np.pi
    return np.stack([x, y, th], axis=-1)


def _se2_between(a, b):
    c, s = np.cos(a[..., 2]), np.sin(a[..., 2])
    dx, dy = b[..., 0] - a[..., 0], b[..., 1] - a[..., 1]
    th = np.mod(b[..., 2] - a[..., 2] + np.pi, 2 * np.pi) - np.pi
    return np.stack([c * dx + s * dy, -s * dx + c * dy, th], axis=-1)


def se2_grid(num_poses: int = 1000, loops_per_pose: int = 3, radius: float = 2.0,
             noise=(0.05, 0.05, 0.02), seed: int = SEED) -> Problem:
    """SE2 lattice random walk (config C2): odometry + up to ``loops_per_pose``
    closures to the most recent earlier poses within ``radius`` (excluding i-1)."""
    rng = _rng(seed, 2)
    N = num_poses
    turns = rng.choice([-1, 0, 0, 1], size=N)
    heading = np.zeros(N, np.int64)
    pos = np.zeros((N, 2), np.int64)
    dirs = np.array([[1, 0], [0, 1], [-1, 0], [0, -1]])
    for i in range(1, N):
        heading[i] = (heading[i - 1] + turns[i]) % 4
        pos[i] = pos[i - 1] + dirs[heading[i]]
    th = heading * (np.pi / 2)
    th = np.mod(th + np.pi, 2 * np.pi) - np.pi
    gt = np.stack([pos[:, 0].astype(float), pos[:, 1].astype(float), th], axis=1)
    a_list = [np.arange(N - 1)]
    b_list = [np.arange(1, N)]
    cells: dict = {}
    r = int(math.ceil(radius))
    la, lb = [], []
    for i in range(N):
        px, py = int(pos[i, 0]), int(pos[i, 1])
        cand = []
        for dx in range(-r, r + 1):
            for dy in range(-r, r + 1):
                if dx * dx + dy * dy > radius * radius:
                    continue
                for j in cells.get((px + dx, py + dy), ()):
                    if j < i - 1:
                        cand.append(j)
        if cand:
            cand = sorted(set(cand))[-loops_per_pose:]
            for j in cand:
                la.append(j)
                lb.append(i)
        cells.setdefault((px, py), []).append(i)
        lst = cells[(px, py)]
        if len(lst) > 8:
            del lst[0]
    a_list.append(np.asarray(la, np.int64))
    b_list.append(np.asarray(lb, np.int64))
    a = np.concatenate(a_list)
    b = np.concatenate(b_list)
    rel = _se2_between(gt[a], gt[b])
    m = len(a)
    nz = rng.standard_normal((m, 3)) * np.asarray(noise)
    meas = rel + nz
    meas[:, 2] = np.mod(meas[:, 2] + np.pi, 2 * np.pi) - np.pi
    info = np.diag(1.0 / np.square(noise))
    est = np.empty((N, 3))
    est[0] = gt[0]
    for i in range(1, N):
        est[i] = _se2_compose(est[i - 1], meas[i - 1])
    fixed = np.zeros(N, np.int32)
    fixed[0] = 1
    verts = VertexSet(V_SE2, np.arange(N, dtype=np.int32), est, fixed, np.zeros(N, np.int32))
    edges = EdgeSet(E_SE2, a.astype(np.int32), b.astype(np.int32), meas, np.broadcast_to(info, (m, 3, 3)).copy())
    return Problem(f"se2grid{N}", [verts], [edges], 3, 0)


# ---------------------------------------------------------------- 2D landmark SLAM (BlockSolver_3_2)
def slam2d(num_poses: int = 1000, landmarks_per_cell: float = 1.0, sensor_range: float = 2.5,
           max_obs_per_pose: int = 8, odo_noise=(0.05, 0.05, 0.01), point_noise=(0.05, 0.05),
           seed: int = SEED) -> Problem:
    """SE2 lattice random walk (as ``se2_grid``) with XY landmarks scattered over the visited area
    (``landmarks_per_cell`` per unit cell); every pose observes up to ``max_obs_per_pose`` nearest landmarks
    within ``sensor_range`` (EdgeSE2PointXY: z = x_i^-1 * l + noise), consecutive poses are joined by EdgeSE2
    odometry. Landmarks nobody observes are dropped; pose 0 is fixed; landmarks are marginalised (Schur).
    Initial estimates: chained noisy odometry for the poses, each landmark from its first observation."""
    rng = _rng(seed, 4)
    N = num_poses
    turns = rng.choice([-1, 0, 0, 1], size=N)
    heading = np.zeros(N, np.int64)
    pos = np.zeros((N, 2), np.int64)
    dirs = np.array([[1, 0], [0, 1], [-1, 0], [0, -1]])
    for i in range(1, N):
        heading[i] = (heading[i - 1] + turns[i]) % 4
        pos[i] = pos[i - 1] + dirs[heading[i]]
    th = np.mod(heading * (np.pi / 2) + np.pi, 2 * np.pi) - np.pi
    gt = np.stack([pos[:, 0].astype(float), pos[:, 1].astype(float), th], axis=1)
    # landmarks: uniform over the cells within sensor range of the trajectory
    r = int(math.ceil(sensor_range))
    cells = {(int(x) + dx, int(y) + dy) for x, y in pos for dx in range(-r, r + 1) for dy in range(-r, r + 1)}
    cells = sorted(cells)
    nper = rng.poisson(landmarks_per_cell, size=len(cells))
    lm = np.concatenate([np.asarray(c, float)[None] + rng.random((k, 2)) for c, k in zip(cells, nper) if k > 0])
    grid: dict = {}
    for j, (x, y) in enumerate(lm):
        grid.setdefault((int(math.floor(x)), int(math.floor(y))), []).append(j)
    oa, ob = [], []
    for i in range(N):
        px, py = gt[i, 0], gt[i, 1]
        cand = [j for dx in range(-r - 1, r + 2) for dy in range(-r - 1, r + 2)
                for j in grid.get((int(math.floor(px)) + dx, int(math.floor(py)) + dy), ())]
        if not cand:
            continue
        cand = np.asarray(cand)
        d2 = (lm[cand, 0] - px) ** 2 + (lm[cand, 1] - py) ** 2
        keep = cand[d2 <= sensor_range ** 2]
        keep = keep[np.argsort(d2[d2 <= sensor_range ** 2], kind="stable")][:max_obs_per_pose]
        for j in np.sort(keep):
            oa.append(i)
            ob.append(j)
    oa = np.asarray(oa, np.int64)
    ob = np.asarray(ob, np.int64)
    used = np.unique(ob)
    remap = -np.ones(len(lm), np.int64)
    remap[used] = np.arange(len(used))
    lm = lm[used]
    ob = remap[ob]
    L = len(lm)
    # measurements
    c, s_ = np.cos(gt[oa, 2]), np.sin(gt[oa, 2])
    dx, dy = lm[ob, 0] - gt[oa, 0], lm[ob, 1] - gt[oa, 1]
    zo = np.stack([c * dx + s_ * dy, -s_ * dx + c * dy], axis=1) + rng.standard_normal((len(oa), 2)) * np.asarray(point_noise)
    a = np.arange(N - 1)
    rel = _se2_between(gt[a], gt[a + 1])
    zodo = rel + rng.standard_normal((N - 1, 3)) * np.asarray(odo_noise)
    zodo[:, 2] = np.mod(zodo[:, 2] + np.pi, 2 * np.pi) - np.pi
    est = np.empty((N, 3))
    est[0] = gt[0]
    for i in range(1, N):
        est[i] = _se2_compose(est[i - 1], zodo[i - 1])
    lest = np.zeros((L, 2))
    seen = np.zeros(L, bool)
    for k in range(len(oa)):
        j = ob[k]
        if seen[j]:
            continue
        seen[j] = True
        i = oa[k]
        cc, ss = math.cos(est[i, 2]), math.sin(est[i, 2])
        lest[j] = [est[i, 0] + cc * zo[k, 0] - ss * zo[k, 1], est[i, 1] + ss * zo[k, 0] + cc * zo[k, 1]]
    fixed = np.zeros(N, np.int32)
    fixed[0] = 1
    pose_ids = np.arange(N, dtype=np.int32)
    lm_ids = (N + np.arange(L)).astype(np.int32)
    poses = VertexSet(V_SE2, pose_ids, est, fixed, np.zeros(N, np.int32))
    points = VertexSet(V_XY, lm_ids, lest, np.zeros(L, np.int32), np.ones(L, np.int32))
    odo = EdgeSet(E_SE2, pose_ids[a], pose_ids[a + 1], zodo, np.broadcast_to(np.diag(1.0 / np.square(odo_noise)), (N - 1, 3, 3)).copy())
    obs = EdgeSet(E_SE2_XY, pose_ids[oa], lm_ids[ob], zo, np.broadcast_to(np.diag(1.0 / np.square(point_noise)), (len(oa), 2, 2)).copy())
    return Problem(f"slam2d{N}x{L}", [poses, points], [odo, obs], 3, 2)


# ---------------------------------------------------------------- BA
def _small_rot(rng, n, sigma):
    axis = rng.standard_normal((n, 3))
    ang = rng.standard_normal(n) * sigma
    return _axis_angle(axis, ang)


def _ba_scene(num_cameras, num_points, obs_per_point, window, pixel_noise, cam_rot_noise, cam_trans_noise,
              point_noise, fixed_cameras, seed):
    """The scene of :func:`ba`: the problem and, per observation, the true point in its camera's frame and the true
    (noise-free) projection.  Every random draw is ba()'s, in ba()'s order."""
    rng = _rng(seed, 3)
    C, P, k = num_cameras, num_points, obs_per_point
    W = min(window, C)
    k = min(k, W)
    centers = np.stack([np.arange(C) * 0.04, np.zeros(C), np.zeros(C)], axis=1)
    Rw = _small_rot(rng, C, 0.02)        # world->cam rotation
    tw = -np.einsum("nij,nj->ni", Rw, centers)
    ws = rng.integers(0, C - W + 1, size=P)
    # k distinct cameras of the window: argsort of random keys
    keys = rng.random((P, W))
    sel = np.sort(np.argsort(keys, axis=1)[:, :k], axis=1)
    cams = ws[:, None] + sel              # [P, k] sorted camera indices
    px = centers[ws, 0] + rng.random(P) * (W - 1) * 0.04
    pts = np.stack([px, rng.random(P) * 2 - 1, 3.0 + 2.0 * rng.random(P)], axis=1)
    fx = fy = 1000.0
    cx, cy = 320.0, 240.0
    cflat = cams.reshape(-1)
    pflat = np.repeat(np.arange(P), k)
    pc = np.einsum("nij,nj->ni", Rw[cflat], pts[pflat]) + tw[cflat]
    uv = np.stack([pc[:, 0] / pc[:, 2] * fx + cx, pc[:, 1] / pc[:, 2] * fy + cy], axis=1)
    uv_true = uv.copy()
    uv += rng.standard_normal(uv.shape) * pixel_noise
    # initial estimates
    dR = _small_rot(rng, C, cam_rot_noise)
    R0 = dR @ Rw
    t0 = tw + rng.standard_normal((C, 3)) * cam_trans_noise
    nf = min(fixed_cameras, C)
    R0[:nf], t0[:nf] = Rw[:nf], tw[:nf]
    cam_est = np.concatenate([t0, rot_to_quat(R0)], axis=1)
    pt_est = pts + rng.standard_normal(pts.shape) * point_noise
    cam_ids = np.arange(C, dtype=np.int32)
    pt_ids = (C + np.arange(P)).astype(np.int32)
    fixed = np.zeros(C, np.int32)
    fixed[:nf] = 1
    cams_v = VertexSet(V_SE3_EXPMAP, cam_ids, cam_est, fixed, np.zeros(C, np.int32))
    pts_v = VertexSet(V_XYZ, pt_ids, pt_est, np.zeros(P, np.int32), np.ones(P, np.int32))
    m = len(cflat)
    info = np.broadcast_to(np.eye(2), (m, 2, 2)).copy()
    params = np.broadcast_to(np.array([fx, fy, cx, cy]), (m, 4)).copy()
    edges = EdgeSet(E_SE3_PROJECT_XYZ, pt_ids[pflat], cam_ids[cflat], uv, info, params)
    return Problem(f"ba{C}x{P}k{k}w{W}", [cams_v, pts_v], [edges], 6, 3), pc, uv_true


def ba(num_cameras: int = 1000, num_points: int = 100_000, obs_per_point: int = 10, window: int = 64,
       pixel_noise: float = 1.0, cam_rot_noise: float = 0.002, cam_trans_noise: float = 0.01,
       point_noise: float = 0.05, fixed_cameras: int = 2, seed: int = SEED) -> Problem:
    """BAL-style synthetic BA (config C4/C5).  Camera i sits at x = 0.04 i on a line
    (ba_demo.cpp:216-231) with a small random attitude; every point is seen by
    exactly ``obs_per_point`` distinct cameras drawn from a window of ``window``
    consecutive cameras.  fx = fy = 1000, cx = 320, cy = 240, Omega = I2.
    The first ``fixed_cameras`` cameras are fixed: one fixed camera leaves the
    monocular scale unobservable (rank-deficient Schur system), two fix it."""
    return _ba_scene(num_cameras, num_points, obs_per_point, window, pixel_noise, cam_rot_noise, cam_trans_noise,
                     point_noise, fixed_cameras, seed)[0]


def ba_stereo(num_cameras: int = 1000, num_points: int = 100_000, obs_per_point: int = 10, window: int = 64,
              pixel_noise: float = 1.0, cam_rot_noise: float = 0.002, cam_trans_noise: float = 0.01,
              point_noise: float = 0.05, fixed_cameras: int = 2, seed: int = SEED, bf: float = 100.3,
              stereo_fraction: float = 1.0, disparity_noise: float = 1.0, info: np.ndarray | None = None) -> Problem:
    """The scene of :func:`ba` (same arguments, same cameras, points, estimates and left-image measurements) seen by a
    stereo rig: EdgeStereoSE3ProjectXYZ observations (u_l, v, u_r) with u_r = u_true - bf / z_true + noise, the noise
    (sigma ``disparity_noise``) from an rng stream of its own.  params are fx fy cx cy bf; ``info`` is the 3x3
    information of every stereo edge (default I3).  With ``stereo_fraction`` < 1 that fraction of the observations
    (chosen at random, again from a stream of its own) is stereo and the rest stay monocular in a second EdgeSet: the
    mixed graph of a stereo SLAM system's local BA.  A stereo rig observes the scale, so one fixed camera is enough."""
    prob, pc, uv_true = _ba_scene(num_cameras, num_points, obs_per_point, window, pixel_noise, cam_rot_noise,
                                  cam_trans_noise, point_noise, fixed_cameras, seed)
    mono = prob.edges[0]
    m = len(mono.v0)
    ur = uv_true[:, 0] - bf / pc[:, 2] + _rng(seed, 5).standard_normal(m) * disparity_noise
    if stereo_fraction >= 1.0:
        st = np.ones(m, bool)
    else:
        st = _rng(seed, 6).random(m) < stereo_fraction
    ns = int(st.sum())
    meas = np.stack([mono.meas[st, 0], mono.meas[st, 1], ur[st]], axis=1)
    om = np.eye(3) if info is None else np.asarray(info, np.float64).reshape(3, 3)
    params = np.concatenate([mono.params[st], np.full((ns, 1), float(bf))], axis=1)
    edges = [EdgeSet(E_STEREO_SE3_PROJECT_XYZ, mono.v0[st].copy(), mono.v1[st].copy(), meas,
                     np.broadcast_to(om, (ns, 3, 3)).copy(), params)]
    if ns < m:
        edges.append(EdgeSet(E_SE3_PROJECT_XYZ, mono.v0[~st].copy(), mono.v1[~st].copy(), mono.meas[~st].copy(),
                             mono.info[~st].copy(), mono.params[~st].copy()))
    return Problem(prob.name + f"_stereo{stereo_fraction:g}", prob.vertices, edges, 6, 3)


def sba(num_cameras: int = 1000, num_points: int = 100_000, obs_per_point: int = 10, window: int = 64,
        stereo: bool = False, pixel_noise: float = 1.0, cam_rot_noise: float = 0.002, cam_trans_noise: float = 0.01,
        point_noise: float = 0.05, fixed_cameras: int | None = None, seed: int = SEED, baseline: float = 0.1,
        disparity_noise: float = 1.0) -> Problem:
    """The scene of :func:`ba` in the sba types: V_CAM cameras (the camera-to-world inverse of ba()'s estimates, with
    fx fy cx cy and ``baseline`` in the vertex), the same points and left-image measurements, observed through
    EdgeProjectP2MC or, with ``stereo``, EdgeProjectP2SC (u_r = u_true - fx * baseline / z_true + noise, the noise from
    an rng stream of its own).  Omega = I.  Two cameras are fixed for monocular graphs, one for stereo ones (a stereo
    rig observes the scale), unless ``fixed_cameras`` says otherwise."""
    nf = (1 if stereo else 2) if fixed_cameras is None else fixed_cameras
    prob, pc, uv_true = _ba_scene(num_cameras, num_points, obs_per_point, window, pixel_noise, cam_rot_noise,
                                  cam_trans_noise, point_noise, nf, seed)
    cams, pts = prob.vertices
    mono = prob.edges[0]
    fx, fy, cx, cy = mono.params[0]
    # world->cam (t, q) -> cam->world: R^T, -R^T t
    Rcw = np.transpose(quat_to_rot(cams.est[:, 3:7]), (0, 2, 1))
    tcw = -np.einsum("nij,nj->ni", Rcw, cams.est[:, 0:3])
    C = len(cams.ids)
    est = np.concatenate([tcw, rot_to_quat(Rcw), np.broadcast_to([fx, fy, cx, cy, float(baseline)], (C, 5))], axis=1)
    cams_v = VertexSet(V_CAM, cams.ids, est, cams.fixed, cams.marginalized)
    m = len(mono.v0)
    if stereo:
        ur = uv_true[:, 0] - fx * baseline / pc[:, 2] + _rng(seed, 5).standard_normal(m) * disparity_noise
        meas = np.stack([mono.meas[:, 0], mono.meas[:, 1], ur], axis=1)
        edges = EdgeSet(E_PROJECT_P2SC, mono.v0, mono.v1, meas, np.broadcast_to(np.eye(3), (m, 3, 3)).copy(), None)
    else:
        edges = EdgeSet(E_PROJECT_P2MC, mono.v0, mono.v1, mono.meas, mono.info, None)
    return Problem("s" + prob.name + ("_stereo" if stereo else ""), [cams_v, pts], [edges], 6, 3)


def sba_twin(prob: Problem) -> Problem:
    """The host-Jacobian twin of a graph with sba edges: every E_PROJECT_P2MC / E_PROJECT_P2SC set as an E_HOSTJ(2) /
    E_HOSTJ(3) set (32 + D) between the same vertices with the same information; the caller supplies the payload."""
    edges = []
    for es in prob.edges:
        if es.etype in (E_PROJECT_P2MC, E_PROJECT_P2SC):
            edges.append(EdgeSet(32 + ERR_DIM[es.etype], es.v0.copy(), es.v1.copy(), None, es.info.copy(), None))
        else:
            edges.append(es)
    return Problem(prob.name + "/hostj", list(prob.vertices), edges, prob.pose_dim, prob.landmark_dim)


def ba_camparams(num_cameras: int = 1000, num_points: int = 100_000, obs_per_point: int = 10, window: int = 64,
                 stereo: bool = False, stereo_fraction: float | None = None, focal: float = 1000.0,
                 baseline: float = 0.1, pixel_noise: float = 1.0, cam_rot_noise: float = 0.002,
                 cam_trans_noise: float = 0.01, point_noise: float = 0.05, fixed_cameras: int | None = None,
                 seed: int = SEED, disparity_noise: float = 1.0, info: np.ndarray | None = None) -> Problem:
    """The scene of :func:`ba` (same cameras, points, estimates and pixel noise) in g2o's own BA types, as upstream
    ba_demo builds it: EdgeProjectXYZ2UV observations (u, v) or, with ``stereo``, EdgeProjectXYZ2UVU ones (u, v, u_r)
    with u_r = (x - baseline) / z * focal + cx + noise (the noise, sigma ``disparity_noise``, from ba_stereo's stream).
    Every edge names one CameraParameters record ``focal cx cy baseline`` (cx = 320, cy = 240).  ``info`` is the
    information of every stereo edge (default I3).  With ``stereo_fraction`` that fraction of the observations (chosen
    as ba_stereo chooses them) is XYZ2UVU and the rest XYZ2UV in a second EdgeSet.  Two cameras are fixed for a purely
    monocular graph, one otherwise, unless ``fixed_cameras`` says otherwise."""
    frac = (1.0 if stereo else 0.0) if stereo_fraction is None else float(stereo_fraction)
    nf = (2 if frac <= 0.0 else 1) if fixed_cameras is None else fixed_cameras
    prob, pc, uv_true = _ba_scene(num_cameras, num_points, obs_per_point, window, pixel_noise, cam_rot_noise,
                                  cam_trans_noise, point_noise, nf, seed)
    mono = prob.edges[0]
    m = len(mono.v0)
    cx, cy = mono.params[0, 2], mono.params[0, 3]
    f, b = float(focal), float(baseline)
    noise = mono.meas - uv_true  # _ba_scene's pixel noise, whatever its focal length
    uv = np.stack([pc[:, 0] / pc[:, 2] * f + cx, pc[:, 1] / pc[:, 2] * f + cy], axis=1) + noise
    ur = (pc[:, 0] - b) / pc[:, 2] * f + cx + _rng(seed, 5).standard_normal(m) * disparity_noise
    if frac >= 1.0:
        st = np.ones(m, bool)
    elif frac <= 0.0:
        st = np.zeros(m, bool)
    else:
        st = _rng(seed, 6).random(m) < frac
    ns = int(st.sum())
    rec = np.array([f, cx, cy, b])
    edges = []
    if ns:
        om = np.eye(3) if info is None else np.asarray(info, np.float64).reshape(3, 3)
        edges.append(EdgeSet(E_PROJECT_XYZ2UVU, mono.v0[st].copy(), mono.v1[st].copy(),
                             np.concatenate([uv[st], ur[st, None]], axis=1), np.broadcast_to(om, (ns, 3, 3)).copy(),
                             np.broadcast_to(rec, (ns, 4)).copy()))
    if ns < m:
        edges.append(EdgeSet(E_PROJECT_XYZ2UV, mono.v0[~st].copy(), mono.v1[~st].copy(), uv[~st].copy(),
                             mono.info[~st].copy(), np.broadcast_to(rec, (m - ns, 4)).copy()))
    return Problem(prob.name + f"_camparams{frac:g}", prob.vertices, edges, 6, 3)


def camparams_twin(prob: Problem) -> Problem:
    """The same graph in the fork's types: every E_PROJECT_XYZ2UV set as E_SE3_PROJECT_XYZ with fx fy cx cy =
    f f cx cy, every E_PROJECT_XYZ2UVU set as E_STEREO_SE3_PROJECT_XYZ with bf = f * b.  The monocular twin computes
    the same numbers; the stereo twin's error differs in its rounding (a float bf, u - bf / z)."""
    edges = []
    for es in prob.edges:
        if es.etype == E_PROJECT_XYZ2UV:
            f, cx, cy = es.params[:, 0], es.params[:, 1], es.params[:, 2]
            edges.append(EdgeSet(E_SE3_PROJECT_XYZ, es.v0.copy(), es.v1.copy(), es.meas.copy(), es.info.copy(),
                                 np.stack([f, f, cx, cy], axis=1)))
        elif es.etype == E_PROJECT_XYZ2UVU:
            f, cx, cy, b = es.params[:, 0], es.params[:, 1], es.params[:, 2], es.params[:, 3]
            edges.append(EdgeSet(E_STEREO_SE3_PROJECT_XYZ, es.v0.copy(), es.v1.copy(), es.meas.copy(), es.info.copy(),
                                 np.stack([f, f, cx, cy, f * b], axis=1)))
        else:
            edges.append(es)
    return Problem(prob.name + "/twin", list(prob.vertices), edges, prob.pose_dim, prob.landmark_dim)


def by_name(name: str, scale: str = "full") -> Problem:
    """BASELINE configs.  ``scale='small'`` gives parity-test sizes."""
    small = scale == "small"
    if name == "C1":
        return sphere(10, 10) if small else sphere(50, 50)
    if name == "C2":
        return se2_grid(800 if small else 100_000)
    if name == "C3":
        return sphere(20, 20, extra_lap2=True) if small else sphere(250, 400, extra_lap2=True)
    if name == "C4":
        return ba(40, 1500) if small else ba(1000, 100_000)
    if name == "C5":
        return ba(80, 4000) if small else ba(4000, 1_000_000)
    if name == "C4R":  # C4 with random covisibility (dense reduced camera system)
        return ba(120, 3000, window=120) if small else ba(1000, 100_000, window=1000)
    if name == "S2":  # BlockSolver_3_2: 2D landmark SLAM (not a BASELINE config)
        return slam2d(300) if small else slam2d(100_000)
    raise KeyError(name)


def landmark_shard(prob: Problem, rank: int, nranks: int) -> Problem:
    """Sub-problem of landmark shard ``rank``: every camera, the contiguous landmark range
    [P*rank/nranks, P*(rank+1)/nranks) of the landmark order and the observations of those
    landmarks — the same partition the device engine uses (engine.cpp setup_edges_device)."""
    cams, pts = prob.vertices
    e = prob.edges[0]
    P = pts.ids.size
    a, b = P * rank // nranks, P * (rank + 1) // nranks
    keep = slice(a, b)
    ids = pts.ids[keep]
    m = (e.v0 >= ids[0]) & (e.v0 <= ids[-1]) if ids.size else np.zeros(e.v0.size, bool)
    pv = VertexSet(pts.vtype, ids.copy(), pts.est[keep].copy(), pts.fixed[keep].copy(), pts.marginalized[keep].copy())
    ev = EdgeSet(e.etype, e.v0[m].copy(), e.v1[m].copy(), e.meas[m].copy(), e.info[m].copy(),
                 None if e.params is None else e.params[m].copy())
    return Problem(f"{prob.name}/shard{rank}of{nranks}", [cams, pv], [ev], prob.pose_dim, prob.landmark_dim)


def landmark_subset(prob: Problem, ids, name: str = "subset") -> Problem:
    """Sub-problem of every camera and the landmarks whose ids are in ``ids`` (any subset, e.g. the aligned shard a rank
    holds, SparseOptimizer.local_landmark_ids), with the observations of those landmarks."""
    cams, pts = prob.vertices
    e = prob.edges[0]
    keep = np.isin(pts.ids, np.asarray(ids))
    m = np.isin(e.v0, pts.ids[keep])
    pv = VertexSet(pts.vtype, pts.ids[keep].copy(), pts.est[keep].copy(), pts.fixed[keep].copy(),
                   pts.marginalized[keep].copy())
    ev = EdgeSet(e.etype, e.v0[m].copy(), e.v1[m].copy(), e.meas[m].copy(), e.info[m].copy(),
                 None if e.params is None else e.params[m].copy())
    return Problem(f"{prob.name}/{name}", [cams, pv], [ev], prob.pose_dim, prob.landmark_dim)


# ---------------------------------------------------------------- unary edges (priors)
def with_priors(prob: Problem, etype: int, every: int = 10, sigma=0.1, seed: int = SEED, drop_fixed: bool = False,
                offset=None, start: int = 0, count: int | None = None) -> Problem:
    """A copy of ``prob`` with priors of one unary type (E_SE2_PRIOR, E_SE2_XY_PRIOR, E_XY_PRIOR, E_SE3_PRIOR,
    E_XYZ_PRIOR) on every ``every``-th vertex of the type it attaches to (from vertex ``start`` of that type's first
    vertex set, at most ``count`` of them).  The measurement is the vertex's estimate (for E_SE3_PRIOR composed with
    ``offset``, x y z qx qy qz qw, None = identity) plus Gaussian noise of ``sigma`` (a scalar or one value per error
    component); the information is sigma^-1 (I + A)(I + A)^T sigma^-1 with A random per edge: SPD, not diagonal.
    ``drop_fixed`` un-fixes every fixed vertex, so the priors alone hold the gauge.  ``prob`` itself is left
    unchanged; the existing edge sets are shared, the vertex sets copied."""
    vt = PRIOR_VERTEX[etype]
    D, nm = ERR_DIM[etype], MEAS_DIM[etype]
    rng = _rng(seed, 16 + etype)
    verts = [VertexSet(v.vtype, v.ids.copy(), v.est.copy(),
                       np.zeros_like(v.fixed) if drop_fixed else v.fixed.copy(), v.marginalized.copy())
             for v in prob.vertices]
    vs = next(v for v in verts if v.vtype == vt)
    sel = np.arange(start, len(vs.ids), every)
    if count is not None:
        sel = sel[:count]
    n = len(sel)
    est = vs.est[sel]
    sg = np.broadcast_to(np.asarray(sigma, np.float64), (D,))
    noise = rng.standard_normal((n, D)) * sg
    params = None
    if etype == E_SE2_PRIOR:
        meas = est + noise
        meas[:, 2] = np.mod(meas[:, 2] + np.pi, 2 * np.pi) - np.pi
    elif etype == E_SE2_XY_PRIOR:
        meas = est[:, :2] + noise
    elif etype in (E_XY_PRIOR, E_XYZ_PRIOR):
        meas = est + noise
    else:  # E_SE3_PRIOR: z = X * P * exp(noise)
        R, t = quat_to_rot(est[:, 3:7]), est[:, 0:3]
        if offset is not None:
            off = np.asarray(offset, np.float64).reshape(7)
            qo = off[3:7] / np.linalg.norm(off[3:7])
            Ro = quat_to_rot(qo[None])[0]
            t = t + R @ off[0:3]
            R = R @ Ro
            params = np.broadcast_to(np.concatenate([off[0:3], qo]), (n, 7)).copy()
        ang = np.linalg.norm(noise[:, 3:6], axis=1)
        dR = _axis_angle(np.where(ang[:, None] > 0, noise[:, 3:6], [1.0, 0.0, 0.0]), 2 * ang)
        meas = np.concatenate([t + np.einsum("nij,nj->ni", R, noise[:, 0:3]), rot_to_quat(R @ dR)], axis=1)
    A = np.eye(D) + 0.3 * rng.standard_normal((n, D, D))
    info = np.einsum("nij,nkj->nik", A, A) / (sg[:, None] * sg[None, :])
    info = 0.5 * (info + np.transpose(info, (0, 2, 1)))
    es = EdgeSet(etype, vs.ids[sel].copy(), None, meas, info, params)
    return Problem(prob.name + f"+prior{etype}x{n}", verts, list(prob.edges) + [es], prob.pose_dim, prob.landmark_dim)


def twin_of(prob: Problem) -> Problem:
    """The binary-only twin of a graph with priors: one fixed identity vertex I per needed type (an unused id each) and
    every E_SE2_PRIOR(v; z) as E_SE2(I, v; z), every E_SE3_PRIOR(v; z) with the identity offset as E_SE3_QUAT(I, v; z),
    every E_XY_PRIOR(l; z) as E_SE2_XY(I, l; z).  With I the identity the reference's binary edges give the prior's
    error and its free-side Jacobian exactly, so H, b, chi2, lambda_0 and the hessian order are those of the prior
    graph.  The other unary types have no twin (KeyError)."""
    twin = {E_SE2_PRIOR: (E_SE2, V_SE2), E_SE3_PRIOR: (E_SE3_QUAT, V_SE3_QUAT), E_XY_PRIOR: (E_SE2_XY, V_SE2)}
    next_id = max(int(v.ids.max()) for v in prob.vertices if len(v.ids)) + 1
    ident: dict = {}
    verts = list(prob.vertices)
    edges = []
    for es in prob.edges:
        if es.v1 is not None:
            edges.append(es)
            continue
        bt, ivt = twin[es.etype]
        if es.etype == E_SE3_PRIOR and es.params is not None and not np.array_equal(
                es.params, np.broadcast_to([0, 0, 0, 0, 0, 0, 1.0], es.params.shape)):
            raise KeyError("an SE3 prior with an offset has no binary twin")
        if ivt not in ident:
            e0 = np.zeros((1, EST_DIM[ivt]))
            if ivt == V_SE3_QUAT:
                e0[0, 6] = 1.0
            ident[ivt] = next_id
            verts.append(VertexSet(ivt, np.array([next_id], np.int32), e0, np.ones(1, np.int32), np.zeros(1, np.int32)))
            next_id += 1
        iv = np.full(len(es.v0), ident[ivt], np.int32)
        edges.append(EdgeSet(bt, iv, es.v0.copy(), es.meas.copy(), es.info.copy(), None))
    return Problem(prob.name + "/twin", verts, edges, prob.pose_dim, prob.landmark_dim)


# ---------------------------------------------------------------- slam3d landmark graphs
def slam3d_landmarks(num_poses: int = 40, num_points: int = 600, kind=E_SE3_XYZ, offset=None, camera=None,
                     obs_per_point: int = 4, pose_noise=(0.02, 0.01), point_noise: float = 0.05,
                     meas_noise=(0.02, 1.0, 0.02, 0.002), seed: int = SEED) -> Problem:
    """3D SLAM with landmarks (the shape of g2o_simulator3d's output): ``num_poses`` VertexSE3 poses on a circle of
    radius 3 (sensor axis z pointing outwards, the first pose fixed) with E_SE3_QUAT odometry between consecutive ones,
    and ``num_points`` VertexPointXYZ points (marginalized), each observed from the ``obs_per_point`` poses nearest
    along the trajectory to the pose it was drawn in front of.  ``kind`` is one of E_SE3_XYZ, E_SE3_XYZ_DEPTH,
    E_SE3_XYZ_DISPARITY or a sequence of them: one edge set per kind over the same (pose, point) pairs.  ``offset``
    (x y z qx qy qz qw, None = identity) is the sensor offset on the pose, ``camera`` (fx fy cx cy, default
    520 510 320 240) the intrinsics of the two camera kinds.  A point is drawn 3 to 6 units in front of its sensor and
    an observation is kept only where the ground-truth sensor-frame z is >= 1 (the scene is ~10 across).
    ``pose_noise`` = (translation, quaternion) sigma of the odometry, ``point_noise`` of the initial point estimates,
    ``meas_noise`` = sigma of (sensor-frame xyz, pixels, depth, inverse depth).  The information is
    sigma^-1 (I + A)(I + A)^T sigma^-1 with A random per edge: SPD, not diagonal."""
    kinds = [int(kind)] if np.isscalar(kind) else [int(k) for k in kind]
    n = num_poses
    rng = _rng(seed, 40)
    th = 2 * math.pi * np.arange(n) / n
    zero, one = np.zeros(n), np.ones(n)
    Rt = np.stack([np.stack([-np.sin(th), zero, np.cos(th)], 1), np.stack([np.cos(th), zero, np.sin(th)], 1),
                   np.stack([zero, one, zero], 1)], 1)  # columns: tangent, up, outward radial
    tt = 3.0 * np.stack([np.cos(th), np.sin(th), 0.1 * np.sin(3 * th)], 1)
    # odometry prev^-1 * cur with noise, and the chained initial estimate (as sphere())
    a, b = np.arange(0, n - 1), np.arange(1, n)
    Rrel = np.transpose(Rt[a], (0, 2, 1)) @ Rt[b]
    trel = np.einsum("nji,nj->ni", Rt[a], tt[b] - tt[a])
    st, sq = pose_noise
    qn = rng.standard_normal((n - 1, 3)) * sq
    ang = np.linalg.norm(qn, axis=1)
    dR = _axis_angle(np.where(ang[:, None] > 0, qn, [1.0, 0.0, 0.0]), 2 * ang)
    Rm = Rrel @ dR
    tm = trel + rng.standard_normal((n - 1, 3)) * st
    odo_meas = np.concatenate([tm, rot_to_quat(Rm)], axis=1)
    Rm = quat_to_rot(odo_meas[:, 3:7])
    odo_info = np.zeros((6, 6))
    odo_info[0:3, 0:3] = np.eye(3) / (st * st)
    odo_info[3:6, 3:6] = np.eye(3) / (sq * sq)
    Rc, tc = np.empty((n, 3, 3)), np.empty((n, 3))
    Rc[0], tc[0] = Rt[0], tt[0]
    for i in range(1, n):
        Rc[i] = Rc[i - 1] @ Rm[i - 1]
        tc[i] = Rc[i - 1] @ tm[i - 1] + tc[i - 1]
    fixed = np.zeros(n, np.int32)
    fixed[0] = 1
    poses = VertexSet(V_SE3_QUAT, np.arange(n, dtype=np.int32), _iso_vec(Rc, tc), fixed, np.zeros(n, np.int32))
    odo = EdgeSet(E_SE3_QUAT, a.astype(np.int32), b.astype(np.int32), odo_meas, np.broadcast_to(odo_info, (n - 1, 6, 6)).copy())
    # the sensor frames S_i = X_i * P
    off = np.array([0, 0, 0, 0, 0, 0, 1.0]) if offset is None else np.asarray(offset, np.float64).reshape(7).copy()
    off[3:7] /= np.linalg.norm(off[3:7])
    Rp = quat_to_rot(off[None, 3:7])[0]
    Rs, ts = Rt @ Rp, tt + Rt @ off[0:3]
    # points: drawn in the sensor frame of an anchor pose, seen from the poses nearest to it along the trajectory
    m = num_points
    anchor = rng.integers(0, n, m)
    local = np.stack([rng.uniform(-1.5, 1.5, m), rng.uniform(-1.5, 1.5, m), rng.uniform(3.0, 6.0, m)], 1)
    pts = ts[anchor] + np.einsum("nij,nj->ni", Rs[anchor], local)
    steps = np.array([(k + 1) // 2 * (1 if k % 2 else -1) for k in range(obs_per_point)])  # 0, 1, -1, 2, -2, ...
    op = ((anchor[:, None] + steps[None, :]) % n).ravel()
    ol = np.repeat(np.arange(m), obs_per_point)
    pn = np.einsum("nji,nj->ni", Rs[op], pts[ol] - ts[op])
    keep = pn[:, 2] >= 1.0
    op, ol, pn = op[keep], ol[keep], pn[keep]
    ne = len(op)
    pid = (n + np.arange(m)).astype(np.int32)
    points = VertexSet(V_XYZ, pid, pts + rng.standard_normal((m, 3)) * point_noise, np.zeros(m, np.int32),
                       np.ones(m, np.int32))
    cam = np.array([520.0, 510.0, 320.0, 240.0]) if camera is None else np.asarray(camera, np.float64).reshape(4)
    s_xyz, s_px, s_d, s_id = meas_noise
    edges = [odo]
    for kd in kinds:
        r = _rng(seed, 41 + kd)
        if kd == E_SE3_XYZ:
            sg = np.full(3, s_xyz)
            z = pn.copy()
            params = None if offset is None else np.broadcast_to(off, (ne, 7)).copy()
        else:
            u = cam[0] * pn[:, 0] / pn[:, 2] + cam[2]
            v = cam[1] * pn[:, 1] / pn[:, 2] + cam[3]
            if kd == E_SE3_XYZ_DEPTH:
                sg, z = np.array([s_px, s_px, s_d]), np.stack([u, v, pn[:, 2]], 1)
            elif kd == E_SE3_XYZ_DISPARITY:
                sg, z = np.array([s_px, s_px, s_id]), np.stack([u, v, 1.0 / pn[:, 2]], 1)
            else:
                raise KeyError(kd)
            params = np.broadcast_to(np.concatenate([off, cam]), (ne, 11)).copy()
        z = z + r.standard_normal((ne, 3)) * sg
        A = np.eye(3) + 0.3 * r.standard_normal((ne, 3, 3))
        info = np.einsum("nij,nkj->nik", A, A) / (sg[:, None] * sg[None, :])
        info = 0.5 * (info + np.transpose(info, (0, 2, 1)))
        edges.append(EdgeSet(kd, poses.ids[op].copy(), pid[ol].copy(), z, info, params))
    name = f"slam3d{n}x{m}k" + "".join(str(k) for k in kinds)
    return Problem(name, [poses, points], edges, 6, 3)


# ---------------------------------------------------------------- EdgeSE3Expmap pose graphs
def _se3_exp(u):
    """SE3Quat::exp of [n, 6] (omega, upsilon) -> (R [n, 3, 3], t [n, 3])."""
    u = np.asarray(u, np.float64).reshape(-1, 6)
    om, ups = u[:, :3], u[:, 3:]
    th = np.linalg.norm(om, axis=1)
    small = th < 1e-5
    t1 = np.where(small, 1.0, th)
    Om = np.zeros((len(u), 3, 3))
    Om[:, 0, 1], Om[:, 0, 2] = -om[:, 2], om[:, 1]
    Om[:, 1, 0], Om[:, 1, 2] = om[:, 2], -om[:, 0]
    Om[:, 2, 0], Om[:, 2, 1] = -om[:, 1], om[:, 0]
    Om2 = Om @ Om
    a = np.where(small, 1.0, np.sin(t1) / t1)[:, None, None]
    b = np.where(small, 0.5, (1 - np.cos(t1)) / (t1 * t1))[:, None, None]
    d = np.where(small, 1.0 / 6.0, (t1 - np.sin(t1)) / (t1 * t1 * t1))[:, None, None]
    eye = np.eye(3)[None]
    return eye + a * Om + b * Om2, np.einsum("nij,nj->ni", eye + b * Om + d * Om2, ups)


def _spd_info(rng, n, sg):
    """sigma^-1 (I + A)(I + A)^T sigma^-1 with A random per edge: SPD, not diagonal."""
    D = len(sg)
    A = np.eye(D) + 0.3 * rng.standard_normal((n, D, D))
    info = np.einsum("nij,nkj->nik", A, A) / (sg[:, None] * sg[None, :])
    return 0.5 * (info + np.transpose(info, (0, 2, 1)))


def expmap_pose_graph(num_poses: int = 200, loops: int = 40, rot_noise: float = 0.01, trans_noise: float = 0.02,
                      init: str = "odometry", seed: int = SEED) -> Problem:
    """A pose graph on the BA camera parameterisation: ``num_poses`` VertexSE3Expmap cameras (world->camera, as in
    :func:`ba`) on a rising circle of radius 5, looking along the direction of travel, joined by EdgeSE3Expmap
    odometry (i, i + 1) and ``loops`` loop closures (i, j), j > i + 1, drawn at random.  With the edge's error
    log(Tj^-1 C Ti) the measurement is C = Tj exp(noise) Ti^-1 of the true poses: at the true poses the error of an
    edge is its noise, (omega, upsilon) with sigmas (``rot_noise``, ``trans_noise``).  The information is
    sigma^-1 (I + A)(I + A)^T sigma^-1 with A random per edge: SPD, not diagonal.  Pose 0 is fixed.  Initial
    estimates: ``init`` = "odometry" chains the measured odometry from pose 0, "truth" takes the true poses."""
    n = num_poses
    rng = _rng(seed, 60)
    th = 2 * math.pi * np.arange(n) / max(n, 8) * 1.0
    pos = np.stack([5 * np.cos(th), 5 * np.sin(th), 0.02 * np.arange(n)], 1)
    zero, one = np.zeros(n), np.ones(n)
    # camera-to-world attitude: x right (outward radial), y down (-z), z forward (tangent); a small random tilt on top
    Rc = np.stack([np.stack([np.cos(th), zero, -np.sin(th)], 1), np.stack([np.sin(th), zero, np.cos(th)], 1),
                   np.stack([zero, -one, zero], 1)], 1) @ _small_rot(rng, n, 0.05)
    Rw = np.transpose(Rc, (0, 2, 1))
    tw = -np.einsum("nij,nj->ni", Rw, pos)
    a = np.arange(0, n - 1)
    b = np.arange(1, n)
    if loops > 0 and n > 2:
        la = rng.integers(0, n - 2, loops)
        lb = la + 2 + (rng.random(loops) * (n - 2 - la)).astype(np.int64)
        a, b = np.concatenate([a, la]), np.concatenate([b, np.minimum(lb, n - 1)])
    m = len(a)
    sg = np.array([rot_noise] * 3 + [trans_noise] * 3)
    Rn, tn = _se3_exp(rng.standard_normal((m, 6)) * sg)
    # C = Tj * N * Ti^-1, (R1, t1) * (R2, t2) = (R1 R2, t1 + R1 t2)
    Rjn, tjn = Rw[b] @ Rn, tw[b] + np.einsum("nij,nj->ni", Rw[b], tn)
    Rm = Rjn @ np.transpose(Rw[a], (0, 2, 1))
    tm = tjn - np.einsum("nij,nj->ni", Rm, tw[a])
    meas = np.concatenate([tm, rot_to_quat(Rm)], axis=1)
    info = _spd_info(rng, m, sg)
    if init == "truth":
        R0, t0 = Rw, tw
    else:  # Tj = C * Ti along the odometry edges (zero error on them)
        Rq = quat_to_rot(meas[: n - 1, 3:7])
        R0, t0 = np.empty((n, 3, 3)), np.empty((n, 3))
        R0[0], t0[0] = Rw[0], tw[0]
        for i in range(1, n):
            R0[i] = Rq[i - 1] @ R0[i - 1]
            t0[i] = Rq[i - 1] @ t0[i - 1] + tm[i - 1]
    fixed = np.zeros(n, np.int32)
    fixed[0] = 1
    ids = np.arange(n, dtype=np.int32)
    verts = VertexSet(V_SE3_EXPMAP, ids, np.concatenate([t0, rot_to_quat(R0)], axis=1), fixed, np.zeros(n, np.int32))
    edges = EdgeSet(E_SE3_EXPMAP, ids[a].copy(), ids[b].copy(), meas, info)
    return Problem(f"expmap{n}l{loops}", [verts], [edges], 6, 0)


# ---------------------------------------------------------------- pose-only projections
def _pose_only_set(cam_ids, xw, uv, K, ur, bf, rng, pixel_sigma):
    """One pose-only edge set: monocular (``ur`` None) or stereo. K: [n, 4] fx fy cx cy."""
    n = len(cam_ids)
    if ur is None:
        return EdgeSet(E_SE3_PROJECT_XYZ_ONLYPOSE, cam_ids, None, uv, _spd_info(rng, n, np.full(2, pixel_sigma)),
                       np.concatenate([xw, K], axis=1))
    return EdgeSet(E_STEREO_SE3_PROJECT_XYZ_ONLYPOSE, cam_ids, None, np.concatenate([uv, ur[:, None]], axis=1),
                   _spd_info(rng, n, np.full(3, pixel_sigma)), np.concatenate([xw, K, np.full((n, 1), float(bf))], axis=1))


def pose_only(num_cameras: int = 8, points_per_camera: int = 120, stereo: bool = False, pixel_noise: float = 1.0,
              cam_rot_noise: float = 0.002, cam_trans_noise: float = 0.01, point_noise: float = 0.01,
              bf: float = 100.3, seed: int = SEED) -> Problem:
    """Pose optimisation: ``num_cameras`` free VertexSE3Expmap cameras, each observing its own points through
    EdgeSE3ProjectXYZOnlyPose (``stereo``: EdgeStereoSE3ProjectXYZOnlyPose) edges.  Cameras, points and left-image
    measurements are those of :func:`ba`'s scene maker with num_cameras * points_per_camera points, each seen by one
    camera (the scene deals the points to the cameras at random, so a camera holds points_per_camera of them on
    average); no camera is fixed.  Xw of an edge is the scene's point estimate (the true point plus ``point_noise``),
    which nothing optimises.  Stereo: u_r = u_true - bf / z_true + noise, as :func:`ba_stereo`.  The information is
    sigma^-1 (I + A)(I + A)^T sigma^-1 with A random per edge.  No landmarks: pose_dim 6, landmark_dim 0."""
    prob, pc, uv_true = _ba_scene(num_cameras, num_cameras * points_per_camera, 1, 1, pixel_noise, cam_rot_noise,
                                  cam_trans_noise, point_noise, 0, seed)
    cams, pts = prob.vertices
    e = prob.edges[0]
    xw = pts.est[e.v0 - pts.ids[0]]
    rng = _rng(seed, 61)
    ur = None
    if stereo:
        ur = uv_true[:, 0] - bf / pc[:, 2] + _rng(seed, 62).standard_normal(len(e.v0)) * pixel_noise
    es = _pose_only_set(e.v1.copy(), xw, e.meas.copy(), e.params.copy(), ur, bf, rng, pixel_noise)
    return Problem(f"poseonly{num_cameras}x{points_per_camera}" + ("s" if stereo else ""), [cams], [es], 6, 0)


def with_pose_only(prob: Problem, every: int = 3, per_camera: int = 20, stereo: bool = False, point_noise: float = 0.01,
                   bf: float = 100.3, seed: int = SEED) -> Problem:
    """A copy of a BA problem (:func:`ba`) with pose-only edges on every ``every``-th camera (fixed ones included:
    their edges are inactive): the camera's first ``per_camera`` observations again, each as a pose-only edge whose Xw
    is the point's estimate plus ``point_noise``.  Stereo: u_r = u - bf / z at the camera's and the point's estimates.
    ``prob`` is left unchanged; vertex and edge sets are shared."""
    cams, pts = prob.vertices[0], prob.vertices[1]
    e = next(x for x in prob.edges if x.etype == E_SE3_PROJECT_XYZ)
    rng = _rng(seed, 63)
    sel = []
    for c in cams.ids[::every]:
        sel.append(np.nonzero(e.v1 == c)[0][:per_camera])
    sel = np.concatenate(sel)
    pt = pts.est[e.v0[sel] - pts.ids[0]]
    xw = pt + rng.standard_normal(pt.shape) * point_noise
    ur = None
    if stereo:
        ce = cams.est[e.v1[sel] - cams.ids[0]]
        z = np.einsum("nij,nj->ni", quat_to_rot(ce[:, 3:7]), pt)[:, 2] + ce[:, 2]
        ur = e.meas[sel, 0] - bf / z
    es = _pose_only_set(e.v1[sel].copy(), xw, e.meas[sel].copy(), e.params[sel].copy(), ur, bf, rng, 1.0)
    return Problem(prob.name + f"+poseonly{len(sel)}", prob.vertices, list(prob.edges) + [es], prob.pose_dim,
                   prob.landmark_dim)


def pose_only_twin(prob: Problem) -> Problem:
    """The same graph with every pose-only edge replaced by the binary projection edge (E_SE3_PROJECT_XYZ,
    E_STEREO_SE3_PROJECT_XYZ) to a **fixed** V_XYZ vertex at Xw, one new vertex (an unused id) per edge.  A fixed
    vertex takes no part in the system, so H, b and the hessian order are the pose-only graph's.  For the monocular
    type the twin's error is the pose-only edge's exactly; for the stereo type only to the float rounding of 1/z
    (the pose-only edge rounds 1/z to float, the binary one bf)."""
    next_id = max(int(v.ids.max()) for v in prob.vertices if len(v.ids)) + 1
    verts, edges = list(prob.vertices), []
    for es in prob.edges:
        if es.etype not in POSE_ONLY_BINARY:
            edges.append(es)
            continue
        n = len(es.v0)
        ids = (next_id + np.arange(n)).astype(np.int32)
        next_id += n
        verts.append(VertexSet(V_XYZ, ids, es.params[:, :3].copy(), np.ones(n, np.int32), np.ones(n, np.int32)))
        edges.append(EdgeSet(POSE_ONLY_BINARY[es.etype], ids, es.v0.copy(), es.meas.copy(), es.info.copy(),
                             es.params[:, 3:].copy()))
    return Problem(prob.name + "/twin", verts, edges, prob.pose_dim, prob.landmark_dim)


# ---------------------------------------------------------------- offset pose graphs, bearing-only landmarks
def _loop_pairs(rng, n, loops):
    """Odometry (i, i + 1) and ``loops`` closures (i, j), j > i + 1, drawn at random."""
    a, b = np.arange(0, n - 1), np.arange(1, n)
    if loops > 0 and n > 2:
        la = rng.integers(0, n - 2, loops)
        lb = la + 2 + (rng.random(loops) * (n - 2 - la)).astype(np.int64)
        a, b = np.concatenate([a, la]), np.concatenate([b, np.minimum(lb, n - 1)])
    return a, b


def se3_offset_graph(num_poses: int = 40, loops: int = 80, num_offsets: int = 2, rot_noise: float = 0.01,
                     trans_noise: float = 0.02, seed: int = SEED) -> Problem:
    """An SE3 pose graph measured between sensor frames (EdgeSE3Offset, what g2o_simulator3d's pose sensor writes):
    ``num_poses`` VertexSE3 bodies on a rising circle joined by odometry and ``loops`` loop closures.  The body carries
    ``num_offsets`` (1 or 2) sensors with distinct mounting offsets; an edge measures Z = (Xi Pi)^-1 (Xj Pj) * noise
    between the sensor of its from vertex and that of its to vertex, the sensor pair alternating from edge to edge
    when there are two.  params [m, 14]: the from vertex's offset, then the to vertex's.  Information: SPD, not
    diagonal.  Pose 0 is fixed; initial estimates are the true poses perturbed."""
    n = num_poses
    rng = _rng(seed, 70)
    th = 2 * math.pi * np.arange(n) / max(n, 8)
    pos = np.stack([5 * np.cos(th), 5 * np.sin(th), 0.05 * np.arange(n)], 1)
    R = _axis_angle(np.tile([0.0, 0.0, 1.0], (n, 1)), th + 0.5 * math.pi) @ _small_rot(rng, n, 0.2)
    offR = _axis_angle(np.array([[0.3, -0.5, 0.8], [-0.7, 0.2, 0.4]]), np.array([0.6, -1.1]))
    offt = np.array([[0.2, -0.1, 0.3], [-0.15, 0.25, 0.1]])
    a, b = _loop_pairs(rng, n, loops)
    m = len(a)
    k = np.arange(m)
    si = (k % 2) if num_offsets > 1 else np.zeros(m, np.int64)
    sj = ((k // 2) % 2) if num_offsets > 1 else np.zeros(m, np.int64)
    # n2w = X P
    Rni, tni = R[a] @ offR[si], pos[a] + np.einsum("nij,nj->ni", R[a], offt[si])
    Rnj, tnj = R[b] @ offR[sj], pos[b] + np.einsum("nij,nj->ni", R[b], offt[sj])
    Rz = np.transpose(Rni, (0, 2, 1)) @ Rnj
    tz = np.einsum("nji,nj->ni", Rni, tnj - tni)
    sg = np.array([trans_noise] * 3 + [rot_noise] * 3)
    Rz = Rz @ _small_rot(rng, m, rot_noise)
    tz = tz + rng.standard_normal((m, 3)) * trans_noise
    meas = np.concatenate([tz, rot_to_quat(Rz)], axis=1)
    info = _spd_info(rng, m, sg)
    offv = np.concatenate([offt, rot_to_quat(offR)], axis=1)
    params = np.concatenate([offv[si], offv[sj]], axis=1)
    R0 = R @ _small_rot(rng, n, 0.03)
    t0 = pos + rng.standard_normal((n, 3)) * 0.05
    R0[0], t0[0] = R[0], pos[0]
    fixed = np.zeros(n, np.int32)
    fixed[0] = 1
    ids = np.arange(n, dtype=np.int32)
    verts = VertexSet(V_SE3_QUAT, ids, _iso_vec(R0, t0), fixed, np.zeros(n, np.int32))
    edges = EdgeSet(E_SE3_OFFSET, ids[a].copy(), ids[b].copy(), meas, info, params)
    return Problem(f"se3offset{n}l{loops}o{num_offsets}", [verts], [edges], 6, 0)


def se2_offset_graph(num_poses: int = 40, loops: int = 80, num_offsets: int = 2, noise=(0.03, 0.03, 0.01),
                     seed: int = SEED) -> Problem:
    """The 2D sibling of :func:`se3_offset_graph` (EdgeSE2Offset): VertexSE2 bodies on a circle, one or two sensors
    with distinct offsets (x y theta), Z = (Xi Pi)^-1 (Xj Pj) + noise.  params [m, 6]."""
    n = num_poses
    rng = _rng(seed, 71)
    th = 2 * math.pi * np.arange(n) / max(n, 8)
    gt = np.stack([5 * np.cos(th), 5 * np.sin(th), np.mod(th + 0.5 * math.pi + np.pi, 2 * np.pi) - np.pi], 1)
    gt[:, 2] += rng.standard_normal(n) * 0.2
    gt[:, 2] = np.mod(gt[:, 2] + np.pi, 2 * np.pi) - np.pi
    off = np.array([[0.3, -0.2, 0.7], [-0.25, 0.4, -1.2]])
    a, b = _loop_pairs(rng, n, loops)
    m = len(a)
    k = np.arange(m)
    si = (k % 2) if num_offsets > 1 else np.zeros(m, np.int64)
    sj = ((k // 2) % 2) if num_offsets > 1 else np.zeros(m, np.int64)
    ni, nj = _se2_compose(gt[a], off[si]), _se2_compose(gt[b], off[sj])
    meas = _se2_between(ni, nj) + rng.standard_normal((m, 3)) * np.asarray(noise)
    meas[:, 2] = np.mod(meas[:, 2] + np.pi, 2 * np.pi) - np.pi
    info = _spd_info(rng, m, np.asarray(noise, float))
    params = np.concatenate([off[si], off[sj]], axis=1)
    est = gt + rng.standard_normal((n, 3)) * np.array([0.05, 0.05, 0.03])
    est[0] = gt[0]
    est[:, 2] = np.mod(est[:, 2] + np.pi, 2 * np.pi) - np.pi
    fixed = np.zeros(n, np.int32)
    fixed[0] = 1
    ids = np.arange(n, dtype=np.int32)
    verts = VertexSet(V_SE2, ids, est, fixed, np.zeros(n, np.int32))
    edges = EdgeSet(E_SE2_OFFSET, ids[a].copy(), ids[b].copy(), meas, info, params)
    return Problem(f"se2offset{n}l{loops}o{num_offsets}", [verts], [edges], 3, 0)


def bearing_scene(num_poses: int = 12, num_landmarks: int = 30, obs_per_landmark: int = 4, bearing_noise: float = 0.01,
                  odo_noise=(0.03, 0.03, 0.01), seed: int = SEED) -> Problem:
    """Bearing-only 2D landmark SLAM (EdgeSE2PointXYBearing, what g2o_simulator2d's bearing sensor writes):
    ``num_poses`` VertexSE2 poses on a circle of radius 6 around ``num_landmarks`` VertexPointXY landmarks scattered
    within radius 2 of its centre, so that every pose sees every landmark at a distance of at least 4 and two poses
    see one landmark under different directions (parallax).  Each landmark is seen from ``obs_per_landmark`` (>= 3)
    distinct poses spread over the circle; consecutive poses are joined by EdgeSE2 odometry, which with the fixed pose
    0 sets the gauge and the scale.  The landmarks are marginalised (BlockSolver_3_2).  Initial estimates: the true
    values perturbed."""
    n, L, k = num_poses, num_landmarks, min(obs_per_landmark, num_poses)
    rng = _rng(seed, 72)
    th = 2 * math.pi * np.arange(n) / n
    gt = np.stack([6 * np.cos(th), 6 * np.sin(th), np.mod(th + np.pi + np.pi, 2 * np.pi) - np.pi], 1)  # facing the centre
    gt[:, 2] = np.mod(gt[:, 2] + rng.standard_normal(n) * 0.3 + np.pi, 2 * np.pi) - np.pi
    rad, ang = 2.0 * np.sqrt(rng.random(L)), 2 * math.pi * rng.random(L)
    lm = np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
    # landmark l: poses start + round(j n / k), j < k, spread over the circle
    start = rng.integers(0, n, L)
    op = (start[:, None] + np.round(np.arange(k) * n / k).astype(np.int64)[None, :]) % n
    oa, ob = op.reshape(-1), np.repeat(np.arange(L), k)
    order = np.lexsort((ob, oa))
    oa, ob = oa[order], ob[order]
    c, s = np.cos(gt[oa, 2]), np.sin(gt[oa, 2])
    dx, dy = lm[ob, 0] - gt[oa, 0], lm[ob, 1] - gt[oa, 1]
    z = np.arctan2(-s * dx + c * dy, c * dx + s * dy) + rng.standard_normal(len(oa)) * bearing_noise
    z = np.mod(z + np.pi, 2 * np.pi) - np.pi
    a = np.arange(n - 1)
    zodo = _se2_between(gt[a], gt[a + 1]) + rng.standard_normal((n - 1, 3)) * np.asarray(odo_noise)
    zodo[:, 2] = np.mod(zodo[:, 2] + np.pi, 2 * np.pi) - np.pi
    est = gt + rng.standard_normal((n, 3)) * np.array([0.05, 0.05, 0.02])
    est[0] = gt[0]
    est[:, 2] = np.mod(est[:, 2] + np.pi, 2 * np.pi) - np.pi
    lest = lm + rng.standard_normal((L, 2)) * 0.1
    fixed = np.zeros(n, np.int32)
    fixed[0] = 1
    pose_ids = np.arange(n, dtype=np.int32)
    lm_ids = (n + np.arange(L)).astype(np.int32)
    poses = VertexSet(V_SE2, pose_ids, est, fixed, np.zeros(n, np.int32))
    points = VertexSet(V_XY, lm_ids, lest, np.zeros(L, np.int32), np.ones(L, np.int32))
    odo = EdgeSet(E_SE2, pose_ids[a], pose_ids[a + 1], zodo,
                  np.broadcast_to(np.diag(1.0 / np.square(odo_noise)), (n - 1, 3, 3)).copy())
    w = (1.0 / bearing_noise ** 2) * (1.0 + 0.5 * rng.random(len(oa)))  # per-edge scalar information
    obs = EdgeSet(E_SE2_XY_BEARING, pose_ids[oa], lm_ids[ob], z[:, None].copy(), w[:, None, None].copy())
    return Problem(f"bearing{n}x{L}", [poses, points], [odo, obs], 3, 2)


def offset_twin(prob: Problem) -> Problem:
    """The host-Jacobian twin of a graph with offset / bearing edges: every E_SE3_OFFSET, E_SE2_OFFSET and
    E_SE2_XY_BEARING set as an E_HOSTJ(6) / (3) / (1) set (32 + D) between the same vertices with the same
    information; the caller supplies the payload."""
    edges = []
    for es in prob.edges:
        if es.etype in (E_SE3_OFFSET, E_SE2_OFFSET, E_SE2_XY_BEARING):
            edges.append(EdgeSet(32 + ERR_DIM[es.etype], es.v0.copy(), es.v1.copy(), None, es.info.copy(), None))
        else:
            edges.append(es)
    return Problem(prob.name + "/hostj", list(prob.vertices), edges, prob.pose_dim, prob.landmark_dim)


# ---------------------------------------------------------------- types_icp scenes
def _gicp_rot0(normal):
    """EdgeGICP::makeRot0 (types_icp.h:84-96): rows n x y, y, n with y = (0,1,0) - n_y n normalised."""
    n = np.asarray(normal, np.float64).reshape(3)
    y = np.array([0.0, 1.0, 0.0]) - n[1] * n
    yn = float(np.linalg.norm(y))
    if not (yn > 0.0 and np.isfinite(yn)):
        raise ValueError("gicp: a normal parallel to (0,1,0) makes the reference's makeRot0 divide by zero")
    y = y / yn
    return np.stack([np.cross(n, y), y, n])


def gicp_prec(normal, e: float = 0.01):
    """EdgeGICP::prec0 / prec1 (types_icp.h:111-130): R0^T diag(e, e, 1) R0, the point-to-plane information."""
    R0 = _gicp_rot0(normal)
    return R0.T @ np.diag([e, e, 1.0]) @ R0


def gicp_cov(normal, e: float = 0.01):
    """EdgeGICP::cov0 / cov1 (types_icp.h:133-152): R0^T diag(1, 1, e) R0, the plane-to-plane covariance."""
    R0 = _gicp_rot0(normal)
    return R0.T @ np.diag([1.0, 1.0, e]) @ R0


def gicp_pack(M):
    """[n, 3, 3] symmetric -> [n, 6] packed upper triangles 00 01 11 02 12 22 (the order of Edge_V_V_GICP's params)."""
    M = np.asarray(M, np.float64).reshape(-1, 3, 3)
    return np.stack([M[:, 0, 0], M[:, 0, 1], M[:, 1, 1], M[:, 0, 2], M[:, 1, 2], M[:, 2, 2]], 1)


def _gicp_normals(k: np.ndarray) -> np.ndarray:
    """gicp_demo's normals (0, i, 1) normalised, i taken modulo 50 (the demo's i runs to 999, where the normal is
    within 1e-3 of the direction makeRot0 cannot take)."""
    n = np.stack([np.zeros(len(k)), (k % 50).astype(np.float64), np.ones(len(k))], 1)
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def _gicp_edges(rng, R, t, a, b, pts, pl_pl, euc_noise, k0=0):
    """Edge_V_V_GICP correspondences of world points ``pts`` [m, 3] between scans a[m] and b[m] with true poses
    (R, t): pos = T^-1 p + noise, gicp_demo's normals; point-to-plane information prec0(0.01) or, with ``pl_pl``,
    the covariances cov0(0.01) | cov1(0.01) and no information."""
    m = len(a)
    p0 = np.einsum("nji,nj->ni", R[a], pts - t[a]) + rng.standard_normal((m, 3)) * euc_noise
    p1 = np.einsum("nji,nj->ni", R[b], pts - t[b]) + rng.standard_normal((m, 3)) * euc_noise
    kk = (k0 + np.arange(m)) % 50  # the fifty distinct normals: one prec0 / cov0 each
    base = _gicp_normals(np.arange(50))
    nm = base[kk]
    meas = np.concatenate([p0, nm, p1, nm], 1)
    if pl_pl:
        cov = gicp_pack(np.stack([gicp_cov(x, 0.01) for x in base]))[kk]
        return meas, None, np.concatenate([cov, cov], 1)
    return meas, np.stack([gicp_prec(x, 0.01) for x in base])[kk], None


def gicp_pair(n_points: int = 1000, pl_pl: bool = False, euc_noise: float = 0.01, seed: int = SEED) -> Problem:
    """gicp_demo.cpp's scene: two VertexSE3 at (0, 0, 0) and (0, 0, 1), the first fixed, ``n_points`` world points in
    the box of the demo seen from both with Gaussian noise, one Edge_V_V_GICP per point; the second pose starts at
    (0, 0, 0.2).  ``pl_pl``: the edge set is plane-to-plane (params cov0 | cov1, info None)."""
    rng = _rng(seed, 80)
    pts = np.stack([(rng.random(n_points) - 0.5) * 3, rng.random(n_points) - 0.5, rng.random(n_points) + 10], 1)
    R = np.broadcast_to(np.eye(3), (2, 3, 3)).copy()
    t = np.array([[0.0, 0, 0], [0, 0, 1.0]])
    a, b = np.zeros(n_points, np.int64), np.ones(n_points, np.int64)
    meas, info, params = _gicp_edges(rng, R, t, a, b, pts, pl_pl, euc_noise)
    t0 = t.copy()
    t0[1, 2] = 0.2
    ids = np.arange(2, dtype=np.int32)
    verts = VertexSet(V_SE3_QUAT, ids, _iso_vec(R, t0), np.array([1, 0], np.int32), np.zeros(2, np.int32))
    edges = EdgeSet(E_V_V_GICP, ids[a].copy(), ids[b].copy(), meas, info, params)
    return Problem(f"gicp_pair{n_points}{'pl' if pl_pl else ''}", [verts], [edges], 6, 0)


def gicp_scans(num_scans: int = 8, neighbours: int = 2, points_per_pair=256, pl_pl: bool = False, fixed=(0,),
               euc_noise: float = 0.01, seed: int = SEED) -> Problem:
    """Scan registration on a ring: ``num_scans`` VertexSE3 on a circle of radius 3 looking at its centre, each matched
    to its next ``neighbours`` scans by Edge_V_V_GICP correspondences of points scattered around the centre.
    ``points_per_pair``: one number, or a sequence cycled over the pairs (deliberately uneven multiplicities, e.g.
    (1, 64, 200)).  Every third pair is entered the other way round for the second half of its edges, so that one
    vertex pair holds edges (i, j) and (j, i).  ``fixed``: the fixed scans.  The initial estimates are the true poses
    perturbed.  Edges are in pair order; within a pair in point order."""
    n = num_scans
    rng = _rng(seed, 81)
    th = 2 * math.pi * np.arange(n) / n
    t = np.stack([3 * np.cos(th), 3 * np.sin(th), 0.1 * np.arange(n)], 1)
    R = _axis_angle(np.tile([0.0, 0.0, 1.0], (n, 1)), th + math.pi) @ _small_rot(rng, n, 0.2)
    mult = [int(points_per_pair)] if np.isscalar(points_per_pair) else [int(x) for x in points_per_pair]
    pairs = [(i, (i + d) % n) for i in range(n) for d in range(1, neighbours + 1) if (i + d) % n != i]
    a, b, pts = [], [], []
    for q, (i, j) in enumerate(pairs):
        m = mult[q % len(mult)]
        ai, bi = np.full(m, i), np.full(m, j)
        if q % 3 == 2:  # the second half of the pair's edges the other way round
            ai[m // 2:], bi[m // 2:] = j, i
        a.append(ai)
        b.append(bi)
        pts.append(rng.standard_normal((m, 3)) * np.array([1.0, 1.0, 0.5]))
    a, b, pts = np.concatenate(a), np.concatenate(b), np.concatenate(pts)
    meas, info, params = _gicp_edges(rng, R, t, a, b, pts, pl_pl, euc_noise)
    R0 = R @ _small_rot(rng, n, 0.02)
    t0 = t + rng.standard_normal((n, 3)) * 0.03
    fx = np.zeros(n, np.int32)
    for i in fixed:
        fx[i] = 1
        R0[i], t0[i] = R[i], t[i]
    ids = np.arange(n, dtype=np.int32)
    verts = VertexSet(V_SE3_QUAT, ids, _iso_vec(R0, t0), fx, np.zeros(n, np.int32))
    edges = EdgeSet(E_V_V_GICP, ids[a].copy(), ids[b].copy(), meas, info, params)
    return Problem(f"gicp_scans{n}x{neighbours}{'pl' if pl_pl else ''}", [verts], [edges], 6, 0)


def gicp_sba(n_matches: int = 200, n_points: int = 100, num_cams: int = 2, pix_noise: float = 1.0,
             euc_noise: float = 0.01, kcam=(150.0, 150.0, 320.0, 240.0, 0.075), seed: int = SEED) -> Problem:
    """gicp_sba_demo.cpp's scene: ``num_cams`` VertexSCam (V_SE3_QUAT, camera-to-world) at (0, 0, i), the first fixed,
    ``n_matches`` Edge_V_V_GICP correspondences between consecutive cameras (point-to-plane, prec0(0.01)) and
    ``n_points`` marginalised points in front of the cameras, each seen by every camera through an Edge_XYZ_VSC
    (u v u_r with pixel noise, the disparity's a sixteenth; identity information; one shared record fx fy cx cy
    baseline).  The points start a little off their true positions, the free cameras off theirs."""
    rng = _rng(seed, 82)
    C = num_cams
    R = np.broadcast_to(np.eye(3), (C, 3, 3)).copy()
    t = np.stack([np.zeros(C), np.zeros(C), np.arange(C, dtype=np.float64)], 1)
    box = lambda m: np.stack([(rng.random(m) - 0.5) * 3, rng.random(m) - 0.5, rng.random(m) + 10], 1)  # noqa: E731
    a = np.arange(n_matches) % (C - 1)
    meas, info, _ = _gicp_edges(rng, R, t, a, a + 1, box(n_matches), False, euc_noise)
    pts = box(n_points)
    fx, fy, cx, cy, bl = kcam
    pa, ca = np.repeat(np.arange(n_points), C), np.tile(np.arange(C), n_points)
    pc = pts[pa] - t[ca]  # identity rotations
    z = np.stack([fx * pc[:, 0] / pc[:, 2] + cx, fy * pc[:, 1] / pc[:, 2] + cy,
                  fx * (pc[:, 0] - bl) / pc[:, 2] + cx], 1)
    z += rng.standard_normal(z.shape) * np.array([pix_noise, pix_noise, pix_noise / 16.0])
    t0 = t + rng.standard_normal((C, 3)) * 0.05
    R0 = R @ _small_rot(rng, C, 0.01)
    R0[0], t0[0] = R[0], t[0]
    cam_ids = np.arange(C, dtype=np.int32)
    pt_ids = (C + np.arange(n_points)).astype(np.int32)
    fixed = np.zeros(C, np.int32)
    fixed[0] = 1
    cams = VertexSet(V_SE3_QUAT, cam_ids, _iso_vec(R0, t0), fixed, np.zeros(C, np.int32))
    points = VertexSet(V_XYZ, pt_ids, pts + rng.standard_normal((n_points, 3)) * 0.1, np.zeros(n_points, np.int32),
                       np.ones(n_points, np.int32))
    gicp = EdgeSet(E_V_V_GICP, cam_ids[a].copy(), cam_ids[a + 1].copy(), meas, info, None)
    vsc = EdgeSet(E_XYZ_VSC, pt_ids[pa].copy(), cam_ids[ca].copy(), z,
                  np.broadcast_to(np.eye(3), (len(pa), 3, 3)).copy(), np.broadcast_to(np.asarray(kcam), (len(pa), 5)).copy())
    return Problem(f"gicp_sba{n_matches}x{n_points}", [cams, points], [gicp, vsc], 6, 3)


def icp_twin(prob: Problem) -> Problem:
    """The host-Jacobian twin of a graph with types_icp edges: every E_V_V_GICP and E_XYZ_VSC set as an E_HOSTJ(3) set
    (35) between the same vertices; the caller supplies the payload.  A point-to-plane set and a VSC set keep their
    information.  A plane-to-plane set carries identity information: its records are whitened, [L^T e | L^T Ji |
    L^T Jj] with Omega = L L^T at the current state, which gives the same quadratic form and the same chi2 under every
    robust kernel."""
    edges = []
    for es in prob.edges:
        if es.etype in (E_V_V_GICP, E_XYZ_VSC):
            plpl = es.etype == E_V_V_GICP and es.params is not None
            info = np.broadcast_to(np.eye(3), (len(es.v0), 3, 3)).copy() if plpl else es.info.copy()
            edges.append(EdgeSet(32 + 3, es.v0.copy(), es.v1.copy(), None, info, None))
        else:
            edges.append(es)
    return Problem(prob.name + "/hostj", list(prob.vertices), edges, prob.pose_dim, prob.landmark_dim)


# ---------------------------------------------------------------- Sim3 pose graphs
def _sim3_mul(a, b):
    """(R, t, s) * (R, t, s) of similarity transforms x -> s R x + t, batched."""
    (Ra, ta, sa), (Rb, tb, sb) = a, b
    return Ra @ Rb, sa[:, None] * np.einsum("nij,nj->ni", Ra, tb) + ta, sa * sb


def _sim3_inv(a):
    R, t, s = a
    Rt = np.transpose(R, (0, 2, 1))
    return Rt, -np.einsum("nij,nj->ni", Rt, t) / s[:, None], 1.0 / s


def _sim3_vec(a):
    R, t, s = a
    return np.concatenate([t, rot_to_quat(R), s[:, None]], axis=1)


def sim3_pose_graph(num_poses: int = 40, loops: int = 80, rot_noise: float = 0.02, trans_noise: float = 0.03,
                    scale_noise: float = 0.02, drift: float = 0.03, seed: int = SEED) -> Problem:
    """A 7-DoF pose graph (VertexSim3Expmap keyframes, EdgeSim3): ``num_poses`` world->camera similarities on a ring
    of radius 5, the camera looking along the direction of travel, whose scale drifts as a monocular map's does: log
    s_i is a random walk of step ``drift``.  Odometry (i, i + 1) and ``loops`` closures (i, j), j > i + 1.  With the
    edge's error log(C Si Sj^-1) the measurement is C = N Sj Si^-1 of the true keyframes, N a random similarity of
    rotation angle ~ ``rot_noise``, translation ~ ``trans_noise`` and log scale +-(1 .. 2) ``scale_noise``: at the
    true keyframes an edge's error is log N.  Information: sigma^-1 (I + A)(I + A)^T sigma^-1 in (omega, upsilon,
    sigma) order, A random per edge: SPD, not diagonal.  Keyframe 0 is fixed; the others start at the truth moved by a
    similarity of 0.03 rad, 0.05 and 3 % of scale, so that every edge's rotation error stays far below 2 rad."""
    n = num_poses
    rng = _rng(seed, 80)
    th = 2 * math.pi * np.arange(n) / max(n, 8)
    pos = np.stack([5 * np.cos(th), 5 * np.sin(th), 0.05 * np.arange(n)], 1)
    zero, one = np.zeros(n), np.ones(n)
    Rc = np.stack([np.stack([np.cos(th), zero, -np.sin(th)], 1), np.stack([np.sin(th), zero, np.cos(th)], 1),
                   np.stack([zero, -one, zero], 1)], 1) @ _small_rot(rng, n, 0.1)
    s = np.exp(np.cumsum(np.concatenate([[0.0], rng.standard_normal(n - 1) * drift])))
    Rw = np.transpose(Rc, (0, 2, 1))
    truth = (Rw, -s[:, None] * np.einsum("nij,nj->ni", Rw, pos), s)
    a, b = _loop_pairs(rng, n, loops)
    m = len(a)
    sel = lambda S, k: (S[0][k], S[1][k], S[2][k])  # noqa: E731
    sn = np.exp(rng.choice([-1.0, 1.0], m) * scale_noise * (1.0 + rng.random(m)))
    noise = (_small_rot(rng, m, rot_noise), rng.standard_normal((m, 3)) * trans_noise, sn)
    meas = _sim3_vec(_sim3_mul(noise, _sim3_mul(sel(truth, b), _sim3_inv(sel(truth, a)))))
    info = _spd_info(rng, m, np.array([rot_noise] * 3 + [trans_noise] * 3 + [scale_noise]))
    move = (_small_rot(rng, n, 0.03), rng.standard_normal((n, 3)) * 0.05, np.exp(rng.standard_normal(n) * 0.03))
    est = _sim3_vec(_sim3_mul(move, truth))
    est[0] = _sim3_vec(truth)[0]
    fixed = np.zeros(n, np.int32)
    fixed[0] = 1
    ids = np.arange(n, dtype=np.int32)
    verts = VertexSet(V_SIM3, ids, est, fixed, np.zeros(n, np.int32))
    edges = EdgeSet(E_SIM3, ids[a].copy(), ids[b].copy(), meas, info)
    return Problem(f"sim3_{n}l{loops}", [verts], [edges], 7, 0)


def sim3_twin(prob: Problem) -> Problem:
    """The host-Jacobian twin of a Sim3 graph: every E_SIM3 set as an E_HOSTJ(7) set (39) between the same vertices
    with the same information; the caller supplies the payload."""
    edges = [EdgeSet(32 + 7, es.v0.copy(), es.v1.copy(), None, es.info.copy(), None) if es.etype == E_SIM3 else es
             for es in prob.edges]
    return Problem(prob.name + "/hostj", list(prob.vertices), edges, prob.pose_dim, prob.landmark_dim)


# ---------------------------------------------------------------- examples/bal
def bal_project(cam: np.ndarray, X: np.ndarray) -> np.ndarray:
    """EdgeObservationBAL's prediction (bal_example.cpp:191-238) for cameras [n, 9] rx ry rz tx ty tz f k1 k2 and points
    [n, 3]: P = R(w) X + t by Rodrigues' formula (theta == 0: X + w x X), p = -P.xy / P.z, f (1 + k1 r2 + k2 r2^2) p."""
    w, t = cam[:, :3], cam[:, 3:6]
    th = np.sqrt(np.sum(w * w, 1))[:, None]
    v = w / np.where(th > 0, th, 1.0)
    c, s = np.cos(th), np.sin(th)
    P = np.where(th > 0, X * c + np.cross(v, X) * s + v * np.sum(v * X, 1)[:, None] * (1 - c), X + np.cross(w, X)) + t
    p = -P[:, :2] / P[:, 2:3]
    r2 = np.sum(p * p, 1)
    return (cam[:, 6] * (1 + cam[:, 7] * r2 + cam[:, 8] * r2 * r2))[:, None] * p


def bal(num_cameras: int = 49, num_points: int = 7776, num_observations: int = 31843, pixel_noise: float = 0.5,
        point_noise: float = 0.01, seed: int = SEED) -> Problem:
    """A synthetic "Bundle Adjustment in the Large" problem; the defaults are the shape of Ladybug's
    problem-49-7776-pre.txt. Cameras (V_CAM_BAL, ids 0 .. num_cameras-1) drive along x looking down -z with small
    attitudes, f 400 - 600, |k1| <= 0.05, |k2| <= 0.01; points (V_XYZ, marginalised, ids behind the cameras') lie 4 - 7
    in front of the track. Every point is seen by at least two cameras of a window of consecutive ones, the remaining
    observations are spread at random; Omega = I2, nothing is fixed (as bal_example leaves the gauge to LM)."""
    rng = _rng(seed, 90)
    nc, npt, no = num_cameras, num_points, num_observations
    assert nc >= 2 and no >= 2 * npt and no <= nc * npt
    x0 = 0.25 * np.arange(nc)
    w = 0.05 * rng.standard_normal((nc, 3))
    cams = np.concatenate([w, np.stack([-x0, np.zeros(nc), np.zeros(nc)], 1) + 0.02 * rng.standard_normal((nc, 3)),
                           rng.uniform(400, 600, (nc, 1)), rng.uniform(-0.05, 0.05, (nc, 1)), rng.uniform(-0.01, 0.01, (nc, 1))], 1)
    cnt = 2 + rng.multinomial(no - 2 * npt, np.full(npt, 1.0 / npt))
    cnt = np.minimum(cnt, nc)
    short = no - int(cnt.sum())  # counts cut at num_cameras: hand the rest to the points with room, in order
    for k in range(npt):
        if short <= 0:
            break
        add = min(short, nc - int(cnt[k]))
        cnt[k] += add
        short -= add
    first = np.array([rng.integers(0, nc - c + 1) for c in cnt])
    ci = np.concatenate([f + np.arange(c) for f, c in zip(first, cnt)])
    pi = np.repeat(np.arange(npt), cnt)
    centre = x0[first] + 0.25 * (cnt - 1) / 2.0  # in front of the middle of the point's window
    pts = np.stack([centre + rng.uniform(-1.5, 1.5, npt), rng.uniform(-1.5, 1.5, npt), -rng.uniform(4.0, 7.0, npt)], 1)
    obs = bal_project(cams[ci], pts[pi]) + pixel_noise * rng.standard_normal((len(ci), 2))
    info = np.broadcast_to(np.eye(2), (len(ci), 2, 2)).copy()
    start = pts + point_noise * rng.standard_normal((npt, 3))
    verts = [VertexSet(V_CAM_BAL, np.arange(nc, dtype=np.int32), cams, np.zeros(nc, np.int32), np.zeros(nc, np.int32)),
             VertexSet(V_XYZ, (nc + np.arange(npt)).astype(np.int32), start, np.zeros(npt, np.int32), np.ones(npt, np.int32))]
    return Problem(f"bal_{nc}_{npt}", verts, [EdgeSet(E_OBSERVATION_BAL, ci.astype(np.int32), (nc + pi).astype(np.int32), obs, info)], 9, 3)
