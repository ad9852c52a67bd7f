"""Helpers of the edge-level tests (tests/test_gpu_edge_levels.py, tests/test_edge_levels_host.py): one numpy graph
over every device edge family (the restatements of unary_ref, slam3d_ref and expmap_ref), per-edge chi2 and camera-frame
depth from it, sub-problems by edge mask (the "twin" a level filter must equal), the host classification rule and the
test inputs. Nothing here touches the device."""
import numpy as np

import expmap_ref
import slam3d_ref
from g2o_amd import synth

E_BA, E_STEREO_BA = synth.E_SE3_PROJECT_XYZ, synth.E_STEREO_SE3_PROJECT_XYZ
E_MONO, E_STEREO = expmap_ref.E_MONO, expmap_ref.E_STEREO
LEVEL_KEEP = -2147483648


class Graph(expmap_ref.Graph):
    """expmap_ref.Graph (priors, SE2, SE2-XY, EdgeSE3Expmap, the pose-only and BA projections) with slam3d_ref's
    EdgeSE3 and landmark edges."""

    def edge(self, es, k, est=None, binary=None):
        if es.v1 is not None and (es.etype in slam3d_ref.KINDS or es.etype == synth.E_SE3_QUAT):
            return slam3d_ref.Graph.edge(self, es, k, est, binary)
        return super().edge(es, k, est, binary)


def edge_set(prob, etype):
    (es,) = [e for e in prob.edges if e.etype == etype]
    return es


def edge_chi2(prob, etype, est=None):
    """Edge::chi2() = e^T Omega e of every edge of the type (active or not), in edge order."""
    g, es = Graph(prob), edge_set(prob, etype)
    out = np.zeros(len(es.v0))
    for k in range(len(es.v0)):
        e, _ = g.edge(es, k, est)
        out[k] = float(e @ es.info[k] @ e)
    return out


def depth_z(prob, etype, est=None):
    """The point's z in the camera frame per edge of a projection type (isDepthPositive is z > 0)."""
    g, es = Graph(prob), edge_set(prob, etype)
    z = np.zeros(len(es.v0))
    for k in range(len(es.v0)):
        if etype in (E_MONO, E_STEREO):
            T, xw = g._est(est, es.v0[k])[1], es.params[k, :3]
        else:
            T, xw = g._est(est, es.v1[k])[1], g._est(est, es.v0[k])[1]
        z[k] = (expmap_ref.qrot(T[3:7], xw) + T[:3])[2]
    return z


def classify(chi2, chi2_max, z=None, levels=None, inlier=0, outlier=1):
    """The callers' rule: bad = chi2 > max || (check_depth && !(z > 0)); returns (levels, counts)."""
    over = chi2 > chi2_max
    behind = np.zeros_like(over) if z is None else ~(z > 0)
    bad = over | behind
    lv = np.zeros(len(chi2), np.int32) if levels is None else np.asarray(levels, np.int32).copy()
    if outlier != LEVEL_KEEP:
        lv[bad] = outlier
    if inlier != LEVEL_KEEP:
        lv[~bad] = inlier
    return lv, dict(over_chi2=int(over.sum()), depth_failed=int(behind.sum()), bad=int(bad.sum()))


def gap_threshold(chi2, q=0.8, window=0.1):
    """A threshold in the middle of the widest gap between neighbouring sorted chi2 values near the q-quantile;
    returns (threshold, relative gap)."""
    s = np.sort(chi2)
    if len(s) == 1:
        return 0.5 * s[0], 0.5
    lo = max(int((q - window) * len(s)), 0)
    hi = min(max(int((q + window) * len(s)), lo + 2), len(s))
    k = lo + int(np.argmax(np.diff(s[lo:hi])))
    thr = 0.5 * (s[k] + s[k + 1])
    return thr, (s[k + 1] - s[k]) / thr


def subproblem(prob, keep, name="twin"):
    """Every vertex of prob and, per edge type, the edges whose keep[etype] entry is true (a type without an entry
    whole; a set left empty dropped)."""
    edges = []
    for es in prob.edges:
        m = keep.get(es.etype)
        if m is None:
            edges.append(es)
            continue
        m = np.asarray(m, bool)
        if not m.any():
            continue
        edges.append(synth.EdgeSet(es.etype, es.v0[m], None if es.v1 is None else es.v1[m], es.meas[m], es.info[m],
                                   None if es.params is None else es.params[m]))
    return synth.Problem(prob.name + "_" + name, prob.vertices, edges, prob.pose_dim, prob.landmark_dim)


def third_levels(prob, seed):
    """{edge type: levels} with a pseudo-random third of the edges of every type at level 1."""
    rng = np.random.default_rng(seed)
    out = {}
    for es in prob.edges:
        n = len(es.v0)
        lv = np.zeros(n, np.int32)
        lv[rng.permutation(n)[: n // 3]] = 1
        out[es.etype] = lv
    return out


def ba_levels(prob, seed):
    """third_levels of a BA graph (edge set 0: v0 the landmark) arranged so that one landmark has every observation at
    level 1 (it leaves the system) and another keeps a single one. Returns (levels, gone id, single id)."""
    lv = third_levels(prob, seed)
    es = prob.edges[0]
    pts = [vs for vs in prob.vertices if np.any(vs.marginalized)][0]
    gone, single = int(pts.ids[3]), int(pts.ids[7])
    l0 = lv[es.etype]
    for i in np.unique(es.v0):  # every other landmark keeps an observation on level 0
        rows = np.flatnonzero(es.v0 == i)
        if np.all(l0[rows] == 1):
            l0[rows[0]] = 0
    l0[es.v0 == gone] = 1
    rows = np.flatnonzero(es.v0 == single)
    l0[rows] = 1
    l0[rows[1]] = 0
    return lv, gone, single


def apply_levels(opt, levels):
    for etype, lv in levels.items():
        opt.set_edge_levels(etype, lv)


def slam2d_problem():
    """SE2 poses with XY landmarks: E_SE2 odometry and E_SE2_XY observations, Schur on the 3 x 2 blocks."""
    return synth.slam2d(num_poses=30, seed=synth.SEED + 3)


def behind_camera(prob, etype, rows, depth=-0.5):
    """A copy of a projection problem in which the points of the edges `rows` of the type sit behind their camera
    (camera-frame z = depth): BA types move the landmark (every edge of it follows), pose-only types their Xw. The
    measurements of the moved edges follow, so that every edge keeps the error (and the chi2, up to rounding) it had:
    an edge behind its camera is then no outlier by its chi2 alone."""
    g, es = Graph(prob), edge_set(prob, etype)
    verts, edges = list(prob.vertices), list(prob.edges)
    if etype in (E_MONO, E_STEREO):
        par = es.params.copy()
        for k in rows:
            T = g._est(None, es.v0[k])[1]
            pc = expmap_ref.qrot(T[3:7], par[k, :3]) + T[:3]
            pc[2] = depth
            qi = T[3:7] * np.array([-1, -1, -1, 1.0])
            par[k, :3] = expmap_ref.qrot(qi, pc - T[:3])
        edges[prob.edges.index(es)] = synth.EdgeSet(es.etype, es.v0, None, es.meas, es.info, par)
    else:
        vi = [i for i, vs in enumerate(verts) if vs.vtype == synth.V_XYZ][0]
        vs = verts[vi]
        est = vs.est.copy()
        for k in rows:
            T = g._est(None, es.v1[k])[1]
            r = int(np.flatnonzero(vs.ids == es.v0[k])[0])
            pc = expmap_ref.qrot(T[3:7], est[r]) + T[:3]
            pc[2] = depth
            qi = T[3:7] * np.array([-1, -1, -1, 1.0])
            est[r] = expmap_ref.qrot(qi, pc - T[:3])
        verts[vi] = synth.VertexSet(vs.vtype, vs.ids, est, vs.fixed, vs.marginalized)
    moved = synth.Problem(prob.name + "_behind", verts, edges, prob.pose_dim, prob.landmark_dim)
    g1, es1 = Graph(moved), edge_set(moved, etype)
    meas = es1.meas.copy()
    for k in range(len(es.v0)):
        e0, e1 = g.edge(es, k)[0], g1.edge(es1, k)[0]
        if not np.array_equal(e0, e1):
            meas[k] += e0 - e1
    edges[edges.index(es1)] = synth.EdgeSet(es1.etype, es1.v0, es1.v1, meas, es1.info, es1.params)
    return synth.Problem(moved.name, verts, edges, prob.pose_dim, prob.landmark_dim)
