"""g2o_amd — MI355X-native BlockSolver<p,l> backend for g2o.

Python mirror of the reference's operator/plugin interface for this path
(``g2o::SparseOptimizer`` + ``OptimizationAlgorithmLevenberg`` + the ``Solver``
plugin, see ``include/g2o_hip.h``) over the C ABI of ``libg2o_hip.so``.
The library is hand-written HIP for gfx950; there is no CPU fallback: every
compute call fails loudly when the library or a GPU is missing.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from . import synth  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("G2OHIP_LIB") or os.path.join(HERE, "libg2o_hip.so")


class BatchStats(C.Structure):
    """G2OBatchStatistics (core/batch_stats.h:42-72) + lambda."""
    _fields_ = [
        ("iteration", C.c_int), ("numVertices", C.c_int), ("numEdges", C.c_int),
        ("chi2", C.c_double), ("lambda_", C.c_double),
        ("timeResiduals", C.c_double), ("timeQuadraticForm", C.c_double),
        ("levenbergIterations", C.c_int),
        ("timeSchurComplement", C.c_double), ("timeSymbolicDecomposition", C.c_double),
        ("timeNumericDecomposition", C.c_double), ("timeLinearSolution", C.c_double),
        ("timeLinearSolver", C.c_double), ("timeUpdate", C.c_double), ("timeIteration", C.c_double),
        ("hessianDimension", C.c_longlong), ("hessianPoseDimension", C.c_longlong),
        ("hessianLandmarkDimension", C.c_longlong), ("choleskyNNZ", C.c_longlong),
    ]


class Config(C.Structure):
    _fields_ = [("max_trials_after_failure", C.c_int), ("user_lambda_init", C.c_double), ("verbose", C.c_int)]


# EdgeStereoSE3ProjectXYZ (include/g2o_hip.h G2OHIP_E_STEREO_SE3_PROJECT_XYZ): meas u_l v u_r, params fx fy cx cy bf
E_STEREO_SE3_PROJECT_XYZ = 6


# slam3d landmark edges (include/g2o_hip.h G2OHIP_E_SE3_XYZ*): v0 the VertexSE3 pose, v1 the point; meas x y z /
# u v depth / u v 1/depth; params the sensor offset x y z qx qy qz qw (XYZ: or None, the identity), the camera types'
# followed by fx fy cx cy
E_SE3_XYZ, E_SE3_XYZ_DEPTH, E_SE3_XYZ_DISPARITY = 7, 8, 9


# EdgeSE3Expmap (G2OHIP_E_SE3_EXPMAP): v0 = Ti, v1 = Tj, both V_SE3_EXPMAP; meas the SE3Quat C (tx ty tz qx qy qz qw)
E_SE3_EXPMAP = 10


# the sba types (include/g2o_hip.h G2OHIP_V_CAM, G2OHIP_E_PROJECT_P2MC / _P2SC): VertexCam, estimate x y z qx qy qz qw
# (camera-to-world) fx fy cx cy baseline; v0 the point, v1 the camera; meas u v / u v u_r; params None
V_CAM = 6
E_PROJECT_P2MC, E_PROJECT_P2SC = 11, 12


# offset and bearing edges (include/g2o_hip.h G2OHIP_E_SE3_OFFSET, _SE2_OFFSET, _SE2_XY_BEARING): EdgeSE3Offset between
# two V_SE3_QUAT (meas x y z qx qy qz qw, params [n, 14]: the from vertex's offset, then the to vertex's, or None),
# EdgeSE2Offset between two V_SE2 (meas x y theta, params [n, 6] or None), EdgeSE2PointXYBearing from a V_SE2 pose to a
# V_XY point (meas one angle, info 1x1, params None); EDGE_TAGS: their .g2o tags
E_SE3_OFFSET, E_SE2_OFFSET, E_SE2_XY_BEARING = 13, 14, 15
EDGE_TAGS = {E_SE3_OFFSET: "EDGE_SE3_OFFSET", E_SE2_OFFSET: "EDGE_SE2_OFFSET", E_SE2_XY_BEARING: "EDGE_BEARING_SE2_XY"}


# g2o's own BA edges on a CameraParameters parameter (include/g2o_hip.h G2OHIP_E_PROJECT_XYZ2UV / _XYZ2UVU): v0 the
# V_XYZ point, v1 the V_SE3_EXPMAP camera; meas u v / u v u_r; params [n, 4] focal_length cx cy baseline
E_PROJECT_XYZ2UV, E_PROJECT_XYZ2UVU = 23, 24


# types_icp (include/g2o_hip.h G2OHIP_E_V_V_GICP, G2OHIP_E_XYZ_VSC): Edge_V_V_GICP between two V_SE3_QUAT (meas [n, 12]
# pos0 normal0 pos1 normal1, info [n, 3, 3] the point-to-plane information, params None; or params [n, 12], cov0 then
# cov1 as packed upper triangles 00 01 11 02 12 22: the whole set plane-to-plane, info may then be None);
# Edge_XYZ_VSC from a V_XYZ point to a V_SE3_QUAT camera standing for the VertexSCam (meas u v u_r, params [n, 5]
# fx fy cx cy baseline). ICP_EDGE_TAGS: the .g2o tag (Edge_XYZ_VSC has none: the reference's read / write return false);
# kept beside EDGE_TAGS, which holds the offset and bearing tags alone
E_V_V_GICP, E_XYZ_VSC = 25, 26
ICP_EDGE_TAGS = {E_V_V_GICP: "EDGE_V_V_GICP"}


# types/sim3 (include/g2o_hip.h G2OHIP_V_SIM3, G2OHIP_E_SIM3): VertexSim3Expmap, estimate tx ty tz qx qy qz qw s
# (world->camera), dimension 7; EdgeSim3 between two of them, meas a Sim3 in the same layout, info [n, 7, 7] in (omega,
# upsilon, sigma) order, params None. SIM3_TAGS: their .g2o tags (load(sim3=True))
V_SIM3 = 7
E_SIM3 = 27
SIM3_TAGS = {"vertex": "VERTEX_SIM3:EXPMAP", "edge": "EDGE_SIM3:EXPMAP"}
# EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ (G2OHIP_E_SIM3_PROJECT_XYZ, ..._INVERSE_XYZ): v0 a fixed V_XYZ point, v1 a
# V_SIM3; meas [n, 2] u v, info [n, 2, 2], params None: the intrinsics are camera 1 (inverse: camera 2) of v1,
# SparseOptimizer.set_sim3_cameras. SIM3_PROJECT_TAGS: their .g2o tags (load(sim3=True, sim3_project=True))
E_SIM3_PROJECT, E_SIM3_PROJECT_INVERSE = 28, 29
SIM3_PROJECT_TAGS = {E_SIM3_PROJECT: "EDGE_PROJECT_SIM3_XYZ:EXPMAP",
                     E_SIM3_PROJECT_INVERSE: "EDGE_PROJECT_INVERSE_SIM3_XYZ:EXPMAP"}
# examples/bal (G2OHIP_V_CAM_BAL, G2OHIP_E_OBSERVATION_BAL): VertexCameraBAL, estimate [n, 9] rx ry rz tx ty tz f k1 k2,
# dimension 9; EdgeObservationBAL from it (v0) to a V_XYZ point (v1), meas [n, 2] u v, info [n, 2, 2], params None. No
# .g2o tag: SparseOptimizer.load_bal / save_bal read and write the BAL text format
V_CAM_BAL = synth.V_CAM_BAL
E_OBSERVATION_BAL = synth.E_OBSERVATION_BAL


# EdgeGICP::prec0 / cov0 in numpy, and the packed form of the covariances (ValueError on a normal parallel to (0,1,0))
gicp_prec, gicp_cov, gicp_pack = synth.gicp_prec, synth.gicp_cov, synth.gicp_pack


# edge types the device does not know: host-supplied error + Jacobians (include/g2o_hip.h G2OHIP_E_HOSTJ)
def E_HOSTJ(D: int) -> int:
    return 32 + D


# unary edge types (BaseUnaryEdge; include/g2o_hip.h G2OHIP_E_*_PRIOR): EdgeSet.v1 is None
E_SE2_PRIOR, E_SE2_XY_PRIOR, E_XY_PRIOR, E_SE3_PRIOR, E_XYZ_PRIOR = 16, 17, 18, 19, 20


# pose-only projections on a V_SE3_EXPMAP camera (G2OHIP_E_*_ONLYPOSE), unary: meas u v / u_l v u_r; params
# Xw.x Xw.y Xw.z fx fy cx cy (stereo + bf)
E_SE3_PROJECT_XYZ_ONLYPOSE, E_STEREO_SE3_PROJECT_XYZ_ONLYPOSE = 21, 22


# any other BaseUnaryEdge: host-supplied error + Jacobian, payload [e | Ji] per edge (G2OHIP_E_HOSTJ_UNARY)
def E_HOSTJ_UNARY(D: int) -> int:
    return 48 + D


# g2ohip_load_g2o_ex flags
LOAD_UNARY = 1
LOAD_SLAM3D = 2
LOAD_EXPMAP = 4
LOAD_SBA = 8
LOAD_OFFSET = 16
LOAD_CAMERAPARAMS = 32
LOAD_ICP = 64
LOAD_SIM3 = 128
LOAD_SIM3_PROJECT = 256

# robust kernels (G2OHIP_RK_*, robust_kernel_impl.cpp)
RK = {"none": 0, "Huber": 1, "PseudoHuber": 2, "Cauchy": 3, "GemanMcClure": 4, "Welsch": 5, "Fair": 6, "Tukey": 7,
      "Saturated": 8, "DCS": 9}

HOST_EDGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double))

EXPORTS = [
    "g2ohip_graph_create", "g2ohip_graph_destroy", "g2ohip_add_vertices", "g2ohip_add_edges",
    "g2ohip_load_g2o", "g2ohip_load_g2o_ex", "g2ohip_save_g2o", "g2ohip_num_vertices", "g2ohip_num_edges",
    "g2ohip_set_robust_kernel", "g2ohip_set_host_jacobians", "g2ohip_set_host_edge_callback",
    "g2ohip_solver_diag_absmax", "g2ohip_solver_set_eta", "g2ohip_solver_linear_iterations",
    "g2ohip_get_estimates", "g2ohip_set_estimates", "g2ohip_minimal_state", "g2ohip_set_algorithm",
    "g2ohip_initialize", "g2ohip_chi2", "g2ohip_optimize", "g2ohip_optimize_step",
    "g2ohip_solver_build_structure", "g2ohip_solver_build_system", "g2ohip_solver_set_lambda",
    "g2ohip_solver_restore_diagonal", "g2ohip_solver_solve", "g2ohip_solver_vector_size", "g2ohip_solver_block_dims",
    "g2ohip_solver_get_x", "g2ohip_solver_get_b", "g2ohip_solver_multiply_hessian",
    "g2ohip_solver_linear_residual", "g2ohip_solver_factor_info", "g2ohip_solver_compute_marginals", "g2ohip_update", "g2ohip_push", "g2ohip_pop",
    "g2ohip_discard_top", "g2ohip_stage", "g2ohip_linear_solve_ccs", "g2ohip_linear_solve_ccs_ex",
    "g2ohip_comm_unique_id",
    "g2ohip_set_comm", "g2ohip_set_comm_local", "g2ohip_comm_selftest", "g2ohip_comm_selftest_rs", "g2ohip_symbolic_analyze", "g2ohip_symbolic_supernodes", "g2ohip_dist_plan", "g2ohip_local_landmarks", "g2ohip_enable_kernel_timing",
    "g2ohip_kernel_timing_only", "g2ohip_set_stats_level", "g2ohip_kernel_ms",
    "g2ohip_kernel_count", "g2ohip_kernel_bytes", "g2ohip_kernel_flops", "g2ohip_last_error",
    "g2ohip_version", "g2ohip_host_payload_len", "g2ohip_solver_save_hessian", "g2ohip_solver_set_write_debug",
    "g2ohip_comm_local_reduce_host", "g2ohip_runtime_info", "g2ohip_device_synchronize", "g2ohip_lm_scale_factor",
    "g2ohip_measure_peaks", "g2ohip_set_dogleg_params", "g2ohip_dogleg_state", "g2ohip_dogleg_blend",
    "g2ohip_dogleg_next_delta", "g2ohip_structure_only_calc",
    "g2ohip_set_edge_levels", "g2ohip_get_edge_levels", "g2ohip_initialize_level", "g2ohip_edge_chi2",
    "g2ohip_classify_edges", "g2ohip_set_pair_major", "g2ohip_pair_major_info", "g2ohip_set_sim3_fix_scale",
    "g2ohip_set_sim3_cameras", "g2ohip_load_bal", "g2ohip_save_bal",
]

# G2OHIP_LEVEL_KEEP: classify_edges leaves the level of the edges on that side as it is
LEVEL_KEEP = -2147483648


def build(arch: str = "gfx950") -> None:
    """Compile libg2o_hip.so in-tree with hipcc (cross-compiles without a GPU)."""
    subprocess.run(["make", "-s", "-C", HERE, f"ARCH={arch}", "-j8"], check=True)


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} not built: run g2o_amd.build() (hipcc --offload-arch=gfx950)")
    L = C.CDLL(LIB_PATH)
    P, I, D, LL = C.c_void_p, C.c_int, C.c_double, C.c_longlong
    sig = {
        "g2ohip_graph_create": ([I], P),
        "g2ohip_graph_destroy": ([P], None),
        "g2ohip_add_vertices": ([P, I, I, P, P, P, P], I),
        "g2ohip_add_edges": ([P, I, I, P, P, P, P, P], I),
        "g2ohip_load_g2o": ([P, C.c_char_p, I], I),
        "g2ohip_load_g2o_ex": ([P, C.c_char_p, I, C.c_uint], I),
        "g2ohip_save_g2o": ([P, C.c_char_p], I),
        "g2ohip_load_bal": ([P, C.c_char_p, I], I),
        "g2ohip_save_bal": ([P, C.c_char_p], I),
        "g2ohip_num_vertices": ([P], I),
        "g2ohip_num_edges": ([P], I),
        "g2ohip_set_robust_kernel": ([P, I, I, D], I),
        "g2ohip_set_host_jacobians": ([P, I, P], I),
        "g2ohip_set_host_edge_callback": ([P, HOST_EDGE_FN, P], I),
        "g2ohip_solver_diag_absmax": ([P, P], I),
        "g2ohip_solver_set_eta": ([P, D], I),
        "g2ohip_solver_linear_iterations": ([P], I),
        "g2ohip_get_estimates": ([P, I, P, P], I),
        "g2ohip_set_estimates": ([P, I, P], I),
        "g2ohip_minimal_state": ([P, P], I),
        "g2ohip_set_algorithm": ([P, C.c_char_p], I),
        "g2ohip_initialize": ([P], I),
        "g2ohip_initialize_level": ([P, I], I),
        "g2ohip_set_edge_levels": ([P, I, I, P, P], I),
        "g2ohip_get_edge_levels": ([P, I, P, I], I),
        "g2ohip_edge_chi2": ([P, I, P, P], I),
        "g2ohip_classify_edges": ([P, I, D, I, I, I, P], I),
        "g2ohip_update_initialization": ([P], I),
        "g2ohip_chi2": ([P], D),
        "g2ohip_optimize": ([P, P, I, P], I),
        "g2ohip_optimize_step": ([P, P, I, P], I),
        "g2ohip_solver_build_structure": ([P], I),
        "g2ohip_solver_build_system": ([P], I),
        "g2ohip_solver_set_lambda": ([P, D, I], I),
        "g2ohip_solver_restore_diagonal": ([P], I),
        "g2ohip_solver_solve": ([P], I),
        "g2ohip_solver_vector_size": ([P], LL),
        "g2ohip_solver_block_dims": ([P, P], I),
        "g2ohip_solver_get_x": ([P, P], I),
        "g2ohip_solver_get_b": ([P, P], I),
        "g2ohip_solver_multiply_hessian": ([P, P, P], I),
        "g2ohip_solver_linear_residual": ([P, P], I),
        "g2ohip_solver_factor_info": ([P, P, I], I),
        "g2ohip_solver_compute_marginals": ([P, I, P, P, P], I),
        "g2ohip_update": ([P, P], I),
        "g2ohip_push": ([P], I),
        "g2ohip_pop": ([P], I),
        "g2ohip_discard_top": ([P], I),
        "g2ohip_stage": ([P, D, P, P, P, P, P], I),
        "g2ohip_linear_solve_ccs": ([I, I, P, P, P, P, P, I, P], I),
        "g2ohip_linear_solve_ccs_ex": ([I, I, P, P, P, P, P, I, P, P, I], I),
        "g2ohip_comm_unique_id": ([P], I),
        "g2ohip_set_comm": ([P, P, I, I], I),
        "g2ohip_set_comm_local": ([P, C.c_char_p, I, I], I),
        "g2ohip_comm_selftest": ([I, P, I, P, P], I),
        "g2ohip_comm_selftest_rs": ([I, P, I, P, P, P], I),
        "g2ohip_debug_phases": ([P, I], I),
        "g2ohip_symbolic_analyze": ([I, I, I, P, P, P, P], I),
        "g2ohip_symbolic_supernodes": ([I, I, I, P, P, P, P, P, I], I),
        "g2ohip_dist_plan": ([I, I, I, P, P, I, I, I, P, P, P, I], I),
        "g2ohip_local_landmarks": ([P, P, I], I),
        "g2ohip_enable_kernel_timing": ([P, I], None),
        "g2ohip_kernel_timing_only": ([P, C.c_char_p], None),
        "g2ohip_set_stats_level": ([P, I], None),
        "g2ohip_kernel_ms": ([P, C.c_char_p], D),
        "g2ohip_kernel_count": ([P, C.c_char_p], LL),
        "g2ohip_kernel_bytes": ([P, C.c_char_p], D),
        "g2ohip_kernel_flops": ([P, C.c_char_p], D),
        "g2ohip_last_error": ([], C.c_char_p),
        "g2ohip_version": ([], C.c_char_p),
        "g2ohip_lm_scale_factor": ([D], D),
        "g2ohip_measure_peaks": ([I, P, I], I),
        "g2ohip_set_dogleg_params": ([P, D, I, D, D], I),
        "g2ohip_set_pair_major": ([P, I], I),
        "g2ohip_pair_major_info": ([P, P], I),
        "g2ohip_set_sim3_fix_scale": ([P, I], I),
        "g2ohip_set_sim3_cameras": ([P, I, P, P, P], I),
        "g2ohip_dogleg_state": ([P, P, I], I),
        "g2ohip_dogleg_blend": ([D, D, D, D, D, D, P], I),
        "g2ohip_dogleg_next_delta": ([D, D, D], D),
        "g2ohip_structure_only_calc": ([P, I, P, I, I, P], I),
        "g2ohip_host_payload_len": ([P, I], LL),
        "g2ohip_solver_save_hessian": ([P, C.c_char_p], I),
        "g2ohip_solver_set_write_debug": ([P, I], I),
        "g2ohip_comm_local_reduce_host": ([C.c_char_p, I, I, P, LL, I], I),
        "g2ohip_runtime_info": ([C.c_char_p, I], I),
        "g2ohip_device_synchronize": ([I], I),
    }
    for name, (args, res) in sig.items():
        f = getattr(L, name)
        f.argtypes = args
        f.restype = res
    _lib = L
    return L


def runtime_info() -> dict:
    """The HIP runtime / RCCL this library is bound to (resolved library paths + versions)."""
    import json
    buf = C.create_string_buffer(2048)
    lib().g2ohip_runtime_info(buf, len(buf))
    return json.loads(buf.value.decode())


def device_synchronize(device: int = 0) -> None:
    _check(lib().g2ohip_device_synchronize(device), "device_synchronize")


def dogleg_blend(hgn_norm, hsd_norm, hsd_sq, c, bma_sq, delta):
    """The dogleg trial's step choice as host and device take it: (step type 1 SD / 2 GN / 3 DL, coef0, coef1) with
    hdl = coef0 hsd + coef1 hgn (optimization_algorithm_dogleg.cpp:153-175). Needs no GPU."""
    coef = np.zeros(2)
    step = lib().g2ohip_dogleg_blend(hgn_norm, hsd_norm, hsd_sq, c, bma_sq, delta, _p(coef))
    return int(step), float(coef[0]), float(coef[1])


def dogleg_next_delta(delta, rho, hdl_norm) -> float:
    """The trust-region update (optimization_algorithm_dogleg.cpp:199-203). Needs no GPU."""
    return float(lib().g2ohip_dogleg_next_delta(delta, rho, hdl_norm))


def measure_peaks(device: int = 0) -> dict:
    """Measured roofline peaks of the device (g2ohip_measure_peaks): HBM streaming copy, FP64 MFMA and VALU issue rates."""
    out = np.zeros(4)
    _check(lib().g2ohip_measure_peaks(device, _p(out), 4), "measure_peaks")
    return {"hbm_copy_GBps": float(out[0]), "fp64_mfma_TFps": float(out[1]), "fp64_valu_TFps": float(out[2]),
            "cus": int(out[3])}


def comm_local_reduce_host(group_key: str, rank: int, nranks: int, buf, is_max: bool = False):
    """The in-process test transport's host reduction (collective-consistency checked); buf is reduced in place."""
    _check(lib().g2ohip_comm_local_reduce_host(group_key.encode(), rank, nranks, _p(buf), buf.size, int(is_max)),
           "comm_local_reduce_host")
    return buf


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def last_error() -> str:
    return lib().g2ohip_last_error().decode()


class G2OHipError(RuntimeError):
    pass


def _check(code, what):
    if code < 0:
        raise G2OHipError(f"{what} failed ({code}): {last_error()}")
    return code


def symbolic_analyze(nblocks: int, bdim: int, bi, bj):
    """Host-only symbolic analysis (ordering + supernodes); returns (perm, stats dict)."""
    bi = np.ascontiguousarray(bi, np.int32)
    bj = np.ascontiguousarray(bj, np.int32)
    perm = np.zeros(nblocks * bdim, np.int32)
    st = np.zeros(5)
    n = lib().g2ohip_symbolic_analyze(nblocks, bdim, len(bi), _p(bi), _p(bj), _p(perm), _p(st))
    _check(n, "symbolic_analyze")
    return perm, dict(nnzL=st[0], flops=st[1], supernodes=int(st[2]), levels=int(st[3]), panel_steps=int(st[4]))


def symbolic_supernodes(nblocks: int, bdim: int, bi, bj):
    """Host-only: (ns, nr, level) arrays of the supernodes symbolic_analyze finds (scalar columns, scalar rows below
    the diagonal block, level with leaves 0)."""
    bi = np.ascontiguousarray(bi, np.int32)
    bj = np.ascontiguousarray(bj, np.int32)
    ns, nr, lv = (np.zeros(nblocks, np.int32) for _ in range(3))
    m = lib().g2ohip_symbolic_supernodes(nblocks, bdim, len(bi), _p(bi), _p(bj), _p(ns), _p(nr), _p(lv), nblocks)
    _check(m, "symbolic_supernodes")
    return ns[:m], nr[:m], lv[:m]


DIST_PLAN_KEYS = ("distributed", "rank_subtrees_s", "shared_s", "replicated_s", "exchange_s", "input_s",
                  "input_replicated_s", "max_rank_subtrees_s", "root_allgather_doubles", "rs_segment_doubles",
                  "rs_tail_doubles", "supernodes", "shard_s", "shard_replicated_s")


def dist_plan(nblocks: int, bdim: int, bi, bj, nranks: int, rank: int = 0, reduce_scatter: bool = True,
              aligned: bool = True, pose_work=None):
    """Host-only: the distributed factorization's cut for `nranks` landmark shards (the model the solver's setup
    runs; aligned: shards follow the cut, the default); returns (model dict, per-supernode owner
    array: rank, -1 shared)."""
    bi = np.ascontiguousarray(bi, np.int32)
    bj = np.ascontiguousarray(bj, np.int32)
    out = np.zeros(len(DIST_PLAN_KEYS))
    cap = 4 * nblocks + 16
    owner = np.full(cap, -1, np.int32)
    pw = None if pose_work is None else np.ascontiguousarray(pose_work, np.float64)
    n = lib().g2ohip_dist_plan(nblocks, bdim, len(bi), _p(bi), _p(bj), nranks, rank,
                               int(reduce_scatter) | (2 if aligned else 0), None if pw is None else _p(pw), _p(out),
                               _p(owner), cap)
    _check(n, "dist_plan")
    d = dict(zip(DIST_PLAN_KEYS, out.tolist()))
    return d, owner[:n]


# g2ohip_linear_solve_ccs_ex's info slots: the leading FACTOR_INFO_KEYS, then the deferred-L21 count
CCS_INFO_KEYS = ("n", "nnzL", "flops", "supernodes", "levels", "max_front", "blocked_fronts", "inplace_levels",
                 "prescatter_levels", "syrk_launches", "bwd_rounds", "deferred_l21_fronts")


def linear_solve_ccs(n, Ap, Ai, Ax, b, block_dim=1, device=0, info=False):
    """LinearSolver::solve on an upper-CCS matrix (LinearSolverCCS contract); info=True also returns the schedule
    summary of the factorization (CCS_INFO_KEYS) as a dict: (ok, x, info)."""
    Ap = np.ascontiguousarray(Ap, np.int32)
    Ai = np.ascontiguousarray(Ai, np.int32)
    Ax = np.ascontiguousarray(Ax, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    x = np.zeros(n)
    nb = n // block_dim
    ends = np.arange(1, nb + 1, dtype=np.int32) * block_dim
    if not info:
        r = lib().g2ohip_linear_solve_ccs(device, n, _p(Ap), _p(Ai), _p(Ax), _p(b), _p(x), nb, _p(ends))
        _check(r, "linear_solve_ccs")
        return bool(r), x
    out = np.zeros(len(CCS_INFO_KEYS))
    r = lib().g2ohip_linear_solve_ccs_ex(device, n, _p(Ap), _p(Ai), _p(Ax), _p(b), _p(x), nb, _p(ends), _p(out),
                                         len(out))
    _check(r, "linear_solve_ccs")
    return bool(r), x, dict(zip(CCS_INFO_KEYS, out.tolist()))


class SparseOptimizer:
    """g2o::SparseOptimizer with a device-resident ``lm_hip_*``, ``gn_hip_*`` or ``dl_hip_*`` algorithm
    (sparse_optimizer.h; optimization_algorithm_levenberg.h, ..._gauss_newton.h, ..._dogleg.h)."""

    def __init__(self, device: int = 0):
        self.h = lib().g2ohip_graph_create(device)
        if not self.h:
            raise G2OHipError(f"g2ohip_graph_create failed: {last_error()}")

    def close(self):
        if getattr(self, "h", None):
            lib().g2ohip_graph_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    # ---- OptimizableGraph ----
    def add_vertices(self, vs):
        ids = np.ascontiguousarray(vs.ids, np.int32)
        est = np.ascontiguousarray(vs.est, np.float64)
        ed = synth.EST_DIM.get(vs.vtype)
        if ed is not None and est.size != len(ids) * ed:  # the C side reads n * ed doubles
            raise G2OHipError(f"add_vertices: vertex type {vs.vtype} takes {ed} estimate values per vertex, got "
                              f"{est.size} for {len(ids)} vertices")
        fx = np.ascontiguousarray(vs.fixed, np.int32)
        mg = np.ascontiguousarray(vs.marginalized, np.int32)
        _check(lib().g2ohip_add_vertices(self.h, vs.vtype, len(ids), _p(ids), _p(est), _p(fx), _p(mg)),
               "add_vertices")

    def add_edges(self, es):
        v0 = np.ascontiguousarray(es.v0, np.int32)
        v1 = None if es.v1 is None else np.ascontiguousarray(es.v1, np.int32)  # None: a unary edge type
        meas = None if es.meas is None else np.ascontiguousarray(es.meas, np.float64)
        info = None if es.info is None else np.ascontiguousarray(es.info, np.float64)  # None: plane-to-plane GICP only
        par = None if es.params is None else np.ascontiguousarray(es.params, np.float64)
        pd = synth.PARAM_DIM.get(es.etype)
        md, D = synth.MEAS_DIM.get(es.etype), synth.ERR_DIM.get(es.etype)
        if es.etype in (E_V_V_GICP, E_XYZ_VSC, E_SIM3, E_SIM3_PROJECT, E_SIM3_PROJECT_INVERSE,
                        E_OBSERVATION_BAL):  # the C side reads n * md and n * D * D doubles
            if meas is None or meas.size != len(v0) * md:
                raise G2OHipError(f"add_edges: edge type {es.etype} takes {md} measurement values per edge, got "
                                  f"{0 if meas is None else meas.size} for {len(v0)} edges")
            if info is not None and info.size != len(v0) * D * D:
                raise G2OHipError(f"add_edges: edge type {es.etype} takes a {D}x{D} information per edge, got "
                                  f"{info.size} values for {len(v0)} edges")
        if par is not None and pd is not None and par.size != len(v0) * pd:  # the C side reads n * pd doubles
            raise G2OHipError(f"add_edges: edge type {es.etype} takes {pd} parameter values per edge, got {par.size} "
                              f"for {len(v0)} edges")
        _check(lib().g2ohip_add_edges(self.h, es.etype, len(v0), _p(v0), _p(v1), _p(meas), _p(info), _p(par)),
               "add_edges")

    def add_problem(self, prob):
        for vs in prob.vertices:
            self.add_vertices(vs)
        for es in prob.edges:
            self.add_edges(es)
        return self

    def set_robust_kernel(self, etype: int, kind, delta: float):
        """Edge::setRobustKernel for every edge of a type; kind = RK name or G2OHIP_RK_* number."""
        k = RK[kind] if isinstance(kind, str) else int(kind)
        _check(lib().g2ohip_set_robust_kernel(self.h, etype, k, float(delta)), "set_robust_kernel")

    def set_host_jacobians(self, etype: int, payload):
        """[e | Ji | Jj] row-major per edge of a host-J type (insertion order), at the device's estimates."""
        payload = np.ascontiguousarray(payload, np.float64)
        _check(lib().g2ohip_set_host_jacobians(self.h, etype, _p(payload)), "set_host_jacobians")

    def set_host_edge_callback(self, fn):
        """fn(edge_type, with_jacobians) -> payload ndarray, called by the device-resident loops for host-J edges."""
        if fn is None:
            self._host_cb = None
            _check(lib().g2ohip_set_host_edge_callback(self.h, HOST_EDGE_FN(), None), "set_host_edge_callback")
            return

        def tramp(user, etype, with_jac, out):
            try:
                pay = np.ascontiguousarray(fn(etype, bool(with_jac)), np.float64)
                want = lib().g2ohip_host_payload_len(self.h, etype)
                if want < 0 or pay.size != want:  # never write past the engine's payload buffer
                    raise G2OHipError(f"host edge callback returned {pay.size} doubles for edge type {etype}, "
                                      f"expected {want} (D * (1 + dim(v0) + dim(v1)) per edge, unary: "
                                      f"D * (1 + dim(v0)))")
                C.memmove(out, pay.ctypes.data, pay.nbytes)
                return 0
            except Exception:  # reported as a failed callback by the engine
                import traceback
                traceback.print_exc()
                return 1

        self._host_cb = HOST_EDGE_FN(tramp)  # keep alive
        _check(lib().g2ohip_set_host_edge_callback(self.h, self._host_cb, None), "set_host_edge_callback")

    def set_estimates(self, vtype: int, est):
        """Overwrite the estimates of one vertex type (insertion order): host-authoritative Solver mode."""
        est = np.ascontiguousarray(est, np.float64)
        _check(lib().g2ohip_set_estimates(self.h, vtype, _p(est)), "set_estimates")

    def load(self, path: str, marginalize_xyz: bool = True, unary: bool = False, slam3d: bool = False,
             expmap: bool = False, sba: bool = False, offset: bool = False, camparams: bool = False,
             icp: bool = False, sim3: bool = False, sim3_project: bool = False):
        """OptimizableGraph::load; unary=True also reads the prior tags (EDGE_PRIOR_SE2, EDGE_PRIOR_SE2_XY,
        EDGE_PRIOR_XY, EDGE_POINTXYZ_PRIOR, EDGE_SE3_PRIOR + PARAMS_SE3OFFSET), slam3d=True the 3D landmark tags
        (VERTEX_TRACKXYZ, EDGE_SE3_TRACKXYZ, EDGE_PROJECT_DEPTH, EDGE_PROJECT_DISPARITY + PARAMS_SE3OFFSET,
        PARAMS_CAMERACALIB), expmap=True EDGE_SE3:EXPMAP, sba=True the sba tags (VERTEX_CAM, EDGE_PROJECT_P2MC,
        EDGE_PROJECT_P2SC), offset=True the offset and bearing tags (EDGE_SE3_OFFSET, EDGE_SE2_OFFSET,
        EDGE_BEARING_SE2_XY + PARAMS_SE3OFFSET, PARAMS_SE2OFFSET), camparams=True g2o's own BA tags
        (EDGE_PROJECT_XYZ2UV:EXPMAP + PARAMS_CAMERAPARAMETERS), icp=True EDGE_V_V_GICP (point-to-plane, the information
        Edge_V_V_GICP::read builds; a normal0 parallel to (0,1,0) fails the load), sim3=True VERTEX_SIM3:EXPMAP and
        EDGE_SIM3:EXPMAP, sim3_project=True (with sim3) EDGE_PROJECT_SIM3_XYZ:EXPMAP and
        EDGE_PROJECT_INVERSE_SIM3_XYZ:EXPMAP, whose points must end up fixed (marginalize_xyz=False and FIX lines); all
        are skipped otherwise."""
        flags = ((LOAD_UNARY if unary else 0) | (LOAD_SLAM3D if slam3d else 0) | (LOAD_EXPMAP if expmap else 0) |
                 (LOAD_SBA if sba else 0) | (LOAD_OFFSET if offset else 0) | (LOAD_CAMERAPARAMS if camparams else 0) |
                 (LOAD_ICP if icp else 0) | (LOAD_SIM3 if sim3 else 0) | (LOAD_SIM3_PROJECT if sim3_project else 0))
        _check(lib().g2ohip_load_g2o_ex(self.h, path.encode(), int(marginalize_xyz), flags), "load")

    def num_vertices(self) -> int:
        return int(lib().g2ohip_num_vertices(self.h))

    def num_edges(self) -> int:
        return int(lib().g2ohip_num_edges(self.h))

    def save(self, path: str):
        _check(lib().g2ohip_save_g2o(self.h, path.encode()), "save")

    def load_bal(self, path: str, marginalize: bool = True):
        """g2ohip_load_bal: a "Bundle Adjustment in the Large" text file (bal_example.cpp:336-406). Cameras become
        V_CAM_BAL vertices with ids 0 .. ncams-1, points V_XYZ vertices behind them (marginalised by default),
        observations E_OBSERVATION_BAL edges with identity information."""
        _check(lib().g2ohip_load_bal(self.h, path.encode(), int(marginalize)), "load_bal")

    def save_bal(self, path: str):
        """g2ohip_save_bal: the same format from the current estimates, 17 significant digits."""
        _check(lib().g2ohip_save_bal(self.h, path.encode()), "save_bal")

    def save_hessian(self, path: str) -> bool:
        """Solver::saveHessian (block_solver.hpp:589-593): Hpp in Octave sparse-matrix text."""
        return bool(_check(lib().g2ohip_solver_save_hessian(self.h, path.encode()), "saveHessian"))

    def set_write_debug(self, on: bool = True):
        """Solver::setWriteDebug: a not-PD factorization writes debug.txt (linear_solver_csparse.h:127-133)."""
        _check(lib().g2ohip_solver_set_write_debug(self.h, int(on)), "setWriteDebug")

    def set_algorithm(self, name: str):
        _check(lib().g2ohip_set_algorithm(self.h, name.encode()), "set_algorithm")

    def set_pair_major(self, enable: bool = True):
        """g2ohip_set_pair_major: False keeps a graph of Edge_V_V_GICP edges on the generic slot path."""
        _check(lib().g2ohip_set_pair_major(self.h, int(bool(enable))), "set_pair_major")

    def set_sim3_fix_scale(self, on: bool = True):
        """VertexSim3Expmap::_fix_scale for every V_SIM3 vertex: oplus zeroes update[6] and EdgeSim3's Jacobians lose
        column 6, as the reference's numeric ones do. H(6, 6) then holds lambda alone: gn_* and dl_* on such a graph
        are not positive definite."""
        _check(lib().g2ohip_set_sim3_fix_scale(self.h, int(bool(on))), "set_sim3_fix_scale")

    def set_sim3_cameras(self, ids, cam1=None, cam2=None):
        """VertexSim3Expmap's two pinhole cameras for the V_SIM3 vertices ``ids``: cam1 / cam2 [n, 4] fx fy cx cy (one
        row is taken for every id), None leaves that camera as it is. E_SIM3_PROJECT reads camera 1 of its Sim3 vertex,
        E_SIM3_PROJECT_INVERSE camera 2; both default to 1 1 0 0 and camera 1 is what a VERTEX_SIM3:EXPMAP line holds."""
        ids = np.ascontiguousarray(np.atleast_1d(ids), np.int32)

        def rows(c):
            if c is None:
                return None
            c = np.asarray(c, np.float64)
            return np.ascontiguousarray(np.broadcast_to(c, (len(ids), 4)) if c.ndim == 1 else c.reshape(len(ids), 4))

        c1, c2 = rows(cam1), rows(cam2)
        _check(lib().g2ohip_set_sim3_cameras(self.h, len(ids), _p(ids), _p(c1), _p(c2)), "set_sim3_cameras")

    def pair_major_info(self) -> dict:
        """After a structure build: whether it is pair-major, and its pairs and chunks."""
        out = np.zeros(3, np.int32)
        _check(lib().g2ohip_pair_major_info(self.h, _p(out)), "pair_major_info")
        return dict(pair_major=bool(out[0]), pairs=int(out[1]), chunks=int(out[2]))

    def set_dogleg_params(self, initial_delta: float = 0.0, max_trials: int = 0, initial_lambda: float = 0.0,
                          lambda_factor: float = 0.0):
        """OptimizationAlgorithmDogleg's properties for the dl_hip_* algorithms (initialDelta 1e4,
        maxTrialsAfterFailure 100, initialLambda 1e-7, lambdaFactor 10); a value <= 0 selects the default."""
        _check(lib().g2ohip_set_dogleg_params(self.h, float(initial_delta), int(max_trials), float(initial_lambda),
                                              float(lambda_factor)), "set_dogleg_params")

    DOGLEG_STEPS = ("Undefined", "Descent", "GN", "Dogleg")  # stepType2Str, by the reference's enum order

    def dogleg_state(self) -> dict:
        """After the last dl_hip_* iteration: trustRegion(), lastStep (1 SD, 2 GN, 3 DL, 0 undefined), lastNumTries,
        the damping of the not-PD branch and wasPDInAllIterations."""
        out = np.zeros(5)
        _check(lib().g2ohip_dogleg_state(self.h, _p(out), 5), "dogleg_state")
        return dict(delta=float(out[0]), step=int(out[1]), tries=int(out[2]), lam=float(out[3]), was_pd=bool(out[4]))

    STRUCTURE_ONLY_COUNTS = ("accepted", "rejected", "gradient_stops", "exhausted", "fixed_skipped")

    def structure_only(self, ids=None, iterations: int = 1, max_trials: int = 10) -> dict:
        """StructureOnlySolver::calc(points, iterations, max_trials) (structure_only_solver.h:72-212) on the device:
        every marginalised landmark (``ids`` None) or the given landmark ids refined with all other vertices held
        fixed, in one kernel launch. ba_demo's sequence is ``structure_only(iterations=10)`` and then
        ``set_algorithm("lm_hip_fix6_3")`` and ``optimize`` on the same handle. Returns the five counts."""
        counts = np.zeros(5, dtype=np.int64)
        if ids is None:
            n, idp = 0, None
        else:
            ida = np.ascontiguousarray(ids, dtype=np.int32)
            n, idp = int(ida.size), _p(ida)
        args = (self.h, n, idp, int(iterations), int(max_trials), _p(counts))
        r = lib().g2ohip_structure_only_calc(*args)
        if r == -2:  # G2OHIP_ERR_STATE: initializeOptimization first, as optimize() does by itself
            self.initialize_optimization()
            r = lib().g2ohip_structure_only_calc(*args)
        _check(r, "structure_only")
        return dict(zip(self.STRUCTURE_ONLY_COUNTS, (int(c) for c in counts)))

    def initialize_optimization(self, level: int = 0):
        """SparseOptimizer::initializeOptimization(level): the edges on ``level`` (every edge when it is negative) and
        the vertices they touch form the system; the handle remembers the level."""
        _check(lib().g2ohip_initialize_level(self.h, int(level)), "initializeOptimization")

    # ---- edge levels, per-edge chi2, outlier classification ----
    LEVEL_KEEP = LEVEL_KEEP

    def set_edge_levels(self, etype: int, levels, idx=None):
        """Edge::setLevel for the edges of a type (insertion order): ``levels[k]`` for edge ``idx[k]``, or for edge k
        when ``idx`` is None (then one level per edge of the type). Takes effect at the next
        initialize_optimization."""
        lv = np.ascontiguousarray(levels, np.int32)
        ix = None if idx is None else np.ascontiguousarray(idx, np.int32)
        if ix is not None and ix.size != lv.size:
            raise ValueError(f"set_edge_levels: {ix.size} indices for {lv.size} levels")
        _check(lib().g2ohip_set_edge_levels(self.h, etype, int(lv.size), _p(ix), _p(lv)), "set_edge_levels")

    def edge_levels(self, etype: int) -> np.ndarray:
        """Edge::level() of every edge of a type, in insertion order."""
        n = _check(lib().g2ohip_get_edge_levels(self.h, etype, None, 0), "edge_levels")
        out = np.zeros(n, np.int32)
        _check(lib().g2ohip_get_edge_levels(self.h, etype, _p(out), n), "edge_levels")
        return out

    def edge_chi2(self, etype: int, depth: bool = False):
        """Edge::chi2() (e^T Omega e, not robustified) of every edge of a type, active or not, at the device's
        estimates; with ``depth`` also isDepthPositive() as a bool array: (chi2, depth_positive)."""
        n = _check(lib().g2ohip_get_edge_levels(self.h, etype, None, 0), "edge_chi2")
        chi = np.zeros(max(n, 1))
        dp = np.zeros(max(n, 1), np.uint8) if depth else None
        _check(lib().g2ohip_edge_chi2(self.h, etype, _p(chi), _p(dp)), "edge_chi2")
        return (chi[:n], dp[:n].astype(bool)) if depth else chi[:n]

    def classify_edges(self, etype: int, chi2_max: float, check_depth: bool = False, inlier_level: int = 0,
                       outlier_level: int = 1) -> dict:
        """One device pass over every edge of a type: bad = chi2 > chi2_max or (check_depth and not z > 0); the edge
        moves to ``outlier_level`` when bad, else to ``inlier_level`` (LEVEL_KEEP: stays where it is). Returns the
        counts ``over_chi2``, ``depth_failed`` and ``bad``."""
        counts = np.zeros(3, np.int64)
        _check(lib().g2ohip_classify_edges(self.h, etype, float(chi2_max), int(check_depth), int(inlier_level),
                                           int(outlier_level), _p(counts)), "classify_edges")
        return dict(over_chi2=int(counts[0]), depth_failed=int(counts[1]), bad=int(counts[2]))

    def update_initialization(self):
        """SparseOptimizer::updateInitialization (online mode, non-Schur): vertices / edges added since
        initialize_optimization join with appended hessian indices; optimize() then continues from the current state."""
        _check(lib().g2ohip_update_initialization(self.h), "updateInitialization")

    def chi2(self) -> float:
        return lib().g2ohip_chi2(self.h)

    def optimize(self, iterations: int, max_trials: int = 10, lambda_init: float = 0.0, verbose: bool = False):
        cfg = Config(max_trials, lambda_init, int(verbose))
        stats = (BatchStats * max(iterations, 1))()
        n = _check(lib().g2ohip_optimize(self.h, C.byref(cfg), iterations, stats), "optimize")
        return n, [stats[i] for i in range(n)]

    def optimize_step(self, iteration: int, max_trials: int = 10, lambda_init: float = 0.0, stats: bool = True):
        cfg = Config(max_trials, lambda_init, 0)
        st = BatchStats()
        r = _check(lib().g2ohip_optimize_step(self.h, C.byref(cfg), iteration, C.byref(st) if stats else None),
                   "optimize_step")
        return r, st

    def minimal_state(self) -> np.ndarray:
        n = _check(lib().g2ohip_minimal_state(self.h, None), "minimal_state")
        out = np.zeros(n)
        lib().g2ohip_minimal_state(self.h, _p(out))
        return out

    def estimates(self, vtype: int) -> np.ndarray:
        n = _check(lib().g2ohip_get_estimates(self.h, vtype, None, None), "get_estimates")
        out = np.zeros((n, synth.EST_DIM[vtype]))
        lib().g2ohip_get_estimates(self.h, vtype, _p(out), None)
        return out

    # ---- Solver plugin (core/solver.h) ----
    def build_structure(self):
        _check(lib().g2ohip_solver_build_structure(self.h), "buildStructure")

    def build_system(self):
        _check(lib().g2ohip_solver_build_system(self.h), "buildSystem")

    def set_lambda(self, lam: float, backup: bool = True):
        _check(lib().g2ohip_solver_set_lambda(self.h, lam, int(backup)), "setLambda")

    def restore_diagonal(self):
        _check(lib().g2ohip_solver_restore_diagonal(self.h), "restoreDiagonal")

    def solve(self) -> bool:
        return bool(_check(lib().g2ohip_solver_solve(self.h), "solve"))

    def vector_size(self) -> int:
        return int(lib().g2ohip_solver_vector_size(self.h))

    def block_dims(self):
        """[PoseDim, LandmarkDim, pose blocks, landmark blocks] of the built structure."""
        d = np.zeros(4, np.int32)
        _check(lib().g2ohip_solver_block_dims(self.h, _p(d)), "block_dims")
        return [int(v) for v in d]

    def x(self) -> np.ndarray:
        out = np.zeros(self.vector_size())
        _check(lib().g2ohip_solver_get_x(self.h, _p(out)), "x")
        return out

    def b(self) -> np.ndarray:
        out = np.zeros(self.vector_size())
        _check(lib().g2ohip_solver_get_b(self.h, _p(out)), "b")
        return out

    def update(self, x=None):
        """SparseOptimizer::update (sparse_optimizer.cpp:441-454): oplus of every free vertex with its part of x, a
        host vector in the Hessian order (see x()); None applies the solver's own x."""
        if x is not None:
            x = np.ascontiguousarray(x, np.float64)
            if x.size != self.vector_size():
                raise ValueError(f"update: x has {x.size} entries, the solver's vector has {self.vector_size()}")
        _check(lib().g2ohip_update(self.h, _p(x)), "update")

    def push(self):
        """SparseOptimizer::push: every vertex's estimate onto its stack."""
        _check(lib().g2ohip_push(self.h), "push")

    def pop(self):
        """SparseOptimizer::pop: the estimates as the matching push() saved them."""
        _check(lib().g2ohip_pop(self.h), "pop")

    def multiply_hessian(self, src) -> np.ndarray:
        """BlockSolverBase::multiplyHessian (block_solver.h:146): Hpp @ src (pose part)."""
        src = np.ascontiguousarray(src, np.float64)
        out = np.zeros_like(src)
        _check(lib().g2ohip_solver_multiply_hessian(self.h, _p(out), _p(src)), "multiplyHessian")
        return out

    def set_eta(self, eta: float):
        """Solver::setEta: forcing term of the lm_pcg6_3_eigen CGLS (default 0.1)."""
        _check(lib().g2ohip_solver_set_eta(self.h, float(eta)), "set_eta")

    def linear_iterations(self) -> int:
        """Iterations of the last iterative linear solve (the CGLS under lm_pcg6_3_eigen, else the block-Jacobi PCG)."""
        return int(lib().g2ohip_solver_linear_iterations(self.h))

    def diag_absmax(self) -> float:
        """max |diag| of the vertex Hessians (computeLambdaInit's input) after buildSystem."""
        r = np.zeros(1)
        _check(lib().g2ohip_solver_diag_absmax(self.h, _p(r)), "diag_absmax")
        return float(r[0])

    def linear_residual(self) -> float:
        """||(A + lambda I) x - b|| / ||b|| of the last solve, computed on the device."""
        r = np.zeros(1)
        _check(lib().g2ohip_solver_linear_residual(self.h, _p(r)), "linear_residual")
        return float(r[0])

    def compute_marginals(self, block_indices):
        """SparseOptimizer::computeMarginals(spinv, blockIndices) (sparse_optimizer.h:129): {(r, c): pd x pd block
        of Hpp^-1} for the Hessian block index pairs, or None when the factorization fails (the reference's false)."""
        pairs = [(int(r), int(c)) for r, c in block_indices]
        rows = np.ascontiguousarray([p[0] for p in pairs] or [0], np.int32)
        cols = np.ascontiguousarray([p[1] for p in pairs] or [0], np.int32)
        pd = self.block_dims()[0]
        out = np.zeros(max(len(pairs), 1) * pd * pd)
        rc = lib().g2ohip_solver_compute_marginals(self.h, len(pairs), _p(rows), _p(cols), _p(out))
        _check(min(rc, 0), "computeMarginals")
        if rc == 0:
            return None
        return {p: out[k * pd * pd:(k + 1) * pd * pd].reshape(pd, pd).T.copy() for k, p in enumerate(pairs)}

    FACTOR_INFO_KEYS = ("n", "nnzL", "flops", "supernodes", "levels", "max_front", "blocked_fronts",
                        "inplace_levels", "prescatter_levels", "syrk_launches", "bwd_rounds", None,
                        "owned_fronts", "shared_fronts", "subtree_roots", "root_exchange_doubles",
                        "model_rank_subtrees_s", "model_shared_s", "model_single_gpu_s", "model_exchange_s",
                        "distributed", "reduce_scatter", "rs_segment_doubles", "rs_tail_doubles", "model_input_s",
                        "model_input_allreduce_s", None,  # None: retired slots (always 0), kept for the ABI layout
                        "band_leaf", "aligned_shards", "local_block_doubles", "exchange_bytes_per_rank",
                        "local_landmarks", "model_shard_s", "deferred_l21_fronts",
                        # the Schur row pass on this rank: tasks and split row chunks of the G-block / Kt-record sets,
                        # partial blocks staged by the parts; camera_list 0: all cameras, no list
                        "schur_tasks", "schur_tasks_kx", "schur_part_groups", "schur_part_groups_kx",
                        "schur_part_blocks", "camera_list")

    def factor_info(self) -> dict:
        out = np.zeros(len(self.FACTOR_INFO_KEYS))
        _check(lib().g2ohip_solver_factor_info(self.h, _p(out), len(out)), "factor_info")
        return {k: v for k, v in zip(self.FACTOR_INFO_KEYS, out.tolist()) if k is not None}

    def local_landmark_ids(self) -> np.ndarray:
        """Ids of the free landmarks this rank's shard holds (landmark sharding; all of them on one rank)."""
        n = _check(lib().g2ohip_local_landmarks(self.h, None, 0), "local_landmarks")
        ids = np.zeros(max(n, 1), np.int32)
        lib().g2ohip_local_landmarks(self.h, _p(ids), n)
        return ids[:n]

    def stage(self, lam: float):
        dims = np.zeros(3, np.int64)
        _check(lib().g2ohip_stage(self.h, 0.0, None, None, None, None, _p(dims)), "stage")
        n, npose = int(dims[0]), int(dims[1])
        b, x, H, bs = np.zeros(n), np.zeros(n), np.zeros((npose, npose)), np.zeros(npose)
        ok = _check(lib().g2ohip_stage(self.h, lam, _p(b), _p(x), _p(H), _p(bs), _p(dims)), "stage")
        return dict(ok=ok, b=b, x=x, Hschur=H, bschur=bs, n=n, np=npose, nl=int(dims[2]))

    # ---- multi-GPU ----
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = (C.c_ubyte * 128)()
        _check(lib().g2ohip_comm_unique_id(buf), "comm_unique_id")
        return bytes(buf)

    @staticmethod
    def comm_selftest(values, device: int = 0):
        """RCCL binding smoke test on one device (one-rank communicator): allreduce sum, allreduce max and the
        in-place reduce-scatter sum (rank 0's segment), each over `values`."""
        v = np.ascontiguousarray(values, np.float64)
        out = np.zeros(2 * v.size)
        rs = np.zeros(v.size)
        uid = (C.c_ubyte * 128).from_buffer_copy(SparseOptimizer.comm_unique_id())
        _check(lib().g2ohip_comm_selftest_rs(device, uid, v.size, _p(v), _p(out), _p(rs)), "comm_selftest")
        return out[: v.size], out[v.size:], rs

    def set_comm(self, uid: bytes, rank: int, nranks: int):
        buf = (C.c_ubyte * 128).from_buffer_copy(uid)
        _check(lib().g2ohip_set_comm(self.h, buf, rank, nranks), "set_comm")

    def set_comm_local(self, group_key: str, rank: int, nranks: int):
        """In-process test transport (see g2ohip_set_comm_local); one host thread per rank."""
        _check(lib().g2ohip_set_comm_local(self.h, group_key.encode(), rank, nranks), "set_comm_local")

    # ---- measurement ----
    def enable_kernel_timing(self, on: bool = True, only: str | None = None):
        """Per-kernel-class HIP-event timing; ``only`` restricts it to one class."""
        lib().g2ohip_kernel_timing_only(self.h, (only or "").encode())
        lib().g2ohip_enable_kernel_timing(self.h, int(on))

    def set_stats_level(self, level: int):
        """G2OBatchStatistics timers: 0 none, 1 timeLinearSolution only, 2 every stage (default)."""
        lib().g2ohip_set_stats_level(self.h, int(level))

    def kernel_ms(self, name: str) -> float:
        return lib().g2ohip_kernel_ms(self.h, name.encode())

    def kernel_count(self, name: str) -> int:
        return lib().g2ohip_kernel_count(self.h, name.encode())

    def kernel_bytes(self, name: str) -> float:
        return lib().g2ohip_kernel_bytes(self.h, name.encode())

    def kernel_flops(self, name: str) -> float:
        return lib().g2ohip_kernel_flops(self.h, name.encode())
