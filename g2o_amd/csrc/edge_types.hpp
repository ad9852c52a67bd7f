// What the host knows about each device edge type, in one table: EDGE_TYPES has one row per G2OHIP_E_* code the
// device linearizes itself (1-3, 5-30). The host-Jacobian types (G2OHIP_E_HOSTJ*, any D and any endpoints) are no rows:
// their facts follow from the code (hostj_dim). The launchers check the rows against the device families at compile
// time (family_dispatch.hpp), so a stride here cannot drift from the one a kernel indexes with.
#pragma once
#include "../../include/g2o_hip.h"

namespace g2ohip {

enum Family {
  FAM_NONE = 0, FAM_BA = 1, FAM_SE3 = 2, FAM_SE2 = 3, FAM_HOSTJ = 4, FAM_SE2XY = 5, FAM_BA_STEREO = 6,
  // slam3d landmark edges (VertexSE3 pose, point): EdgeSE3PointXYZ, ...Depth, ...Disparity
  FAM_SE3_XYZ = 7, FAM_SE3_XYZ_DEPTH = 8, FAM_SE3_XYZ_DISPARITY = 9,
  // EdgeSE3Expmap between two VertexSE3Expmap cameras
  FAM_EXPMAP = 10,
  // sba types (point, VertexCam): EdgeProjectP2MC, EdgeProjectP2SC
  FAM_SBA_MONO = 11, FAM_SBA_STEREO = 12,
  // offset and bearing edges: EdgeSE3Offset, EdgeSE2Offset (two poses, two sensor offsets), EdgeSE2PointXYBearing
  FAM_SE3_OFFSET = 13, FAM_SE2_OFFSET = 14, FAM_SE2XY_BEARING = 15,
  // unary families (BaseUnaryEdge: one vertex, EdgeArgs::v1 / s1 null, DB = 0)
  FAM_U_SE2 = 16, FAM_U_SE2XY = 17, FAM_U_XY = 18, FAM_U_SE3 = 19, FAM_U_XYZ = 20, FAM_U_HOSTJ = 21,
  // pose-only projections on a VertexSE3Expmap camera: EdgeSE3ProjectXYZOnlyPose, EdgeStereoSE3ProjectXYZOnlyPose
  FAM_U_POSE_ONLY = 22, FAM_U_STEREO_POSE_ONLY = 23,
  // EdgeProjectXYZ2UVU (point, VertexSE3Expmap camera, a CameraParameters record): FamilyUVU. A binary family, as
  // FAM_BA_STEREO; EdgeProjectXYZ2UV runs as FAM_BA with the record f f cx cy
  FAM_BA_UVU = 24,
  // Edge_V_V_GICP between two VertexSE3 (types_icp): FamilyGICP, point-to-plane or plane-to-plane per edge set
  FAM_GICP = 25,
  // Edge_XYZ_VSC (point, VertexSCam = a VertexSE3 camera): FamilyVSC, the landmark first as in the BA families
  FAM_VSC = 26,
  // EdgeSim3 between two VertexSim3Expmap (types/sim3): FamilySim3, linearized by k_linearize_sim3
  FAM_SIM3 = 27,
  // EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ (point, VertexSim3Expmap): FamilySim3Project<false> / <true>,
  // linearized by k_linearize_sim3_project (the Sim3 side alone: the point is fixed in every graph that initialises)
  FAM_SIM3_PROJECT = 28, FAM_SIM3_PROJECT_INVERSE = 29,
  // EdgeObservationBAL (VertexCameraBAL, point; examples/bal): FamilyBAL, a 2 x 9 camera Jacobian
  FAM_BAL = 30,
  FAM_COUNT
};

constexpr int vertex_dim(int t) {
  if (t == G2OHIP_V_SIM3) return 7;
  if (t == G2OHIP_V_CAM_BAL) return 9;
  return t == G2OHIP_V_SE3_EXPMAP || t == G2OHIP_V_SE3_QUAT || t == G2OHIP_V_CAM ? 6
         : (t == G2OHIP_V_XYZ || t == G2OHIP_V_SE2 ? 3 : (t == G2OHIP_V_XY ? 2 : -1));
}

// which endpoint a marginalised landmark may be (the Schur path's landmark edges; structure-only reads it for the
// families has_structure_only_form names)
enum LmSide { LM_NONE, LM_V0, LM_V1 };

// lm_pcg6_3_eigen (matrix-free CGLS on the Jacobian of BA edges) refuses a graph that holds one of these; in the order
// the structure build checks them: what the message calls the edges, and what to use instead. 0: not refused
struct CglsRefusal { const char* what; const char* instead; };
inline constexpr CglsRefusal CGLS_REFUSALS[] = {
    {nullptr, nullptr},
    {"the slam3d landmark edges", "lm_pcg6_3 or lm_hip_fix6_3"},
    {"the sba types on a VertexCam", "lm_pcg6_3 or lm_hip_fix6_3"},
    {"the offset and bearing edges", "lm_pcg or lm_hip_var"},
    {"the types_icp edges Edge_V_V_GICP / Edge_XYZ_VSC", "lm_pcg, lm_pcg6_3 or lm_hip_var"},
    {"the CameraParameters edges EdgeProjectXYZ2UV / XYZ2UVU", "lm_pcg6_3 or lm_hip_fix6_3"},
    {"EdgeSE3Expmap", "lm_pcg6_3 or lm_hip_fix6_3"},
};
enum { CGLS_OK, CGLS_SLAM3D, CGLS_SBA, CGLS_OFFSET, CGLS_ICP, CGLS_CAMPARAMS, CGLS_EXPMAP };

struct EdgeTypeInfo {
  int type;       // G2OHIP_E_*
  Family family;  // the device family that linearizes it
  int vtA, vtB;   // G2OHIP_V_* of v0 and v1; vtB = 0: a unary type
  int D;          // error dimension
  // doubles per edge as the caller gives them (g2ohip_add_edges) and as the family's kernels stride the uploaded
  // buffers (F::MEAS, F::PAR); Engine::fill_group_device converts one into the other. GICP: the parameter buffer exists
  // only when the set has covariances (plane-to-plane)
  int nm, np, dev_meas, dev_par;
  LmSide lm;
  bool uniform;  // edges whose information / parameter records are all equal share one record on the device
  bool depth;    // the reference type has isDepthPositive()
  // the .g2o line: TAG v0 [v1] [pid [pid2]] meas[nm] and, with info_upper, the upper triangle of the information
  // row-wise (else the line carries none). tag = nullptr: no file carries the type. load_flag: the G2OHIP_LOAD_* bit
  // that makes the loader read the tag, 0: always read. npid: parameter ids on the line
  const char* tag;
  unsigned load_flag;
  int npid;
  bool info_upper;
  int cgls;  // index into CGLS_REFUSALS
};

namespace edge_types_detail {
constexpr int EXPMAP = G2OHIP_V_SE3_EXPMAP, XYZ = G2OHIP_V_XYZ, SE3 = G2OHIP_V_SE3_QUAT, SE2 = G2OHIP_V_SE2,
              XY = G2OHIP_V_XY, CAM = G2OHIP_V_CAM, SIM3 = G2OHIP_V_SIM3, CAM_BAL = G2OHIP_V_CAM_BAL;
constexpr bool Y = true, N = false;
constexpr const char* NOTAG = nullptr;
// per row:  type, family, vtA, vtB,                      D, nm, np, dev_meas, dev_par,
//           landmark, uniform, depth,                    tag, load flag, pids, info on the line,  CGLS refusal
// sorted by type code (edge_type_info relies on it; asserted below)
constexpr EdgeTypeInfo TABLE[] = {
    {G2OHIP_E_SE3_PROJECT_XYZ, FAM_BA, XYZ, EXPMAP,       2, 2, 4, 2, 4,
     LM_V0, Y, Y,    "EDGE_SE3_PROJECT_XYZ:EXPMAP", 0, 0, Y,  CGLS_OK},  // (the line: + fx fy cx cy behind the information)
    {G2OHIP_E_SE3_QUAT, FAM_SE3, SE3, SE3,                6, 7, 0, 12, 0,  // device: Z^-1 as an isometry [R | t]
     LM_NONE, N, N,  "EDGE_SE3:QUAT", 0, 0, Y,  CGLS_OK},
    {G2OHIP_E_SE2, FAM_SE2, SE2, SE2,                     3, 3, 0, 3, 0,
     LM_NONE, N, N,  "EDGE_SE2", 0, 0, Y,  CGLS_OK},
    {G2OHIP_E_SE2_XY, FAM_SE2XY, SE2, XY,                 2, 2, 0, 2, 0,
     LM_V1, N, N,    "EDGE_SE2_XY", 0, 0, Y,  CGLS_OK},
    {G2OHIP_E_STEREO_SE3_PROJECT_XYZ, FAM_BA_STEREO, XYZ, EXPMAP,  3, 3, 5, 3, 5,
     LM_V0, Y, Y,    NOTAG, 0, 0, N,  CGLS_OK},
    // slam3d: the offset x y z q (7) [+ fx fy cx cy] -> its inverse as an isometry (12) [+ fx fy cx cy]
    {G2OHIP_E_SE3_XYZ, FAM_SE3_XYZ, SE3, XYZ,             3, 3, 7, 3, 12,
     LM_V1, Y, N,    "EDGE_SE3_TRACKXYZ", G2OHIP_LOAD_SLAM3D, 1, Y,  CGLS_SLAM3D},
    {G2OHIP_E_SE3_XYZ_DEPTH, FAM_SE3_XYZ_DEPTH, SE3, XYZ, 3, 3, 11, 3, 16,
     LM_V1, Y, N,    "EDGE_PROJECT_DEPTH", G2OHIP_LOAD_SLAM3D, 1, Y,  CGLS_SLAM3D},
    {G2OHIP_E_SE3_XYZ_DISPARITY, FAM_SE3_XYZ_DISPARITY, SE3, XYZ,  3, 3, 11, 3, 16,
     LM_V1, Y, N,    "EDGE_PROJECT_DISPARITY", G2OHIP_LOAD_SLAM3D, 1, Y,  CGLS_SLAM3D},
    {G2OHIP_E_SE3_EXPMAP, FAM_EXPMAP, EXPMAP, EXPMAP,     6, 7, 0, 8, 0,  // device: the SE3Quat padded to 64 bytes
     LM_NONE, N, N,  "EDGE_SE3:EXPMAP", G2OHIP_LOAD_EXPMAP, 0, Y,  CGLS_EXPMAP},  // (the line: the inverse measurement)
    {G2OHIP_E_PROJECT_P2MC, FAM_SBA_MONO, XYZ, CAM,       2, 2, 0, 2, 0,
     LM_V0, Y, N,    "EDGE_PROJECT_P2MC", G2OHIP_LOAD_SBA, 0, N,  CGLS_SBA},
    {G2OHIP_E_PROJECT_P2SC, FAM_SBA_STEREO, XYZ, CAM,     3, 3, 0, 3, 0,
     LM_V0, Y, N,    "EDGE_PROJECT_P2SC", G2OHIP_LOAD_SBA, 0, N,  CGLS_SBA},
    {G2OHIP_E_SE3_OFFSET, FAM_SE3_OFFSET, SE3, SE3,       6, 7, 14, 12, 24,  // two offsets x y z q -> two isometries
     LM_NONE, Y, N,  "EDGE_SE3_OFFSET", G2OHIP_LOAD_OFFSET, 2, Y,  CGLS_OFFSET},
    {G2OHIP_E_SE2_OFFSET, FAM_SE2_OFFSET, SE2, SE2,       3, 3, 6, 3, 6,
     LM_NONE, Y, N,  "EDGE_SE2_OFFSET", G2OHIP_LOAD_OFFSET, 2, Y,  CGLS_OFFSET},
    {G2OHIP_E_SE2_XY_BEARING, FAM_SE2XY_BEARING, SE2, XY, 1, 1, 0, 1, 0,
     LM_V1, Y, N,    "EDGE_BEARING_SE2_XY", G2OHIP_LOAD_OFFSET, 0, Y,  CGLS_OFFSET},
    // unary types (has_unary_ refuses them under CGLS as a whole)
    {G2OHIP_E_SE2_PRIOR, FAM_U_SE2, SE2, 0,               3, 3, 0, 3, 0,
     LM_NONE, N, N,  "EDGE_PRIOR_SE2", G2OHIP_LOAD_UNARY, 0, Y,  CGLS_OK},
    {G2OHIP_E_SE2_XY_PRIOR, FAM_U_SE2XY, SE2, 0,          2, 2, 0, 2, 0,
     LM_NONE, N, N,  "EDGE_PRIOR_SE2_XY", G2OHIP_LOAD_UNARY, 0, Y,  CGLS_OK},
    {G2OHIP_E_XY_PRIOR, FAM_U_XY, XY, 0,                  2, 2, 0, 2, 0,
     LM_V0, N, N,    "EDGE_PRIOR_XY", G2OHIP_LOAD_UNARY, 0, Y,  CGLS_OK},
    {G2OHIP_E_SE3_PRIOR, FAM_U_SE3, SE3, 0,               6, 7, 7, 24, 0,  // device: Z^-1 and the offset, two isometries
     LM_NONE, N, N,  "EDGE_SE3_PRIOR", G2OHIP_LOAD_UNARY, 1, Y,  CGLS_OK},
    {G2OHIP_E_XYZ_PRIOR, FAM_U_XYZ, XYZ, 0,               3, 3, 0, 3, 0,
     LM_V0, N, N,    "EDGE_POINTXYZ_PRIOR", G2OHIP_LOAD_UNARY, 0, Y,  CGLS_OK},
    // pose-only projections: the caller's record Xw fx fy cx cy [bf]; Xw moves behind the observation on the device
    {G2OHIP_E_SE3_PROJECT_XYZ_ONLYPOSE, FAM_U_POSE_ONLY, EXPMAP, 0,  2, 2, 7, 5, 4,
     LM_NONE, Y, Y,  NOTAG, 0, 0, N,  CGLS_OK},
    {G2OHIP_E_STEREO_SE3_PROJECT_XYZ_ONLYPOSE, FAM_U_STEREO_POSE_ONLY, EXPMAP, 0,  3, 3, 8, 6, 5,
     LM_NONE, Y, Y,  NOTAG, 0, 0, N,  CGLS_OK},
    // CameraParameters edges: f cx cy baseline -> f f cx cy (FamilyBA; no isDepthPositive in the reference) / f f cx cy b
    {G2OHIP_E_PROJECT_XYZ2UV, FAM_BA, XYZ, EXPMAP,        2, 2, 4, 2, 4,
     LM_V0, Y, N,    "EDGE_PROJECT_XYZ2UV:EXPMAP", G2OHIP_LOAD_CAMERAPARAMS, 1, Y,  CGLS_CAMPARAMS},
    {G2OHIP_E_PROJECT_XYZ2UVU, FAM_BA_UVU, XYZ, EXPMAP,   3, 3, 4, 3, 5,
     LM_V0, Y, N,    NOTAG, 0, 0, N,  CGLS_CAMPARAMS},
    // Edge_V_V_GICP: pos0 normal0 pos1 normal1 -> pos0 pos1; the covariances cov0 | cov1 as given
    {G2OHIP_E_V_V_GICP, FAM_GICP, SE3, SE3,               3, 12, 12, 6, 12,
     LM_NONE, Y, N,  "EDGE_V_V_GICP", G2OHIP_LOAD_ICP, 0, N,  CGLS_ICP},
    {G2OHIP_E_XYZ_VSC, FAM_VSC, XYZ, SE3,                 3, 3, 5, 3, 5,
     LM_V0, Y, N,    NOTAG, 0, 0, N,  CGLS_ICP},
    {G2OHIP_E_SIM3, FAM_SIM3, SIM3, SIM3,                 7, 8, 0, 8, 0,  // a Sim3: tx ty tz qx qy qz qw s
     LM_NONE, Y, N,  "EDGE_SIM3:EXPMAP", G2OHIP_LOAD_SIM3, 0, Y,  CGLS_OK},  // (the line: log of the inverse, 7 values)
    // the Sim3 projections: no caller record; the device record is camera 1 (inverse: camera 2) of the edge's Sim3 vertex
    // (CGLS: blocks of 7 are refused before the per-type check)
    {G2OHIP_E_SIM3_PROJECT_XYZ, FAM_SIM3_PROJECT, XYZ, SIM3,  2, 2, 0, 2, 4,
     LM_NONE, Y, N,  "EDGE_PROJECT_SIM3_XYZ:EXPMAP", G2OHIP_LOAD_SIM3_PROJECT, 0, Y,  CGLS_OK},
    {G2OHIP_E_SIM3_PROJECT_INVERSE_XYZ, FAM_SIM3_PROJECT_INVERSE, XYZ, SIM3,  2, 2, 0, 2, 4,
     LM_NONE, Y, N,  "EDGE_PROJECT_INVERSE_SIM3_XYZ:EXPMAP", G2OHIP_LOAD_SIM3_PROJECT, 0, Y,  CGLS_OK},
    // EdgeObservationBAL: the camera first (CGLS: blocks of 9 are refused before the per-type check)
    {G2OHIP_E_OBSERVATION_BAL, FAM_BAL, CAM_BAL, XYZ,     2, 2, 0, 2, 0,
     LM_V1, Y, N,    NOTAG, 0, 0, N,  CGLS_OK},
};
constexpr bool sorted_and_complete() {
  bool seen[FAM_COUNT] = {};
  int prev = 0;
  for (const EdgeTypeInfo& t : TABLE) {
    if (t.type <= prev) return false;
    prev = t.type;
    seen[t.family] = true;
  }
  for (int f = FAM_NONE + 1; f < FAM_COUNT; ++f)
    if (!seen[f] && f != FAM_HOSTJ && f != FAM_U_HOSTJ) return false;
  return true;
}
static_assert(sorted_and_complete(), "EDGE_TYPES: rows sorted by type code, none twice, every device family present");
}  // namespace edge_types_detail
inline constexpr auto& EDGE_TYPES = edge_types_detail::TABLE;

// the row of a device edge type; nullptr: a host-Jacobian type or an unknown code
constexpr const EdgeTypeInfo* edge_type_info(int type) {
  for (const EdgeTypeInfo& t : EDGE_TYPES)
    if (t.type == type) return &t;
  return nullptr;
}

// the families k_structure_only (structure_only.hip) has a point term for: a landmark edge of any other family on a
// marginalised vertex is refused by structure_only_* (EdgeObservationBAL: its point takes the Schur path only)
constexpr bool has_structure_only_form(int f) {
  return f == FAM_BA || f == FAM_BA_STEREO || f == FAM_BA_UVU || f == FAM_SE3_XYZ || f == FAM_SE3_XYZ_DEPTH ||
         f == FAM_SE3_XYZ_DISPARITY || f == FAM_SBA_MONO || f == FAM_SBA_STEREO || f == FAM_VSC || f == FAM_SE2XY ||
         f == FAM_SE2XY_BEARING || f == FAM_U_XYZ || f == FAM_U_XY;
}

// host-Jacobian types: the error dimension is the code's offset, the endpoints are any registered vertices
constexpr bool is_hostj_binary(int e) { return e > G2OHIP_E_HOSTJ(0) && e <= G2OHIP_E_HOSTJ(7); }
constexpr bool is_hostj_unary(int e) { return e > G2OHIP_E_HOSTJ_UNARY(0) && e <= G2OHIP_E_HOSTJ_UNARY(7); }
constexpr bool is_hostj(int e) { return is_hostj_binary(e) || is_hostj_unary(e); }
constexpr int hostj_dim(int e) { return is_hostj_binary(e) ? e - G2OHIP_E_HOSTJ(0) : e - G2OHIP_E_HOSTJ_UNARY(0); }
// the device family of any edge type code; FAM_NONE: unknown
constexpr int edge_family(int e) {
  const EdgeTypeInfo* t = edge_type_info(e);
  return t ? t->family : is_hostj_binary(e) ? FAM_HOSTJ : is_hostj_unary(e) ? FAM_U_HOSTJ : FAM_NONE;
}

// does a column of every row of a family (FAM_BA has two) hold what the family's kernels are compiled with?
constexpr int row_D(const EdgeTypeInfo& t) { return t.D; }
constexpr int row_dev_meas(const EdgeTypeInfo& t) { return t.dev_meas; }
constexpr int row_dev_par(const EdgeTypeInfo& t) { return t.dev_par; }
constexpr int row_DA(const EdgeTypeInfo& t) { return vertex_dim(t.vtA); }
constexpr int row_DB(const EdgeTypeInfo& t) { return t.vtB ? vertex_dim(t.vtB) : 0; }
constexpr bool family_rows_have(Family f, int (*col)(const EdgeTypeInfo&), int want) {
  bool any = false;
  for (const EdgeTypeInfo& t : EDGE_TYPES)
    if (t.family == f) {
      any = true;
      if (col(t) != want) return false;
    }
  return any;
}

}  // namespace g2ohip

