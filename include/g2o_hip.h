/*
 * g2o_hip.h — C ABI of the MI355X-native BlockSolver<p,l> backend (libg2o_hip.so).
 *
 * The drop-in boundary is g2o's own plugin interface for this path (paths
 * relative to the reference tree):
 *
 *   Solver (core/solver.h:44-155) ........ g2ohip_solver_*  (buildStructure /
 *        buildSystem / setLambda / restoreDiagonal / solve / x / b / vectorSize)
 *   LinearSolver<M>::solve (core/linear_solver.h:42-105) .. g2ohip_linear_solve_ccs
 *   OptimizationAlgorithmLevenberg::solve (core/optimization_algorithm_levenberg.cpp:58-150)
 *        + SparseOptimizer::optimize (core/sparse_optimizer.cpp:374-439) ... g2ohip_optimize
 *   OptimizableGraph::load / save (core/optimizable_graph.cpp:397-679) .. g2ohip_load_g2o / g2ohip_save_g2o
 *   OptimizationAlgorithmFactory::construct (core/optimization_algorithm_factory.cpp:84-93)
 *        .. g2ohip_set_algorithm("lm_hip_fix6_3" | "lm_hip_fix3_3" | "lm_hip_fix6_6" | "lm_hip_fix7_3" | "lm_hip_fix9_3" | "lm_hip_var" | "gn_hip_*"
 *           | "dl_hip_*" (Powell's dogleg, core/optimization_algorithm_dogleg.cpp:57-208; the same suffixes)
 *           | "structure_only_3" | "structure_only_2" (StructureOnlySolver<PointDoF>, solvers/structure_only/
 *             structure_only.cpp:64-65, structure_only_solver.h:60-229; g2ohip_structure_only_calc is its calc())
 *           | "{lm,gn}_pcg" | "{lm,gn}_pcg6_3" (block-Jacobi PCG, solver_pcg.cpp:91-98)
 *           | "lm_pcg6_3_eigen" (fork JacobiSolver_6_3 + LinearSolverPCGEigen CGLS, solver_eigen.cpp:80,126))
 *   G2OBatchStatistics (core/batch_stats.h:42-72) .. g2ohip_batch_stats
 *
 * Plain pointers and sizes only; no torch / HIP types cross the boundary.
 * Errors follow the reference: no exceptions, int status codes; a solve that
 * meets a non-positive-definite pivot returns 0 (the reference's `false`,
 * linear_solver_csparse.h:127-133) so the LM retry logic is unchanged.
 * Every compute entry point requires a MI355X (gfx950); there is no CPU path.
 */
#ifndef G2O_HIP_H
#define G2O_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- vertex types (estimate layouts) ---- */
#define G2OHIP_V_SE3_EXPMAP 1 /* VertexSE3Expmap, types_six_dof_expmap.h:84-102: tx ty tz qx qy qz qw (world->cam) */
#define G2OHIP_V_XYZ 2        /* VertexSBAPointXYZ, types_sba.h:137: x y z */
#define G2OHIP_V_SE3_QUAT 3   /* VertexSE3, vertex_se3.h:50: x y z qx qy qz qw (toVectorQT) */
#define G2OHIP_V_SE2 4        /* VertexSE2, vertex_se2.h:40: x y theta */
#define G2OHIP_V_XY 5         /* VertexPointXY, vertex_point_xy.h:39-88: x y (a BlockSolver_3_2 landmark) */
#define G2OHIP_V_CAM 6        /* VertexCam, types_sba.h:71-130: an SBACam (sbacam.h:55-175), dimension 6. The estimate is
                                 the VERTEX_CAM line, 12 doubles: x y z qx qy qz qw fx fy cx cy baseline, t the camera
                                 position in the world and q camera-to-world; g2ohip_add_vertices, g2ohip_get_estimates
                                 and g2ohip_set_estimates take and give 12 per vertex. On entry q is normalised to
                                 unit length with w >= 0 (VertexCam::read, SE3Quat(q, t)). g2ohip_minimal_state gives
                                 x y z qx qy qz (toMinimalVector, no sign change). oplus is SBACam::update: t += u[0:3],
                                 q = q * (u[3:6], sqrt(1 - |u[3:6]|^2)), normalised; no sign flip of w, no identity
                                 fallback: for |u[3:6]|^2 > 1 the square root and with it the rotation are NaN, as in
                                 the reference (the LM / GN / dogleg decisions reject the non-finite chi2) */
#define G2OHIP_V_SIM3 7       /* VertexSim3Expmap, types_seven_dof_expmap.h:61-105, dimension 7. The estimate is a Sim3,
                                 8 doubles: tx ty tz qx qy qz qw s (world->camera, as G2OHIP_V_SE3_EXPMAP; x -> s R x + t).
                                 On entry q is normalised to unit length with w >= 0 (Sim3::normalizeRotation); the device
                                 state is one 64-byte line per vertex. g2ohip_minimal_state gives Sim3::log() in the
                                 reference's order (omega, upsilon, sigma). oplus is Sim3(update) * estimate
                                 (sim3.h:66-135, 255-261) with all four branches of the exponential, and nothing is
                                 normalised afterwards: neither the 7-vector constructor nor operator* does in the
                                 reference. See g2ohip_set_sim3_fix_scale */
#define G2OHIP_V_CAM_BAL 8    /* VertexCameraBAL, examples/bal/bal_example.cpp:59-95, dimension 9. The estimate is 9
                                 doubles: rx ry rz tx ty tz f k1 k2, an angle-axis rotation (world to camera), the
                                 translation, the focal length and two radial distortion coefficients. Nothing is
                                 normalised on entry. oplus is estimate += update (:90-94); g2ohip_minimal_state gives
                                 the 9 values. VertexPointBAL is G2OHIP_V_XYZ as it stands (the same estimate and +=) */
/* ---- edge types ---- */
#define G2OHIP_E_SE3_PROJECT_XYZ 1 /* EdgeSE3ProjectXYZ, types_six_dof_expmap.h:201-229: v0 point, v1 camera;
                                      meas u v; info 2x2; params fx fy cx cy */
#define G2OHIP_E_SE3_QUAT 2        /* EdgeSE3, edge_se3.h: meas x y z qx qy qz qw; info 6x6 */
#define G2OHIP_E_SE2 3             /* EdgeSE2, edge_se2.h:46-52: meas x y theta; info 3x3 */
#define G2OHIP_E_SE2_XY 5          /* EdgeSE2PointXY, edge_se2_pointxy.h:41-75: v0 SE2 pose, v1 XY point; meas x y;
                                      info 2x2 */
#define G2OHIP_E_STEREO_SE3_PROJECT_XYZ 6 /* EdgeStereoSE3ProjectXYZ, types_six_dof_expmap.h:262-290: v0 point
                                      (G2OHIP_V_XYZ), v1 camera (G2OHIP_V_SE3_EXPMAP); meas u_l v u_r; info 3x3; params
                                      fx fy cx cy bf (n*5). As the reference's cam_project takes bf as a float
                                      (:287), the error uses bf rounded to float, the Jacobians the double. A graph
                                      whose only edge type this is takes the fused assembly, as a monocular one does;
                                      with other types beside it (monocular edges, say) the generic one. Not carried by
                                      .g2o files: see g2ohip_load_g2o / g2ohip_save_g2o */
/* slam3d landmark edges: v0 the pose (G2OHIP_V_SE3_QUAT), v1 the point (G2OHIP_V_XYZ), g2o's vertex order for these
 * edges (the opposite of the BA types); info 3x3. The sensor offset is ParameterSE3Offset::offset() as x y z qx qy qz qw;
 * the camera types take ParameterCamera: that offset, then fx fy cx cy. One record per edge; edges whose records are
 * all equal share a single one on the device. They are assembled on the generic slot path (BlockSolver_6_3 with the
 * points marginalized); lm_pcg6_3_eigen refuses them. */
#define G2OHIP_E_SE3_XYZ 7           /* EdgeSE3PointXYZ (EDGE_SE3_TRACKXYZ), edge_se3_pointxyz.cpp:100-135: meas x y z in
                                        the sensor frame; params offset (n*7), or NULL: every offset the identity */
#define G2OHIP_E_SE3_XYZ_DEPTH 8     /* EdgeSE3PointXYZDepth (EDGE_PROJECT_DEPTH), edge_se3_pointxyz_depth.cpp:91-138:
                                        meas u v depth; params offset + fx fy cx cy (n*11), NULL is G2OHIP_ERR_ARG */
#define G2OHIP_E_SE3_XYZ_DISPARITY 9 /* EdgeSE3PointXYZDisparity (EDGE_PROJECT_DISPARITY): meas u v 1/depth; params as
                                        G2OHIP_E_SE3_XYZ_DEPTH */
#define G2OHIP_E_SE3_EXPMAP 10 /* EdgeSE3Expmap (EDGE_SE3:EXPMAP), types_six_dof_expmap.h:104-127: the pose-pose
                                  constraint between two cameras, v0 = Ti and v1 = Tj both G2OHIP_V_SE3_EXPMAP; meas the
                                  SE3Quat C as tx ty tz qx qy qz qw (n*7), in the convention of the vertex estimate
                                  (the rotation is normalised to unit length, w >= 0); info 6x6 in (omega, upsilon)
                                  order, rotation first, as the vertex's oplus; params NULL. error =
                                  log(Tj^-1 * C * Ti); the Jacobians are the reference's adjoints (.cpp:278-293), exact
                                  at zero error only. Generic slot path; lm_pcg6_3_eigen refuses a graph that holds
                                  these edges (g2ohip_last_error says so) */
/* The sba types on a VertexCam (types_sba.h:173-250, what sba_demo builds): v0 the point (G2OHIP_V_XYZ), v1 the camera
 * (G2OHIP_V_CAM); params must be NULL (the intrinsics and the baseline live in the vertex; non-NULL is G2OHIP_ERR_ARG).
 * With pc = R^T (pw - t) the error is projected minus measured, the opposite sign of the expmap projections; the
 * Jacobians are the reference's analytic ones (types_sba.cpp:249-403), exact first derivatives under the vertex's
 * oplus. Robust kernels, edge levels, g2ohip_edge_chi2 and g2ohip_classify_edges take them like any device type; the
 * reference types have no isDepthPositive, so depth_positive != NULL or check_depth is G2OHIP_ERR_ARG. Generic slot
 * path with the 6/3 Schur kernels; lm_pcg6_3_eigen refuses a graph that holds them (g2ohip_last_error says so).
 * EdgeSBACam and EdgeSBAScale, which have no analytic Jacobian in the reference, enter as G2OHIP_E_HOSTJ(6) /
 * G2OHIP_E_HOSTJ(1) between G2OHIP_V_CAM vertices. */
#define G2OHIP_E_PROJECT_P2MC 11 /* EdgeProjectP2MC (EDGE_PROJECT_P2MC): meas u v; info 2x2;
                                    e = (fx pc.x / pc.z + cx - u, fy pc.y / pc.z + cy - v) */
#define G2OHIP_E_PROJECT_P2SC 12 /* EdgeProjectP2SC (EDGE_PROJECT_P2SC): meas u v u_r; info 3x3; rows 0-1 as
                                    G2OHIP_E_PROJECT_P2MC, e2 = fx (pc.x - baseline) / pc.z + cx - u_r */
/* Offset and bearing edges of types_slam3d / types_slam2d, what g2o_simulator3d's pose sensor and g2o_simulator2d's
 * bearing sensor write. Generic slot path. Robust kernels, edge levels, g2ohip_edge_chi2 and g2ohip_classify_edges take
 * them like any device type; none has isDepthPositive, so depth_positive != NULL or check_depth is G2OHIP_ERR_ARG.
 * lm_pcg6_3_eigen refuses a graph that holds any of them (g2ohip_last_error says so). Edges whose parameter records
 * are all equal share one record on the device, and likewise the information. */
#define G2OHIP_E_SE3_OFFSET 13 /* EdgeSE3Offset (EDGE_SE3_OFFSET), edge_se3_offset.cpp:102-132: v0, v1 both
                                  G2OHIP_V_SE3_QUAT; meas x y z qx qy qz qw (q normalised on entry, as
                                  EdgeSE3Offset::read); info 6x6; params n x 14: ParameterSE3Offset::offset() of the
                                  from vertex, then of the to vertex, each x y z qx qy qz qw (q normalised); NULL: both
                                  the identity. error = toVectorMQT(Z^-1 (Xi Pi)^-1 (Xj Pj)); the reference's analytic
                                  Jacobians (isometry3d_gradients.h:84-189, the non-__clang__ branch) */
#define G2OHIP_E_SE2_OFFSET 14 /* EdgeSE2Offset (EDGE_SE2_OFFSET), edge_se2_offset.cpp:102-106: v0, v1 both
                                  G2OHIP_V_SE2; meas x y theta; info 3x3; params n x 6: the two ParameterSE2Offset as
                                  x y theta, from then to; NULL: both the identity. error = Z^-1 (Xi Pi)^-1 (Xj Pj) as
                                  (x, y, normalised angle); exact Jacobians (the reference differentiates numerically) */
#define G2OHIP_E_SE2_XY_BEARING 15 /* EdgeSE2PointXYBearing (EDGE_BEARING_SE2_XY), edge_se2_pointxy_bearing.h:43-50: v0
                                      G2OHIP_V_SE2, v1 G2OHIP_V_XY, in g2o's order; meas one angle; info 1x1; params
                                      must be NULL (non-NULL is G2OHIP_ERR_ARG). With d = v0^-1 * l:
                                      error = normalize_theta(z - atan2(d.y, d.x)); exact Jacobians (the reference
                                      differentiates numerically), singular at d = 0 as the reference's error is. With
                                      marginalised landmarks it runs on the 3/2 Schur path, in structure_only_2 and
                                      on landmark shards, as G2OHIP_E_SE2_XY does */
/* An edge type the device does not know (any BaseBinaryEdge<D, E, Vi, Vj> between registered vertices of
 * dimension 2, 3, 6 or 7): the host's own linearizeOplus (the type's analytic one, or BaseBinaryEdge's numeric
 * central differences, base_binary_edge.hpp:198-266) supplies the error and both Jacobians, see
 * g2ohip_set_host_jacobians; the device assembles, marginalises and solves. meas unused (may be NULL);
 * info D*D. Several host-J types (different D) may coexist with the device types in one graph. */
#define G2OHIP_E_HOSTJ(D) (32 + (D)) /* D = error dimension, 1..7 */
/* ---- unary edge types (BaseUnaryEdge, core/base_unary_edge.hpp:49-78): one vertex, v0; g2ohip_add_edges takes them
 * with v1 == NULL (a non-NULL v1 is G2OHIP_ERR_ARG, as a NULL v1 is for the binary types). A unary edge on a fixed
 * vertex is inactive (sparse_optimizer.cpp:241, allVerticesFixed): it adds nothing to chi2, H or b. A vertex whose
 * only edges are unary is an active vertex like any other. A BA graph that also holds unary edges is assembled on the
 * generic slot path, not the fused one (as a mixed monocular + stereo graph is). ---- */
#define G2OHIP_E_SE2_PRIOR 16    /* EdgeSE2Prior, edge_se2_prior.h:39-77: v0 G2OHIP_V_SE2; meas x y theta; info 3x3 */
#define G2OHIP_E_SE2_XY_PRIOR 17 /* EdgeSE2XYPrior, edge_se2_xyprior.h:39-71: v0 G2OHIP_V_SE2; meas x y; info 2x2 */
#define G2OHIP_E_XY_PRIOR 18     /* EdgeXYPrior, edge_xy_prior.h: v0 G2OHIP_V_XY; meas x y; info 2x2 */
#define G2OHIP_E_SE3_PRIOR 19    /* EdgeSE3Prior, edge_se3_prior.cpp:89-102: v0 G2OHIP_V_SE3_QUAT; meas x y z qx qy qz qw;
                                    info 6x6; params: the sensor offset x y z qx qy qz qw per edge (n*7,
                                    ParameterSE3Offset), NULL = identity */
#define G2OHIP_E_XYZ_PRIOR 20    /* EdgeXYZPrior, edge_xyz_prior.cpp:63-70: v0 G2OHIP_V_XYZ; meas x y z; info 3x3 */
/* The pose-only projections (pose optimisation on tracked frames): unary, v0 the camera (G2OHIP_V_SE3_EXPMAP); the
 * 3-D point Xw and the intrinsics are members of the edge and come in params, one record per edge, NULL is
 * G2OHIP_ERR_ARG. Edges whose intrinsics are all equal share one record on the device. Not carried by .g2o files (the
 * reference's tags hold neither Xw nor the intrinsics): the loader skips the tags, g2ohip_save_g2o on a graph that
 * holds such edges writes nothing and returns G2OHIP_ERR_UNSUPPORTED. */
#define G2OHIP_E_SE3_PROJECT_XYZ_ONLYPOSE 21 /* EdgeSE3ProjectXYZOnlyPose, types_six_dof_expmap.h:232-258, .cpp:569-599:
                                    meas u v; info 2x2; params Xw.x Xw.y Xw.z fx fy cx cy (n*7) */
#define G2OHIP_E_STEREO_SE3_PROJECT_XYZ_ONLYPOSE 22 /* EdgeStereoSE3ProjectXYZOnlyPose, .h:293-319, .cpp:601-665: meas
                                    u_l v u_r; info 3x3; params Xw fx fy cx cy bf (n*8). As the reference's cam_project
                                    keeps 1/z in a float (.cpp:602), the error sees 1/z rounded to float, the Jacobian
                                    the double */
/* ---- g2o's own BA edges on a CameraParameters parameter (what upstream ba_demo builds): v0 the point (G2OHIP_V_XYZ),
 * v1 the camera (G2OHIP_V_SE3_EXPMAP), in g2o's vertex order. params: n*4, one CameraParameters per edge,
 * focal_length cx cy baseline (types_six_dof_expmap.h:42-78); NULL is G2OHIP_ERR_ARG. Edges whose records are all equal
 * share one record on the device. Error with pc = R p + t (SE3Quat::map), all doubles, in the operation order of
 * cam_map / stereocam_uvu_map (types_six_dof_expmap.cpp:74-87). Neither type has an isDepthPositive: depth_positive /
 * check_depth are G2OHIP_ERR_ARG. Alone in a graph either type takes the fused landmark-major assembly, mixed with any
 * other edge type the generic slot path; lm_pcg6_3_eigen refuses them. ---- */
#define G2OHIP_E_PROJECT_XYZ2UV 23  /* EdgeProjectXYZ2UV, types_six_dof_expmap.h:130-152: meas u v; info 2x2;
                                    e = (u - (pc.x/pc.z*f + cx), v - (pc.y/pc.z*f + cy)); the analytic Jacobians of
                                    .cpp:295-333 (G2OHIP_E_SE3_PROJECT_XYZ's with fx = fy = f). The baseline never
                                    enters; it stays on the host and g2ohip_save_g2o writes it back */
#define G2OHIP_E_PROJECT_XYZ2UVU 24 /* EdgeProjectXYZ2UVU, types_six_dof_expmap.h:178-198: meas u v u_r; info 3x3; rows
                                    0-1 as G2OHIP_E_PROJECT_XYZ2UV, row 2 = u_r - ((pc.x - b)/pc.z*f + cx), b the double
                                    as given (not G2OHIP_E_STEREO_SE3_PROJECT_XYZ's error: no float-rounded bf, and
                                    (x - b)/z*f instead of u - bf/z). The reference has no linearizeOplus for this edge
                                    (commented out, .h:196) and differentiates numerically; the device uses the exact
                                    first derivatives: rows 0-1 as XYZ2UV, row 2 = -(f/z, 0, -f(x - b)/z^2) applied to
                                    R for the point and to [-[pc]x | I] in (omega, upsilon) order for the camera, i.e.
                                    G2OHIP_E_STEREO_SE3_PROJECT_XYZ's row 2 with bf = f*b */
/* ---- types_icp (types/icp/types_icp.h): scan registration, what gicp_demo and gicp_sba_demo build. Robust kernels,
 * edge levels, g2ohip_edge_chi2 and g2ohip_classify_edges take both types like any device type; neither has
 * isDepthPositive (depth_positive != NULL or check_depth is G2OHIP_ERR_ARG). lm_pcg6_3_eigen refuses a graph that holds
 * either. ---- */
#define G2OHIP_E_V_V_GICP 25 /* Edge_V_V_GICP (EDGE_V_V_GICP), types_icp.h:161-238, types_icp.cpp:163-203: v0, v1 both
                                G2OHIP_V_SE3_QUAT; meas n x 12 in the file's order pos0 normal0 pos1 normal1 (the device
                                keeps the two positions, the normals stay on the host for g2ohip_save_g2o); info 3x3, the
                                point-to-plane information the caller supplies (gicp_demo: prec0(0.01)).
                                error = T0^-1 (T1 pos1) - pos0; the reference's analytic Jacobians
                                (GICP_ANALYTIC_JACOBIANS). params NULL: point-to-plane. params n x 12 (cov0 then cov1,
                                each the packed upper triangle 00 01 11 02 12 22): plane-to-plane, Omega =
                                (cov0 + R01 cov1 R01^T)^-1 is rebuilt on the device at every evaluation (types_icp.h:
                                220-226; chi2, the robust weight and the quadratic form use it, the Jacobians ignore
                                its dependence on the state, as the reference's do) and info may be NULL. Deviation:
                                the reference keeps pl_pl per edge, here it holds for the whole edge set (adding
                                edges with params to a set without, or the reverse, is G2OHIP_ERR_ARG). A graph whose
                                active binary edges are all of this type, without marginalised vertices, on one rank,
                                is assembled pair-major (g2ohip_set_pair_major) */
#define G2OHIP_E_XYZ_VSC 26  /* Edge_XYZ_VSC, types_icp.h:247-407: v0 G2OHIP_V_XYZ, v1 G2OHIP_V_SE3_QUAT standing for the
                                VertexSCam (a VertexSE3, camera-to-world, with VertexSE3's oplus; its cached w2n / w2i
                                are recomputed from the state on the device); meas u v u_r; info 3x3; params n x 5:
                                fx fy cx cy baseline, the reference's static Kcam and baseline (NULL is
                                G2OHIP_ERR_ARG; equal records are shared). error = mapPoint(point) - measurement in
                                mapPoint's order. The reference differentiates numerically (SCAM_ANALYTIC_JACOBIANS is
                                commented out); the device uses the exact first derivatives. Generic slot path; with
                                marginalised points the 6/3 Schur kernels, structure_only_3 and landmark shards, as
                                the other 6/3 projections. No .g2o file carries it (the reference's read / write
                                return false): g2ohip_save_g2o refuses a graph that holds it */
/* ---- types/sim3 (types_seven_dof_expmap.h): 7-DoF pose graphs, the vocabulary of monocular loop closing. A graph of
 * Sim3 poses is BlockSolver_7_3 without marginalised vertices: {lm,gn,dl}_hip_fix7_3 or *_hip_var. A free marginalised
 * point beside Sim3 poses is refused by the structure build (G2OHIP_ERR_UNSUPPORTED: the 7/3 Schur kernels do not
 * exist), a free non-marginalised one by the one-pose-block-size rule; lm_pcg*, gn_pcg* and lm_pcg6_3_eigen refuse a
 * Sim3 graph (pose blocks of 3 or 6 only). EdgeSim3ProjectXYZ and EdgeInverseSim3ProjectXYZ (ORB-SLAM's OptimizeSim3,
 * where the points are fixed) are the device types G2OHIP_E_SIM3_PROJECT_XYZ and G2OHIP_E_SIM3_PROJECT_INVERSE_XYZ
 * below; as G2OHIP_E_HOSTJ(2) between a fixed G2OHIP_V_XYZ point and a Sim3 vertex they still enter too. ---- */
#define G2OHIP_E_SIM3 27 /* EdgeSim3 (EDGE_SIM3:EXPMAP), types_seven_dof_expmap.h:110-137: v0, v1 both G2OHIP_V_SIM3; meas
                            the Sim3 C, 8 doubles in the vertex layout, normalised on entry as a vertex estimate is; info
                            7x7 in (omega, upsilon, sigma) order; params must be NULL (non-NULL is G2OHIP_ERR_ARG).
                            error = log(C * S0 * S1^-1) with all four branches of Sim3::log (sim3.h:141-220) as written.
                            The reference has no linearizeOplus for this edge and differentiates numerically; the device
                            uses the exact first derivatives of that closed-form log under the vertex's oplus:
                            Ji = M Ad(C), Jj = -M Ad(E), E = C S0 S1^-1, M = d log(exp(d) E) / d d. No isDepthPositive
                            (depth_positive != NULL or check_depth is G2OHIP_ERR_ARG); robust kernels, edge levels,
                            g2ohip_edge_chi2 and g2ohip_classify_edges take it like any device type */
#define G2OHIP_E_SIM3_PROJECT_XYZ 28 /* EdgeSim3ProjectXYZ (EDGE_PROJECT_SIM3_XYZ:EXPMAP), types_seven_dof_expmap.h:141-160:
                            v0 a G2OHIP_V_XYZ point, v1 a G2OHIP_V_SIM3, in g2o's vertex order; meas u v; info 2x2;
                            params must be NULL (non-NULL is G2OHIP_ERR_ARG): the intrinsics are camera 1 of v1
                            (g2ohip_set_sim3_cameras, or the VERTEX_SIM3:EXPMAP line). error = obs -
                            cam_map1(project(S.map(p))), S.map(p) = s (r p) + t in that order. The reference
                            differentiates numerically (its linearizeOplus is commented out); the device uses the exact
                            first derivatives under the vertex's oplus exp(u) S: with x = S.map(p) and
                            P = [[fx/z, 0, -fx x/z^2], [0, fy/z, -fy y/z^2]] at x, Jj = -P [ -[x]x | I | x ] and
                            Ji = -P s R; under g2ohip_set_sim3_fix_scale(1) column 6 of Jj is zero. The point is fixed
                            in every graph that initialises (a free marginalised one needs the 7/3 Schur kernels, a free
                            non-marginalised one breaks the one-pose-block-size rule), so the device forms Jj alone:
                            k_linearize_sim3_project writes the Sim3 vertex's slot and nothing else. No isDepthPositive
                            in the reference (depth_positive != NULL or check_depth is G2OHIP_ERR_ARG); robust kernels,
                            edge levels, g2ohip_edge_chi2, g2ohip_classify_edges, marginals and
                            g2ohip_update_initialization take it like any device type */
#define G2OHIP_E_SIM3_PROJECT_INVERSE_XYZ 29 /* EdgeInverseSim3ProjectXYZ (EDGE_PROJECT_INVERSE_SIM3_XYZ:EXPMAP), :163-180:
                            the same endpoints, measurement and information; the intrinsics are camera 2 of v1. error =
                            obs - cam_map2(project(S.inverse().map(p))), S.inverse() as the reference's constructor
                            builds it (conjugate, conj * (-t / s), 1 / s, then normalizeRotation). With (R', t', s') =
                            S^-1 and y = s' R' p + t': Jj = -P(y) s' R' [ [p]x | -I | -p ], Ji = -P(y) s' R' */
/* ---- examples/bal: "Bundle Adjustment in the Large" problems. Cameras of 9 parameters and marginalised points are
 * BlockSolver<BlockSolverTraits<9, 3>> (bal_example.cpp:301): {lm,gn,dl}_hip_fix9_3 or *_hip_var, with the 9/3 Schur
 * kernels. lm_pcg*, gn_pcg* and lm_pcg6_3_eigen refuse such a graph (pose blocks of 3 or 6 only), as do a sharded
 * structure build (g2ohip_set_comm* with nranks > 1) and structure_only_* on a point that carries the edge; a free
 * non-marginalised point beside the cameras breaks the one-pose-block-size rule. Host-Jacobian edges on a dimension-9
 * vertex are not supported. See g2ohip_load_bal / g2ohip_save_bal. ---- */
#define G2OHIP_E_OBSERVATION_BAL 30 /* EdgeObservationBAL, bal_example.cpp:156-281: v0 the camera (G2OHIP_V_CAM_BAL), v1
                            the point (G2OHIP_V_XYZ), in the reference's vertex order; meas u v; info 2x2 (equal records
                            are shared); params must be NULL (non-NULL is G2OHIP_ERR_ARG). With w = est[0:3] and
                            th = sqrt(w.w): P = X cos th + (v x X) sin th + v (v.X)(1 - cos th), v = w / th (th == 0:
                            P = X + w x X), P += t, p = -P.xy / P.z, r2 = p.p, rp = 1 + k1 r2 + k2 r2 r2,
                            e = f rp p - z, in the reference's operation order (:191-244). The reference differentiates
                            with ceres autodiff (:254-280); the device forms the same exact first derivatives of the
                            expression as written, branch by branch, term by term through th, v, sin and cos. No
                            isDepthPositive in the reference (depth_positive != NULL or check_depth is G2OHIP_ERR_ARG);
                            robust kernels, edge levels, g2ohip_edge_chi2 and g2ohip_classify_edges take it like any
                            device type. No .g2o file carries it (the reference's read / write return false):
                            g2ohip_save_g2o refuses a graph that holds it */
/* Any other BaseUnaryEdge<D, E, V> on a registered vertex of dimension 2, 3, 6 or 7 (an edge type of the application's own, say): the
 * host supplies the error and the Jacobian as for G2OHIP_E_HOSTJ, payload [e (D) | Ji (D x dim(v0))] row-major per
 * edge. meas unused (may be NULL); info D*D. */
#define G2OHIP_E_HOSTJ_UNARY(D) (48 + (D)) /* D = error dimension, 1..7 */

/* robust kernels (robust_kernel_impl.cpp; RobustKernelFactory names) */
#define G2OHIP_RK_NONE 0
#define G2OHIP_RK_HUBER 1
#define G2OHIP_RK_PSEUDO_HUBER 2
#define G2OHIP_RK_CAUCHY 3
#define G2OHIP_RK_GEMAN_MCCLURE 4
#define G2OHIP_RK_WELSCH 5
#define G2OHIP_RK_FAIR 6
#define G2OHIP_RK_TUKEY 7
#define G2OHIP_RK_SATURATED 8
#define G2OHIP_RK_DCS 9

/* status codes */
#define G2OHIP_OK 0
#define G2OHIP_ERR_ARG (-1)
#define G2OHIP_ERR_STATE (-2)
#define G2OHIP_ERR_DEVICE (-3)
#define G2OHIP_ERR_UNSUPPORTED (-4)

/* G2OBatchStatistics (core/batch_stats.h:42-72) + the current lambda */
typedef struct {
  int iteration;
  int numVertices;
  int numEdges;
  double chi2;
  double lambda;
  double timeResiduals;
  double timeQuadraticForm;
  int levenbergIterations;
  double timeSchurComplement;
  double timeSymbolicDecomposition;
  double timeNumericDecomposition;
  double timeLinearSolution;
  double timeLinearSolver;
  double timeUpdate;
  double timeIteration;
  long long hessianDimension;
  long long hessianPoseDimension;
  long long hessianLandmarkDimension;
  long long choleskyNNZ;
} g2ohip_batch_stats;

/* OptimizationAlgorithmLevenberg properties (optimization_algorithm_levenberg.cpp:48-49) */
typedef struct {
  int max_trials_after_failure; /* maxTrialsAfterFailure, default 10 */
  double user_lambda_init;      /* initialLambda, 0 -> tau * max diag (tau = 1e-5) */
  int verbose;                  /* SparseOptimizer::setVerbose: per-iteration line on stderr */
} g2ohip_config;

typedef struct g2ohip_graph g2ohip_graph;

/* ---- graph (OptimizableGraph / SparseOptimizer) ---- */
g2ohip_graph* g2ohip_graph_create(int device);
void g2ohip_graph_destroy(g2ohip_graph* g);
int g2ohip_add_vertices(g2ohip_graph* g, int type, int n, const int* ids, const double* est, const int* fixed,
                        const int* marginalized);
int g2ohip_add_edges(g2ohip_graph* g, int type, int n, const int* v0, const int* v1, const double* meas,
                     const double* info /* n * D*D row-major */, const double* params /* n*4, stereo n*5, or NULL */);
/* meas strides are the type's (G2OHIP_E_V_V_GICP: n*12, G2OHIP_E_XYZ_VSC: n*3). info may be NULL only for a
 * G2OHIP_E_V_V_GICP set in plane-to-plane mode (params given). */
/* params: the intrinsics of the projection types (G2OHIP_ERR_ARG when one of them gets NULL), the offsets of
 * G2OHIP_E_SE3_PRIOR and G2OHIP_E_SE3_XYZ (n*7, or NULL: identity), offset + intrinsics of G2OHIP_E_SE3_XYZ_DEPTH /
 * _DISPARITY (n*11, NULL is G2OHIP_ERR_ARG), the point and intrinsics of the pose-only projections (Xw fx fy cx cy,
 * n*7, stereo + bf, n*8; NULL is G2OHIP_ERR_ARG), the CameraParameters of G2OHIP_E_PROJECT_XYZ2UV / _XYZ2UVU (f cx cy
 * baseline, n*4; NULL is G2OHIP_ERR_ARG), the two covariances of a plane-to-plane G2OHIP_E_V_V_GICP set (n*12, or NULL:
 * point-to-plane), fx fy cx cy baseline of G2OHIP_E_XYZ_VSC (n*5; NULL is G2OHIP_ERR_ARG), NULL for the others (G2OHIP_E_SE3_EXPMAP among them). v1: NULL for the unary types (and only for them). */
/* .g2o files do not carry G2OHIP_E_STEREO_SE3_PROJECT_XYZ: the reference's reader and writer for its tag
 * (EDGE_STEREO_SE3_PROJECT_XYZ:EXPMAP, types_six_dof_expmap.cpp:469-493) move four measurement values through a
 * 3-vector and no intrinsics. The loader skips the tag like any unknown one; g2ohip_save_g2o on a graph that holds
 * such edges writes nothing and returns G2OHIP_ERR_UNSUPPORTED (g2ohip_last_error says why).
 * Nor do they carry G2OHIP_E_PROJECT_XYZ2UVU: the reference's reader for EDGE_PROJECT_XYZ2UVU:EXPMAP
 * (types_six_dof_expmap.cpp:335-346) reads no parameter id, so a loaded edge has no camera and addEdge rejects it
 * (optimizable_graph.cpp:277-280). The loader always skips the tag; g2ohip_save_g2o on a graph that holds such edges
 * writes nothing and returns G2OHIP_ERR_UNSUPPORTED. */
int g2ohip_load_g2o(g2ohip_graph* g, const char* path, int marginalize_xyz);
/* g2ohip_load_g2o with flags. G2OHIP_LOAD_UNARY: the unary tags EDGE_PRIOR_SE2, EDGE_PRIOR_SE2_XY, EDGE_PRIOR_XY,
 * EDGE_POINTXYZ_PRIOR, EDGE_SE3_PRIOR and the PARAMS_SE3OFFSET lines the last one refers to are parsed (by the same
 * parallel chunked parser) instead of skipped; an EDGE_SE3_PRIOR naming a parameter id the file does not define, a
 * prior on a vertex of the wrong type or a short line fails the load (g2ohip_last_error says which). flags = 0 is
 * g2ohip_load_g2o, which skips these tags like any unknown one. */
#define G2OHIP_LOAD_UNARY 1u
/* G2OHIP_LOAD_SLAM3D (may be combined with G2OHIP_LOAD_UNARY): VERTEX_TRACKXYZ id x y z loads as G2OHIP_V_XYZ
 * (marginalized according to marginalize_xyz); PARAMS_SE3OFFSET and PARAMS_CAMERACALIB (id, x y z qx qy qz qw, fx fy cx
 * cy; parameter_camera.cpp:62-85) are read; EDGE_SE3_TRACKXYZ, EDGE_PROJECT_DEPTH and EDGE_PROJECT_DISPARITY (v0 v1
 * paramId m0 m1 m2, then the six upper-triangle information values) load as G2OHIP_E_SE3_XYZ, _DEPTH and _DISPARITY. A
 * parameter id that no line defines, or one of the wrong kind, fails the load with the id in g2ohip_last_error. */
#define G2OHIP_LOAD_SLAM3D 2u
/* G2OHIP_LOAD_EXPMAP (may be combined with the other flags): EDGE_SE3:EXPMAP v0 v1 m0..m6, then the 21 upper-triangle
 * information values, loads as G2OHIP_E_SE3_EXPMAP. As in the reference (types_six_dof_expmap.cpp:114-129) the seven
 * values are cam2world and the stored measurement is their inverse; the information is taken as is. A short line, or
 * an endpoint that is no VERTEX_SE3:EXPMAP, fails the load (g2ohip_last_error names the tag). Without the flag the tag
 * is skipped like any unknown one. The pose-only projection tags (EDGE_SE3_PROJECT_XYZONLYPOSE:EXPMAP,
 * EDGE_STEREO_SE3_PROJECT_XYZONLYPOSE:EXPMAP) are always skipped: see G2OHIP_E_SE3_PROJECT_XYZ_ONLYPOSE. */
#define G2OHIP_LOAD_EXPMAP 4u
/* G2OHIP_LOAD_SBA (may be combined with the other flags): VERTEX_CAM id and 12 values loads as G2OHIP_V_CAM; a line
 * with exactly 7 values takes the reference's defaults 300 300 320 320 0.1 for fx fy cx cy baseline (VertexCam::read,
 * types_sba.cpp:74-112); any other length fails the load, g2ohip_last_error naming the tag. EDGE_PROJECT_P2MC v0 v1 u v
 * and EDGE_PROJECT_P2SC v0 v1 u v u_r load as G2OHIP_E_PROJECT_P2MC / _P2SC with identity information (the reference
 * reads none); an endpoint that is missing or of the wrong type fails the load. Without the flag the three tags are
 * skipped like any unknown one. */
#define G2OHIP_LOAD_SBA 8u
/* G2OHIP_LOAD_OFFSET (may be combined with the other flags): PARAMS_SE2OFFSET id x y theta and PARAMS_SE3OFFSET id
 * x y z qx qy qz qw are read; EDGE_SE3_OFFSET v0 v1 pidFrom pidTo, 7 measurement values and 21 upper-triangle
 * information values loads as G2OHIP_E_SE3_OFFSET; EDGE_SE2_OFFSET v0 v1 pidFrom pidTo x y theta and 6 upper-triangle
 * values as G2OHIP_E_SE2_OFFSET; EDGE_BEARING_SE2_XY v0 v1 angle info00 as G2OHIP_E_SE2_XY_BEARING. A parameter id no
 * line defines or one of the wrong kind, an endpoint that is missing or of the wrong type and a short line fail the
 * load, g2ohip_last_error naming the tag or the id. Without the flag the three edge tags and PARAMS_SE2OFFSET are
 * skipped like any unknown one. */
#define G2OHIP_LOAD_OFFSET 16u
/* G2OHIP_LOAD_CAMERAPARAMS (may be combined with the other flags): PARAMS_CAMERAPARAMETERS id focal_length cx cy
 * baseline is read; EDGE_PROJECT_XYZ2UV:EXPMAP v0 v1 paramId u v info00 info01 info11 (types_six_dof_expmap.cpp:248-263)
 * loads as G2OHIP_E_PROJECT_XYZ2UV. A parameter id no line defines or one of another kind, an endpoint that is missing
 * or of the wrong type and a short line fail the load, g2ohip_last_error naming the tag or the id. Without the flag
 * both tags are skipped like any unknown one. */
#define G2OHIP_LOAD_CAMERAPARAMS 32u
/* G2OHIP_LOAD_ICP (may be combined with the other flags): EDGE_V_V_GICP v0 v1 pos0 normal0 pos1 normal1 (12 values,
 * types_icp.cpp:124-160) loads as G2OHIP_E_V_V_GICP, point-to-plane, with the information Edge_V_V_GICP::read builds:
 * R0^T diag(0.01, 0.01, 1) R0, R0 from makeRot0 (types_icp.h:84-96). Deviation: makeRot0 normalises
 * (0,1,0) - normal0.y normal0 without a check, so a normal0 parallel to (0,1,0) divides by zero; such a line fails the
 * load with G2OHIP_ERR_ARG (g2ohip_last_error names the line number) and nothing of it is stored. An endpoint that is
 * missing or no VERTEX_SE3:QUAT and a short line fail the load too. Without the flag the tag is skipped. */
#define G2OHIP_LOAD_ICP 64u
/* G2OHIP_LOAD_SIM3 (may be combined with the other flags): VERTEX_SIM3:EXPMAP id v0..v6 fx fy cx cy loads as
 * G2OHIP_V_SIM3: the seven values are the log of cam2world and the estimate is Sim3(v).inverse()
 * (types_seven_dof_expmap.cpp:66-87); the four intrinsics (_focal_length1, _principle_point1) stay on the host for
 * g2ohip_save_g2o. A line with exactly 7 values takes the constructor's defaults 1 1 0 0; any other length fails the
 * load, g2ohip_last_error naming the tag. EDGE_SIM3:EXPMAP v0 v1 m0..m6 and the 28 upper-triangle information values
 * loads as G2OHIP_E_SIM3 with the measurement Sim3(m).inverse() (:104-122); a short line or an endpoint that is no
 * VERTEX_SIM3:EXPMAP fails the load. Without the flag both tags are skipped like any unknown one. g2ohip_save_g2o writes both
 * tags the reference's way (:89-102, 124-137): the log of the inverse, the intrinsics, the upper triangle.
 * EDGE_PROJECT_SIM3_XYZ:EXPMAP and EDGE_PROJECT_INVERSE_SIM3_XYZ:EXPMAP are read under G2OHIP_LOAD_SIM3_PROJECT alone. */
#define G2OHIP_LOAD_SIM3 128u
/* G2OHIP_LOAD_SIM3_PROJECT (with G2OHIP_LOAD_SIM3, which reads the vertices): EDGE_PROJECT_SIM3_XYZ:EXPMAP v0 v1 u v i00 i01
 * i11 loads as G2OHIP_E_SIM3_PROJECT_XYZ and EDGE_PROJECT_INVERSE_SIM3_XYZ:EXPMAP, the same line, as
 * G2OHIP_E_SIM3_PROJECT_INVERSE_XYZ (types_seven_dof_expmap.cpp:146-203). A short line, a v0 that is no VERTEX_XYZ or a v1
 * that is no VERTEX_SIM3:EXPMAP fails the load, g2ohip_last_error naming the tag. Camera 1 of a vertex is what its
 * VERTEX_SIM3:EXPMAP line holds; no line carries camera 2, in the reference either: it keeps its default 1 1 0 0 until
 * g2ohip_set_sim3_cameras. The points must end up fixed (FIX lines, marginalize_xyz = 0) or initialisation refuses the
 * graph (see types/sim3 above). Without the flag both tags are skipped like any unknown one. g2ohip_save_g2o writes
 * both tags the reference's way: u v and the upper triangle. */
#define G2OHIP_LOAD_SIM3_PROJECT 256u
int g2ohip_load_g2o_ex(g2ohip_graph* g, const char* path, int marginalize_xyz, unsigned flags);
/* Unary edges are written under the reference's tags and formats (edge_se2_prior.cpp:57-65, edge_se2_xyprior.cpp:50-58,
 * edge_xy_prior.cpp, edge_xyz_prior.cpp:54-61, edge_se3_prior.cpp:77-86), with one PARAMS_SE3OFFSET id x y z qx qy qz qw
 * line per distinct offset ahead of the vertices; host-J unary edges are left out with a warning, as binary host-J
 * ones are. The slam3d landmark edges are written as EDGE_SE3_TRACKXYZ / EDGE_PROJECT_DEPTH / EDGE_PROJECT_DISPARITY
 * (edge_se3_pointxyz.cpp:88-96 and its siblings), their parameters as PARAMS_SE3OFFSET / PARAMS_CAMERACALIB lines, one
 * per distinct record, in one id space with the prior offsets; a G2OHIP_V_XYZ vertex one of these edges touches is
 * written as VERTEX_TRACKXYZ. G2OHIP_E_SE3_EXPMAP edges are written as EDGE_SE3:EXPMAP with the inverse of the
 * measurement and the upper triangle of the information (types_six_dof_expmap.cpp:131-140). A graph holding pose-only
 * projection edges is not written: G2OHIP_ERR_UNSUPPORTED, as for G2OHIP_E_STEREO_SE3_PROJECT_XYZ. G2OHIP_V_CAM
 * vertices are written as VERTEX_CAM with their 12 values, G2OHIP_E_PROJECT_P2MC / _P2SC as EDGE_PROJECT_P2MC /
 * EDGE_PROJECT_P2SC with the measurement alone (types_sba.cpp:114-131, 215-244); the points they touch stay
 * VERTEX_XYZ. These lines cannot carry an information matrix: a graph holding such an edge whose information is not
 * the identity is not written (G2OHIP_ERR_UNSUPPORTED, nothing written). G2OHIP_E_SE3_OFFSET / _SE2_OFFSET edges are
 * written as EDGE_SE3_OFFSET / EDGE_SE2_OFFSET v0 v1 pidFrom pidTo, the measurement and the upper triangle of the
 * information (edge_se3_offset.cpp:90-100, edge_se2_offset.cpp:86-94), with one PARAMS_SE3OFFSET / PARAMS_SE2OFFSET
 * line per distinct offset in the same id space; G2OHIP_E_SE2_XY_BEARING as EDGE_BEARING_SE2_XY v0 v1 angle info00.
 * G2OHIP_E_PROJECT_XYZ2UV edges are written as EDGE_PROJECT_XYZ2UV:EXPMAP v0 v1 paramId u v and the upper triangle of
 * the information (types_six_dof_expmap.cpp:265-276), with one PARAMS_CAMERAPARAMETERS id focal_length cx cy baseline
 * line per distinct record in the same id space. G2OHIP_E_V_V_GICP edges are written as EDGE_V_V_GICP v0 v1 and the 12
 * values pos0 normal0 pos1 normal1 (types_icp.cpp:206-222): as in the reference the line carries neither the
 * information nor the covariances, a reader rebuilds the point-to-plane information from normal0. A graph holding
 * G2OHIP_E_XYZ_VSC or G2OHIP_E_OBSERVATION_BAL edges is not written (G2OHIP_ERR_UNSUPPORTED, nothing written). */
int g2ohip_save_g2o(g2ohip_graph* g, const char* path);
/* The BAL text format as bal_example.cpp:336-406 reads it: "ncams npts nobs", nobs records "cam pt x y", 9 * ncams
 * camera values, 3 * npts point values, with whitespace of any kind between the tokens. Cameras become G2OHIP_V_CAM_BAL
 * vertices with ids 0 .. ncams-1, points G2OHIP_V_XYZ vertices with ids ncams .. ncams+npts-1 (marginalised according to
 * the flag), observations G2OHIP_E_OBSERVATION_BAL edges whose information is the identity, held as one shared record.
 * A short file, counts the file is too short for, a token that is no finite decimal number ("nan", "inf" and
 * hexadecimal floats among them) or an index out of range is G2OHIP_ERR_ARG, g2ohip_last_error names the record, and
 * the graph is left as it was: the file is parsed and checked as a whole before a vertex is added. */
int g2ohip_load_bal(g2ohip_graph* g, const char* path, int marginalize_points);
/* Writes the same format from the current estimates, with 17 significant digits: load -> save -> load is bitwise. The
 * graph must hold only G2OHIP_V_CAM_BAL, G2OHIP_V_XYZ and G2OHIP_E_OBSERVATION_BAL, ids of the shape g2ohip_load_bal
 * gives (cameras 0 .. ncams-1, then the points) and identity information; otherwise G2OHIP_ERR_UNSUPPORTED and nothing
 * is written. */
int g2ohip_save_bal(g2ohip_graph* g, const char* path);
int g2ohip_num_vertices(g2ohip_graph* g);
int g2ohip_num_edges(g2ohip_graph* g);
/* estimates of one vertex type in insertion order (syncs device state to host first) */
int g2ohip_get_estimates(g2ohip_graph* g, int type, double* out, int* ids_out);
/* overwrite estimates of one vertex type (insertion order) — host-authoritative Solver mode */
int g2ohip_set_estimates(g2ohip_graph* g, int type, const double* est);
/* minimal state vector concatenated in vertex-id order (parity checks) */
int g2ohip_minimal_state(g2ohip_graph* g, double* out);

/* OptimizableGraph::Edge::setRobustKernel (optimizable_graph.h; base_binary_edge.hpp:104-135 weighted
 * quadratic form, sparse_optimizer.cpp:102-116 robust chi2) for every edge of a type: kind G2OHIP_RK_*,
 * delta = RobustKernel::setDelta. G2OHIP_RK_NONE removes it. */
int g2ohip_set_robust_kernel(g2ohip_graph* g, int edge_type, int kind, double delta);
/* Host-computed linearization of the G2OHIP_E_HOSTJ(D) edges of one type, in insertion order: per edge
 * [e (D) | Ji (D x dim(v0)) | Jj (D x dim(v1))], row-major, at the estimates the device holds (call after
 * g2ohip_set_estimates, before g2ohip_solver_build_system). The J_host_fallback of SURVEY.md 8b.
 * G2OHIP_E_HOSTJ_UNARY(D) edges: per edge [e (D) | Ji (D x dim(v0))]. */
int g2ohip_set_host_jacobians(g2ohip_graph* g, int edge_type, const double* payload);
/* Callback for the device-resident loops (g2ohip_optimize / g2ohip_chi2) when host-J edges exist: fill the
 * payload of every edge of `edge_type` at the current estimates (read them with g2ohip_get_estimates);
 * with_jacobians = 0 only needs the errors. Return 0 on success. */
typedef int (*g2ohip_host_edge_fn)(void* user, int edge_type, int with_jacobians, double* payload);
int g2ohip_set_host_edge_callback(g2ohip_graph* g, g2ohip_host_edge_fn fn, void* user);
/* Length in doubles of the payload buffer of a host-J edge type (the `payload` the callback fills and
 * g2ohip_set_host_jacobians reads): sum over its edges of D * (1 + dim(v0) + dim(v1)), for a unary host-J type of
 * D * (1 + dim(v0)). A callback must write exactly this many doubles. */
long long g2ohip_host_payload_len(g2ohip_graph* g, int edge_type);

/* OptimizationAlgorithmFactory::construct by name; default "lm_hip_var". "lm_pcg6_3_eigen" (matrix-free CGLS on the
 * Jacobian of BA edges) does not take unary edges (priors, the pose-only projections), the slam3d landmark edges or
 * G2OHIP_E_SE3_EXPMAP: building the structure of such a graph under it returns G2OHIP_ERR_UNSUPPORTED.
 * "dl_hip_{var,fix6_3,fix3_2,fix3_3,fix6_6}" is OptimizationAlgorithmDogleg over the Cholesky solver ("dl_pcg*" is
 * unknown: the reference registers no dogleg over PCG, the step needs an exact Gauss-Newton solve). Under dl_* the
 * max_trials_after_failure and user_lambda_init of g2ohip_config are ignored (g2ohip_set_dogleg_params),
 * g2ohip_batch_stats.levenbergIterations stays 0 and .lambda is the damping of the not-PD branch while it is in use,
 * else 0. A sharded graph (g2ohip_set_comm*, nranks > 1) under dl_* returns G2OHIP_ERR_UNSUPPORTED from the structure
 * build: the step multiplies by Hpp, whose diagonal blocks are partial on a landmark shard. */
int g2ohip_set_algorithm(g2ohip_graph* g, const char* name);
/* OptimizationAlgorithmDogleg properties (optimization_algorithm_dogleg.cpp:45-48); a value <= 0 keeps the default:
 * initialDelta 1e4, maxTrialsAfterFailure 100, initialLambda 1e-7, lambdaFactor 10 */
/* Pair-major assembly (G2OHIP_E_V_V_GICP): a graph whose active binary edges are all Edge_V_V_GICP (unary priors may be
 * present), with no marginalised vertex and on one rank, sorts its edges by vertex pair, sums each chunk of <= 64
 * edges of a pair inside the linearize wave and each pair's chunks in one workgroup, instead of writing and reducing
 * per-edge slots. enable = 0 keeps such a graph on the generic slot path (the same Hpp / b within rounding; for
 * comparisons), 1 (the default) takes the pair-major path where it applies. Takes effect at the next structure build.
 * g2ohip_pair_major_info: out[0] = 1 when the built structure is pair-major, out[1] its pairs, out[2] its chunks. */
int g2ohip_set_pair_major(g2ohip_graph* g, int enable);
/* VertexSim3Expmap::_fix_scale (types_seven_dof_expmap.h:77-78, 101), for every G2OHIP_V_SIM3 vertex of the handle: on = 1
 * makes oplus zero update[6], so the scale of no vertex moves. The reference differentiates EdgeSim3 numerically
 * through oplusImpl, so under _fix_scale column 6 of both of its Jacobians is zero; the device zeroes that column too,
 * and column 6 of the Sim3 projection edges' Jj.
 * H(6, 6) of every vertex block then holds lambda alone: Levenberg-Marquardt works, Gauss-Newton and the undamped
 * dogleg solve on such a graph are not positive definite. That is the reference's behaviour. Host-Jacobian edges on Sim3
 * vertices must supply such Jacobians themselves. on other than 0 or 1: G2OHIP_ERR_ARG. */
int g2ohip_set_sim3_fix_scale(g2ohip_graph* g, int on);
/* VertexSim3Expmap::_focal_length1 / _principle_point1 and _focal_length2 / _principle_point2
 * (types_seven_dof_expmap.h:84-99) of n G2OHIP_V_SIM3 vertices: cam1 and cam2 are n * 4 doubles fx fy cx cy, NULL
 * leaves that camera as it is. Both default to 1 1 0 0; camera 1 is also what a VERTEX_SIM3:EXPMAP line sets and
 * g2ohip_save_g2o writes. G2OHIP_E_SIM3_PROJECT_XYZ reads camera 1 of its v1, G2OHIP_E_SIM3_PROJECT_INVERSE_XYZ camera 2.
 * A change after the edges are on the device reaches it before the next evaluation. An id that is no G2OHIP_V_SIM3
 * vertex: G2OHIP_ERR_ARG, and nothing changes. */
int g2ohip_set_sim3_cameras(g2ohip_graph* g, int n, const int* ids, const double* cam1, const double* cam2);
int g2ohip_pair_major_info(g2ohip_graph* g, int out[3]);
int g2ohip_set_dogleg_params(g2ohip_graph* g, double initial_delta, int max_trials_after_failure,
                             double initial_lambda, double lambda_factor);
/* state after the last dogleg iteration: out[0] delta (trustRegion()), out[1] lastStep (1 SD, 2 GN, 3 DL, 0 undefined;
 * the reference's enum order), out[2] lastNumTries, out[3] currentLambda, out[4] wasPDInAllIterations; n >= 5 */
int g2ohip_dogleg_state(g2ohip_graph* g, double* out, int n);
/* StructureOnlySolver<PointDoF>::calc(points, num_iters, num_max_trials) (structure_only_solver.h:72-212), as ba_demo
 * and sba_demo call it before the joint optimisation: with every other vertex held fixed, each landmark runs its own
 * damped Gauss-Newton loop (mu = 0.01 and nu = 2 fresh per point and per call, :86-87; gradient stop |b| < 0.001, :148;
 * accept on chi2 - new_chi2 > 0 with a finite new_chi2, mu *= 1/3, :179-195; else mu *= nu, nu *= 2 and the point stops
 * after num_max_trials failures in a row, :197-203; a non-finite trial chi2 is a rejected trial). One kernel launch runs
 * all iterations and trials of every point. Callable after g2ohip_initialize under any algorithm.
 * ids == NULL: every marginalised active vertex (init(), :214-225; none: nothing is done, G2OHIP_OK), n is ignored.
 * Otherwise n landmark ids; an unknown id, one that is no marginalised active vertex or one given twice returns
 * G2OHIP_ERR_ARG and changes nothing. num_iters < 0 or num_max_trials < 1: G2OHIP_ERR_ARG. All edges of the landmark
 * count (v->edges(), :82: an edge to a fixed camera included): EdgeSE3ProjectXYZ, EdgeStereoSE3ProjectXYZ, the three
 * slam3d landmark edges, EdgeSE2PointXY, EdgeXYZPrior and EdgeXYPrior in any mix, each under its type's robust kernel.
 * counts (may be NULL) receives the totals over the points: [0] accepted steps, [1] rejected trials, [2] points stopped
 * by the gradient test, [3] points stopped by exhausted trials, [4] fixed points skipped (:104); per-block partial
 * counts summed in block order. Cameras, poses and fixed points are not written; the push / pop stack is not touched;
 * the next chi2, buildSystem, optimize or stage sees the new landmarks. G2OHIP_ERR_UNSUPPORTED (text in
 * g2ohip_last_error): a sharded graph (nranks > 1), a landmark that carries a host-Jacobian edge (G2OHIP_E_HOSTJ*),
 * another edge type on a marginalised vertex.
 * Under "structure_only_3" / "structure_only_2" g2ohip_optimize and g2ohip_optimize_step run calc(points, 1) per
 * iteration (solve(), :65-70: mu restarts at 0.01 every iteration, a trajectory other than calc(points, n)'s), always
 * answer OK (g2ohip_optimize returns the iteration count), fill stats.chi2 with the robust chi2 after the step and
 * leave levenbergIterations 0. g2ohip_initialize (and the calls above) return G2OHIP_ERR_UNSUPPORTED when the
 * marginalised vertices' dimension is not the name's (the reference asserts it, :81). */
int g2ohip_structure_only_calc(g2ohip_graph* g, int n, const int* ids, int num_iters, int num_max_trials,
                               long long* counts);
/* SparseOptimizer::initializeOptimization(0): active edges/vertices, index mapping. The same as
 * g2ohip_initialize_level(g, 0). */
int g2ohip_initialize(g2ohip_graph* g);

/* ---- edge levels, per-edge chi2, outlier classification (the pose-optimisation / local-BA loop of ORB-SLAM-style
 * callers: optimise, read every edge's chi2() and isDepthPositive(), setLevel(1) the bad ones,
 * initializeOptimization(0), optimise again) ---- */
#define G2OHIP_LEVEL_KEEP (-2147483647 - 1)
/* OptimizableGraph::Edge::setLevel / level() (optimizable_graph.h), per edge of a type in insertion order. Every edge
 * starts at level 0. idx == NULL: n must be the type's edge count and levels[k] is edge k's level; otherwise idx[k]
 * selects the edges. An index out of range or given twice, a negative level, or a type the graph holds no edge of
 * returns G2OHIP_ERR_ARG and changes nothing. As in the reference a changed level has no effect until the next
 * g2ohip_initialize*: chi2, optimize, build_system and stage keep the active set of the last initialisation. */
int g2ohip_set_edge_levels(g2ohip_graph* g, int edge_type, int n, const int* idx, const int* levels);
/* the levels of the type's edges into out (up to cap of them; out may be NULL); returns the type's edge count */
int g2ohip_get_edge_levels(g2ohip_graph* g, int edge_type, int* out, int cap);
/* SparseOptimizer::initializeOptimization(level) (sparse_optimizer.cpp:201-279): an edge is active when level < 0 or
 * its level equals `level`, and (unary edges) its vertex is not fixed; a vertex is active when it has an active edge
 * (:228-249), so a landmark whose observations were all set aside leaves the system. Unlike the reference (:241,
 * allVerticesFixed) a binary edge between two fixed vertices stays active, as it always has here: it adds nothing to the
 * system and a constant to g2ohip_chi2. The vertex types of every edge are checked, whatever its level
 * (G2OHIP_ERR_UNSUPPORTED). The handle remembers the level:
 * g2ohip_update_initialization filters the new edges by it, and a graph grown by g2ohip_add_* is initialised again at
 * it by the next chi2 / optimize. No active edge: G2OHIP_ERR_STATE; no active free pose: G2OHIP_ERR_UNSUPPORTED (as
 * g2ohip_initialize on an empty / pose-less graph). Host-Jacobian types take levels like any other (the payload still
 * covers every edge of the type in insertion order), sharded handles too. g2ohip_structure_only_calc and the
 * structure_only_* algorithms use every edge of an active landmark whatever its level (v->edges(),
 * structure_only_solver.h:82); g2ohip_save_g2o writes every edge. */
int g2ohip_initialize_level(g2ohip_graph* g, int level);
/* Edge::chi2() = e^T Omega e (base_edge.h; NOT robustified, whatever robust kernel the type has) of EVERY edge of the
 * type in insertion order, active or not (another level, a unary edge on a fixed vertex, an edge between fixed
 * vertices), at the estimates the device holds. depth_positive (or NULL): isDepthPositive(), (z > 0) of the point in
 * the camera frame, for G2OHIP_E_SE3_PROJECT_XYZ, G2OHIP_E_STEREO_SE3_PROJECT_XYZ and the two *_ONLYPOSE types
 * (types_six_dof_expmap.h:218-222, 248-251, 279-283, 309-312); non-NULL for another type is G2OHIP_ERR_ARG.
 * G2OHIP_ERR_STATE before g2ohip_initialize* (or after edges or vertices were added and nothing initialised since);
 * G2OHIP_ERR_UNSUPPORTED (text in g2ohip_last_error) for host-Jacobian types, whose errors the host holds itself, and
 * on sharded handles (nranks > 1). */
int g2ohip_edge_chi2(g2ohip_graph* g, int edge_type, double* chi2, unsigned char* depth_positive);
/* chi2 / depth test and setLevel in one device pass over every edge of the type:
 * bad = chi2 > chi2_max || (check_depth && !(z > 0)) (a NaN chi2 is not bad by itself, as in the callers' C++);
 * level = bad ? outlier_level : inlier_level, G2OHIP_LEVEL_KEEP in either place leaves that edge's level as it is.
 * counts (or NULL): [0] edges with chi2 > chi2_max, [1] edges failing the depth test (0 when not checked), [2] bad
 * edges. check_depth on a type without the test, or a negative level other than G2OHIP_LEVEL_KEEP: G2OHIP_ERR_ARG.
 * Refusals as g2ohip_edge_chi2. The new levels are what g2ohip_get_edge_levels and the next g2ohip_initialize_level
 * see. */
int g2ohip_classify_edges(g2ohip_graph* g, int edge_type, double chi2_max, int check_depth, int inlier_level,
                          int outlier_level, long long counts[3]);
/* SparseOptimizer::updateInitialization(vset, eset) + BlockSolver::updateStructure (sparse_optimizer.cpp:465-502,
 * block_solver.hpp:258-312), online mode: after g2ohip_initialize (and optimizing), vertices and edges added with
 * g2ohip_add_vertices / g2ohip_add_edges join the optimization without re-indexing the existing ones — each new free
 * vertex (one that has an edge) takes the next hessian index, new vertices in id order; the next optimize / build
 * continues from the current (optimized) state with the grown structure. Non-Schur graphs only, as in the reference:
 * G2OHIP_ERR_UNSUPPORTED when the graph or a new vertex is marginalized (the reference aborts), G2OHIP_ERR_STATE
 * before g2ohip_initialize. Calling g2ohip_initialize instead re-indexes every vertex in id order. */
int g2ohip_update_initialization(g2ohip_graph* g);
/* computeActiveErrors + activeRobustChi2 on the device */
double g2ohip_chi2(g2ohip_graph* g);
/* SparseOptimizer::optimize(iterations) with the device-resident LM loop.
 * stats: array of `iterations` entries or NULL. Returns iterations done, 0 on Fail, <0 on error. */
int g2ohip_optimize(g2ohip_graph* g, const g2ohip_config* cfg, int iterations, g2ohip_batch_stats* stats);
/* One iteration of the SparseOptimizer::optimize loop (iteration 0 rebuilds the structure and the
 * initial lambda, exactly as optimize() does). Returns 0 OK, 1 Terminate, 2 Fail, <0 error. */
int g2ohip_optimize_step(g2ohip_graph* g, const g2ohip_config* cfg, int iteration, g2ohip_batch_stats* stats);

/* ---- Solver-level plugin (core/solver.h:54-137) for a g2o-side BlockSolverHip adapter ---- */
int g2ohip_solver_build_structure(g2ohip_graph* g);             /* Solver::buildStructure */
int g2ohip_solver_build_system(g2ohip_graph* g);                /* Solver::buildSystem */
int g2ohip_solver_set_lambda(g2ohip_graph* g, double lambda, int backup); /* Solver::setLambda */
int g2ohip_solver_restore_diagonal(g2ohip_graph* g);            /* Solver::restoreDiagonal */
int g2ohip_solver_solve(g2ohip_graph* g);                       /* Solver::solve: 1 ok, 0 not PD, <0 error */
long long g2ohip_solver_vector_size(g2ohip_graph* g);           /* Solver::vectorSize */
/* BlockSolver<p, l> traits after build_structure: dims = [PoseDim, LandmarkDim, pose blocks, landmark blocks]
 * (block_solver.h:44-60; Solver::additionalVectorSpace etc. not needed) */
int g2ohip_solver_block_dims(g2ohip_graph* g, int* dims);
/* Solver::x() / Solver::b() (host copies) in the Hessian order: poses, then the free landmarks. On one rank the
 * landmarks follow buildIndexMapping's id order (block_solver.hpp, sparse_optimizer.cpp:207-241). With landmark shards
 * aligned to the factorization's cut (g2ohip_set_comm, N > 1) the landmarks are regrouped by owning rank (stable in
 * id order within a rank). The vectors keep a slot for every landmark, but on a sharded rank only its own landmarks'
 * slots hold this rank's values: one contiguous range of the landmark part, whose landmark ids g2ohip_local_landmarks
 * lists in the order x / b carry them. */
int g2ohip_solver_get_x(g2ohip_graph* g, double* x);
int g2ohip_solver_get_b(g2ohip_graph* g, double* b);
/* BlockSolverBase::multiplyHessian (core/block_solver.h:94,146; used by OptimizationAlgorithmDogleg
 * optimization_algorithm_dogleg.cpp:100,179): dest = Hpp src with the upper blocks mirrored (+ lambda on the
 * diagonal while a setLambda is active), host arrays of hessianPoseDimension. Single rank only. */
int g2ohip_solver_multiply_hessian(g2ohip_graph* g, double* dest, const double* src);
/* max |diagonal entry| of the vertex Hessian blocks (Hpp, Hll) after buildSystem: the quantity
 * OptimizationAlgorithmLevenberg::computeLambdaInit reads through the vertices' mapped Hessians
 * (optimization_algorithm_levenberg.cpp:152-175) in the host-authoritative Solver mode. */
int g2ohip_solver_diag_absmax(g2ohip_graph* g, double* out);
/* Solver::setEta (core/solver.h:137, jacobi_solver.h:142): forcing term of the lm_pcg6_3_eigen CGLS (stop when
 * s.s < eta s0.s0, linear_solver_pcg_eigen.h:170-176); default 0.1 (core/linear_solver.h:66). */
int g2ohip_solver_set_eta(g2ohip_graph* g, double eta);
/* G2OBatchStatistics::iterationsLinearSolver of the last iterative linear solve: the CGLS's under lm_pcg6_3_eigen,
 * the block-Jacobi PCG's under the other *_pcg* algorithms */
int g2ohip_solver_linear_iterations(g2ohip_graph* g);
/* ||(A + lambda I) x - b|| / ||b|| of the last Solver::solve, evaluated on the device (A = the Schur complement
 * with Schur, else Hpp): a size-independent check of the factorization at any problem size. With landmark shards
 * (g2ohip_set_comm) it is a collective: every rank calls it (the reduced system is summed over ranks first when the
 * distributed factorization reduce-scattered it). */
int g2ohip_solver_linear_residual(g2ohip_graph* g, double* rel);
/* Symbolic / schedule summary of the device factorization: out[0..20] = n, nnz(L), flops (this ordering),
 * supernodes, tree levels, largest front, blocked fronts, levels assembled in place, pre-scattered levels,
 * trailing-update launches, big-panel backward rounds, out[11] = 0 (retired slot), and for landmark
 * shards (nranks > 1) this rank's fronts, the shared fronts, the subtree roots, the doubles of the root exchange
 * buffer (nranks all-gathered segments), the cost model of the best cut of the elimination tree (modelled seconds of
 * this rank's subtrees, of the shared top, of the replicated factorization, of the cut's exchanges: root all-gather and
 * x all-reduce) and whether the factorization is distributed (1) or
 * replicated (0: the model preferred replication, or G2OHIP_DIST_FACTOR=0); then out[21..25] = whether the reduced
 * system is reduce-scattered by subtree ownership (1) instead of all-reduced, its per-rank segment and all-reduced tail
 * (doubles), and the modelled seconds of that input exchange and of the plain all-reduce; out[26] = 0 (retired slot);
 * out[27] = the band-leaf size of the ordering (blocks; 0: plain nested dissection); out[28] = 1 when the landmark
 * shards are aligned with the cut (each landmark on the rank whose subtrees its Schur blocks land in, G2OHIP_DIST_ALIGN),
 * out[29] = doubles of this rank's subtree blocks read from its own partial reduced system (never exchanged), out[30] =
 * bytes this rank sends per LM trial through the reduced system's and the factorization's collectives (ring
 * algorithms), out[31] = free landmarks in this rank's shard, out[32] = the modelled sharded work (s) of the busiest
 * rank under this layout, out[33] = fronts whose panel steps factor only their own rows, L21 then formed as one GEMM
 * with the explicit L11^-1 (deferred L21, G2OHIP_CHOL_DEFER_L21); then the Schur row pass's schedule on this rank:
 * out[34], out[35] = tasks of the G-block set and of the Kt-record set (a sharded rank skips the row chunks nobody reads
 * from it), out[36], out[37] = row chunks of either set split into parts (G2OHIP_SCHUR_SPLIT_TASKS), out[38] = the
 * partial blocks those parts stage before their fixed-order sum, out[39] = cameras the split camera pass runs on this
 * rank (0: all cameras, no list). Returns the number of entries available. */
int g2ohip_solver_factor_info(g2ohip_graph* g, double* out, int n);
/* Landmark shards (g2ohip_set_comm / _set_comm_local): the ids of the free landmarks this rank holds (their estimates
 * are current on this rank only); ids may be NULL. Returns the count. With the distributed factorization the shards
 * follow its cut (not id ranges); otherwise they are contiguous ranges of the landmark order. */
int g2ohip_local_landmarks(g2ohip_graph* g, int* ids, int cap);
/* Solver::computeMarginals (core/solver.h:108; BlockSolver::computeMarginals block_solver.hpp:451-460 ->
 * LinearSolverCSparse::solvePattern linear_solver_csparse.h:190-225, MarginalCovarianceCholesky): the pose-block
 * entries (block_rows[k], block_cols[k]) (Hessian indices) of Hpp^-1, Hpp as the last build_system left it (no
 * lambda), each a pd x pd column-major block written to out + k * pd * pd. The whole pose system is factored on the
 * device (the LM's own factor when it factors Hpp), then one multi-right-hand-side supernodal solve per 64 / pd
 * requested block columns. Returns 1, or 0 when Hpp is not positive definite (the reference's bool), or a
 * negative status (unsupported on sharded graphs). */
int g2ohip_solver_compute_marginals(g2ohip_graph* g, int nblocks, const int* block_rows, const int* block_cols,
                                    double* out);
/* SparseOptimizer::update(x) + push/pop/discardTop on the device-resident state */
int g2ohip_update(g2ohip_graph* g, const double* x_host /* NULL: use device x */);
int g2ohip_push(g2ohip_graph* g);
int g2ohip_pop(g2ohip_graph* g);
int g2ohip_discard_top(g2ohip_graph* g);

/* Stage export for parity tests (small problems): after build_system + set_lambda + solve, the
 * dense reduced system and solution. dims: [n, n_pose_scalars, n_landmark_scalars]. */
int g2ohip_stage(g2ohip_graph* g, double lambda, double* b, double* x, double* Hschur_dense, double* bschur,
                 long long* dims);

/* Solver::saveHessian (core/block_solver.hpp:589-593 -> SparseBlockMatrix::writeOctave, sparse_block_matrix.hpp:579-617):
 * Hpp of the last buildSystem (+ lambda while a setLambda is active) as an Octave sparse-matrix text file, every entry of
 * every stored block plus the mirrored off-diagonal blocks, "%.9f". Returns 1 written, 0 not written, <0 error. */
int g2ohip_solver_save_hessian(g2ohip_graph* g, const char* path);
/* Solver::setWriteDebug (core/block_solver.hpp:582-586): when on, a factorization that meets a non-positive pivot
 * writes the matrix it factored (S, or Hpp + lambda) to "debug.txt" in the format of csparse_helper.cpp:62-111, as
 * LinearSolverCSparse::solve does (linear_solver_csparse.h:127-133). Default off. */
int g2ohip_solver_set_write_debug(g2ohip_graph* g, int on);

/* ---- LinearSolver-level plugin (core/linear_solver.h:42-105, LinearSolverCCS) ----
 * Solve A x = b for symmetric PD A given as UPPER CCS (n, Ap[n+1], Ai, Ax) of scalar entries,
 * with an optional block partition (nblocks, block_ends[] cumulative end offsets as in
 * SparseBlockMatrix::rowBlockIndices) used for the block ordering. Returns 1 ok, 0 not PD.
 * Accuracy (tests/test_gpu_cholesky_edges.py): against LAPACK's fp64 Cholesky on the same
 * system the normwise backward error stays within 64 x (measured: at most 10 x) up to cond_2 = 6e10, the forward
 * error within 64 x up to cond_2 = 6e8; at 6e10 one tridiagonal system, which LAPACK's natural order favours, was at
 * 64.8 x. */
int g2ohip_linear_solve_ccs(int device, int n, const int* Ap, const int* Ai, const double* Ax, const double* b,
                            double* x, int nblocks, const int* block_ends);
/* The same solve, and the schedule the factorization took: the first min(ninfo, 12) of info are filled with
 * g2ohip_solver_factor_info's out[0..10] (n, nnz(L), flops, supernodes, levels, largest front, blocked fronts, levels
 * assembled in place, levels pre-scattered, trailing-update launches, big-panel backward rounds) and, as info[11],
 * its out[33] (deferred-L21 fronts). info may be NULL when ninfo is 0. */
int g2ohip_linear_solve_ccs_ex(int device, int n, const int* Ap, const int* Ai, const double* Ax, const double* b,
                               double* x, int nblocks, const int* block_ends, double* info, int ninfo);

/* ---- multi-GPU (landmark sharding + RCCL all-reduce of the reduced camera system) ---- */
int g2ohip_comm_unique_id(unsigned char out[128]);
/* this rank keeps landmark shard `rank` of `nranks` (g2ohip_local_landmarks lists it) */
int g2ohip_set_comm(g2ohip_graph* g, const unsigned char uid[128], int rank, int nranks);
/* Test transport: `nranks` graphs in ONE process (one host thread each, same GPU) that share
 * `group_key` reduce through host memory in rank order instead of RCCL. Same sharding, same
 * call sequence as g2ohip_set_comm; used to test the sharded path on a single-GPU box. A `group_key` starting with
 * "solo:" makes this graph play rank `rank` of `nranks` ALONE with every collective a no-op: the kernels rank `rank`
 * would run, for timing (tools/dist_rank_times.py); its results are not meaningful. */
int g2ohip_set_comm_local(g2ohip_graph* g, const char* group_key, int rank, int nranks);
/* RCCL transport self-test on one device (a one-rank communicator from `uid`): the product's allreduce sum and max
 * (the calls g2ohip_set_comm's ranks make) over n doubles of `in` on a stream of `device`; out (2n doubles) =
 * [sum | max]. A one-GPU box cannot host two ranks of one RCCL communicator, so this is the binding's smoke test there. */
int g2ohip_comm_selftest(int device, const unsigned char uid[128], int n, const double* in, double* out);
/* As g2ohip_comm_selftest, plus the in-place reduce-scatter sum the distributed factorization uses: rs_out (n doubles)
 * = this rank's segment, and the in-place all-gather of its root exchange (checked internally: an error if the
 * rank's own segment changes). (0.1.x wrote the segment as a third block of `out`; 0.2 restored the 2n contract.) */
int g2ohip_comm_selftest_rs(int device, const unsigned char uid[128], int n, const double* in, double* out,
                            double* rs_out);
/* The test transport's rank-ordered host reduction alone (no GPU): `nranks` host threads that share `group_key` each
 * call this with their buffer; every call is checked to be the same collective on every rank (call number, length,
 * operation) and a mismatch returns G2OHIP_ERR_DEVICE on every rank (g2ohip_last_error says which) instead of reading
 * past a buffer. RCCL ranks run the same check when G2OHIP_COMM_CHECK=1 is set. */
int g2ohip_comm_local_reduce_host(const char* group_key, int rank, int nranks, double* buf, long long n, int is_max);
/* JSON text naming the HIP runtime and RCCL libraries this library's calls are bound to (resolved paths) and their
 * versions; returns the length needed including the NUL. */
int g2ohip_runtime_info(char* out, int cap);
/* hipDeviceSynchronize on `device` in this library's HIP runtime (the benchmark's bracket around its timed region). */
int g2ohip_device_synchronize(int device);

/* ---- host-only symbolic analysis (no GPU needed) ----
 * Block pattern of a symmetric matrix given as upper blocks (bi[k] <= bj[k]) of a uniform block
 * size bdim: returns n = nblocks*bdim, fills perm[n] (new -> old scalar) and
 * stats[5] = {nnz(L), factor flops, #supernodes, #levels, level-synchronous 32-column panel steps}. */
int g2ohip_symbolic_analyze(int nblocks, int bdim, int nblk, const int* bi, const int* bj, int* perm, double* stats);
/* The supernodes of the same analysis: per supernode (elimination order) its scalar columns ns, the scalar rows nr
 * below its diagonal block (the front is (ns + nr) square) and its level (leaves 0). Each array is optional and holds
 * `cap` entries; returns the number of supernodes. */
int g2ohip_symbolic_supernodes(int nblocks, int bdim, int nblk, const int* bi, const int* bj, int* ns, int* nr,
                               int* level, int cap);
/* Host-only: the distributed factorization's cut for `nranks` landmark shards of the same block pattern (DESIGN.md §6,
 * the model the solver's setup runs; flags: 1 the input is reduce-scattered by subtree ownership, 2 the landmark shards
 * are aligned with the cut; pose_work, optional: per pose block the seconds of landmark-sharded work that follow it).
 * out[14] = {distributed (the cut beats the replicated model), this rank's subtrees s, shared top s, replicated
 * iteration s (factorization + whole-S all-reduce + uniform sharded work), exchanges s (root all-gather + x
 * all-reduce), input s, replicated input s, slowest rank's subtrees s, root all-gather doubles per rank, input
 * reduce-scatter doubles per rank, input tail all-reduce doubles, supernodes, busiest rank's sharded work s, uniform
 * sharded work s}; sn_owner (cap entries, optional): per supernode its rank, -1 shared. Returns the supernodes. */
int g2ohip_dist_plan(int nblocks, int bdim, int nblk, const int* bi, const int* bj, int nranks, int rank,
                     int flags, const double* pose_work, double* out, int* sn_owner, int cap);

/* ---- measurement hooks ---- */
void g2ohip_enable_kernel_timing(g2ohip_graph* g, int on);
/* restrict the kernel timer to one kernel class (NULL or "": every class); each timed class costs two
 * event records per launch on the stream */
void g2ohip_kernel_timing_only(g2ohip_graph* g, const char* name);
/* G2OBatchStatistics timers: 0 none, 1 timeLinearSolution only (2 events per LM trial), 2 (default)
 * every stage (timeSchurComplement, timeNumericDecomposition, timeLinearSolver, timeUpdate, timeQuadraticForm) */
void g2ohip_set_stats_level(g2ohip_graph* g, int level);
/* per-kernel-class average device time (ms) since the timer was enabled; classes: "linearize", "linearize_unary"
 * (the unary edge groups' launches, timed apart from the binary groups'), "vreduce",
 * "schur_dinv", "schur_diag", "schur_rows", "chol_factor", "chol_solve", "backsub", "error", "oplus" */
double g2ohip_kernel_ms(g2ohip_graph* g, const char* name);
long long g2ohip_kernel_count(g2ohip_graph* g, const char* name);
/* algorithmic bytes / flops of one launch of the named kernel class (for roofline accounting) */
double g2ohip_kernel_bytes(g2ohip_graph* g, const char* name);
double g2ohip_kernel_flops(g2ohip_graph* g, const char* name);
/* development builds (-DG2OHIP_PHASES) only: per-launch phase stamps of the Cholesky kernels,
 * 8 x u64 per record {kernel id, t0, t1..t6}; returns the record count (0 in product builds) */
int g2ohip_debug_phases(unsigned long long* out, int max_records);
const char* g2ohip_last_error(void);
/* Measured roofline peaks of `device` (peaks.hip, ~1 s): out[0] HBM streaming-copy GB/s (read + written bytes of a
 * 2 GiB 16-byte-per-lane copy), out[1] FP64 MFMA TFLOP/s (v_mfma_f64_16x16x4f64 issue loop), out[2] FP64 VALU TFLOP/s (v_fma_f64
 * issue loop), out[3] compute units; n >= 4. Returns 4 or a negative error. */
int g2ohip_measure_peaks(int device, double* out, int n);
/* The accepted LM trial's lambda factor max(1/3, min(2/3, 1 - (2 rho - 1)^3)) exactly as the device decision and the
 * host loop compute it (optimization_algorithm_levenberg.cpp:127-136; the cube rounded once, like glibc's pow). */
double g2ohip_lm_scale_factor(double rho);
/* The two scalar decisions of a dogleg trial exactly as the device kernels take them (one shared function each).
 * step choice and blend of :153-175: hdl = coef[0] * hsd + coef[1] * hgn. Inputs: |hgn|, |hsd|, hsd.hsd,
 * c = hsd.(hgn - hsd), |hgn - hsd|^2, delta. Returns the step type (1 SD, 2 GN, 3 DL). Both beta branches
 * (c <= 0 and c > 0) exactly as written in the reference. */
int g2ohip_dogleg_blend(double hgn_norm, double hsd_norm, double hsd_sq, double c, double bma_sq, double delta,
                        double coef[2]);
/* trust-region update of :199-203 */
double g2ohip_dogleg_next_delta(double delta, double rho, double hdl_norm);
const char* g2ohip_version(void);

#ifdef __cplusplus
}
#endif
#endif
