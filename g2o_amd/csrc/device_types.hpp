// Device-side vertex/edge math for the three edge families on the BlockSolver path.
//
//   EdgeSE3ProjectXYZ  types/sba/types_six_dof_expmap.h:201-229, .cpp:395-455
//   EdgeStereoSE3ProjectXYZ  types/sba/types_six_dof_expmap.h:262-290, .cpp:457-464, 495-541
//   EdgeSE3 (QUAT)     types/slam3d/edge_se3.cpp:77-103, isometry3d_gradients.h:194-260
//   EdgeSE2            types/slam2d/edge_se2.h:46-52, edge_se2.cpp:77-103
//   EdgeSE2PointXY     types/slam2d/edge_se2_pointxy.h:41-75, edge_se2_pointxy.cpp:63-87
//   EdgeSE3PointXYZ, ...Depth, ...Disparity  types/slam3d/edge_se3_pointxyz.cpp:100-135 and its two siblings
//   EdgeSE3Expmap      types/sba/types_six_dof_expmap.h:117-124, .cpp:278-293, slam3d/se3quat.h:99-130, 173-210, 259-268
//   EdgeSE3ProjectXYZOnlyPose, EdgeStereoSE3ProjectXYZOnlyPose  types_six_dof_expmap.h:242-246, 303-307, .cpp:569-665
//   EdgeSE3Offset      types/slam3d/edge_se3_offset.cpp:102-132, isometry3d_gradients.h:84-189 (the Pi / Pj overload)
//   EdgeSE2Offset      types/slam2d/edge_se2_offset.cpp:102-106, parameter_se2_offset.cpp:76-86 (no analytic Jacobian)
//   EdgeSE2PointXYBearing  types/slam2d/edge_se2_pointxy_bearing.h:43-50 (no analytic Jacobian)
//   Edge_V_V_GICP      types/icp/types_icp.h:161-238, types_icp.cpp:49-57, 163-203
//   EdgeSim3, EdgeSim3ProjectXYZ, EdgeInverseSim3ProjectXYZ  types/sim3/types_seven_dof_expmap.h:110-180, sim3.h
//   unary priors       types/slam2d/edge_se2_prior.h:39-77, edge_se2_xyprior.h:39-71, edge_xy_prior.h,
//                      types/slam3d/edge_se3_prior.cpp:89-102 (isometry3d_gradients.h:265-325), edge_xyz_prior.cpp:63-70
//   oplus             types_six_dof_expmap.h:97-100 (SE3Quat::exp * T, se3quat.h:217-257),
//                      types_sba.h:149-153, vertex_se3.h:105-113, vertex_se2.h:51-58
//
// State layouts in HBM (fp64):
//   SE3Quat camera  [8]  tx ty tz qx qy qz qw pad     (one 64-B line per camera)
//   XYZ point       [3]
//   Isometry3 pose  [12] R (row-major 3x3) tx ty tz
//   SE2 pose        [3]  x y theta
//   XY point        [2]
// Jacobians are produced row-major (D x dim) in registers; nothing is stored.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace g2ohip {
namespace dev {

#define DI __device__ __forceinline__

DI void quat_to_R(double qx, double qy, double qz, double qw, double* R) {  // row-major
  const double tx = 2 * qx, ty = 2 * qy, tz = 2 * qz;
  const double twx = tx * qw, twy = ty * qw, twz = tz * qw;
  const double txx = tx * qx, txy = ty * qx, txz = tz * qx;
  const double tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
  R[0] = 1 - (tyy + tzz); R[1] = txy - twz;       R[2] = txz + twy;
  R[3] = txy + twz;       R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy;       R[7] = tyz + twx;       R[8] = 1 - (txx + tyy);
}

// quaternion (x,y,z,w) from a rotation matrix (row-major), Eigen's branch structure
DI void R_to_quat(const double* R, double* q) {
  double t = R[0] + R[4] + R[8];
  if (t > 0) {
    t = sqrt(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (R[7] - R[5]) * t;
    q[1] = (R[2] - R[6]) * t;
    q[2] = (R[3] - R[1]) * t;
  } else {
    int i = 0;
    if (R[4] > R[0]) i = 1;
    if (R[8] > R[i * 4]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = sqrt(R[i * 4] - R[j * 4] - R[k * 4] + 1.0);
    double c[3];
    c[i] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (R[k * 3 + j] - R[j * 3 + k]) * t;
    c[j] = (R[j * 3 + i] + R[i * 3 + j]) * t;
    c[k] = (R[k * 3 + i] + R[i * 3 + k]) * t;
    q[0] = c[0]; q[1] = c[1]; q[2] = c[2];
  }
}

DI void qrot(const double* q, const double* v, double* out) {  // q = (x,y,z,w)
  double uv0 = q[1] * v[2] - q[2] * v[1];
  double uv1 = q[2] * v[0] - q[0] * v[2];
  double uv2 = q[0] * v[1] - q[1] * v[0];
  uv0 += uv0; uv1 += uv1; uv2 += uv2;
  out[0] = v[0] + q[3] * uv0 + (q[1] * uv2 - q[2] * uv1);
  out[1] = v[1] + q[3] * uv1 + (q[2] * uv0 - q[0] * uv2);
  out[2] = v[2] + q[3] * uv2 + (q[0] * uv1 - q[1] * uv0);
}

DI void qmul(const double* a, const double* b, double* o) {  // (x,y,z,w)
  o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
  o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  o[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
  o[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
}

DI void qnormalize_pos(double* q) {  // SE3Quat::normalizeRotation
  if (q[3] < 0) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  q[0] /= n; q[1] /= n; q[2] /= n; q[3] /= n;
}

DI void mat3mul(const double* A, const double* B, double* C) {  // row-major
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}

// ---------------------------------------------------------------- SE3Quat exp (se3quat.h:217-257)
DI void se3_exp(const double* u, double* q, double* t) {
  const double w0 = u[0], w1 = u[1], w2 = u[2];
  const double theta = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
  // Omega = skew(omega) row-major
  const double Om[9] = {0, -w2, w1, w2, 0, -w0, -w1, w0, 0};
  double Om2[9];
  mat3mul(Om, Om, Om2);
  double a, b, c, d;  // R = I + a Om + b Om2 ; V = I + c Om + d Om2
  if (theta < 0.00001) {
    a = 1.0; b = 0.5; c = 0.5; d = 1.0 / 6.0;
  } else {
    const double s = sin(theta), co = cos(theta);
    a = s / theta;
    b = (1 - co) / (theta * theta);
    c = (1 - co) / (theta * theta);
    d = (theta - s) / (theta * theta * theta);
  }
  double R[9], V[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const double I = (k % 4 == 0) ? 1.0 : 0.0;
    R[k] = I + a * Om[k] + b * Om2[k];
    V[k] = I + c * Om[k] + d * Om2[k];
  }
  R_to_quat(R, q);
  t[0] = V[0] * u[3] + V[1] * u[4] + V[2] * u[5];
  t[1] = V[3] * u[3] + V[4] * u[4] + V[5] * u[5];
  t[2] = V[6] * u[3] + V[7] * u[4] + V[8] * u[5];
  qnormalize_pos(q);
}

// ---------------------------------------------------------------- Isometry helpers
DI void iso_inv(const double* X, double* Y) {  // X = [R(9) t(3)]
  Y[0] = X[0]; Y[1] = X[3]; Y[2] = X[6];
  Y[3] = X[1]; Y[4] = X[4]; Y[5] = X[7];
  Y[6] = X[2]; Y[7] = X[5]; Y[8] = X[8];
  Y[9] = -(Y[0] * X[9] + Y[1] * X[10] + Y[2] * X[11]);
  Y[10] = -(Y[3] * X[9] + Y[4] * X[10] + Y[5] * X[11]);
  Y[11] = -(Y[6] * X[9] + Y[7] * X[10] + Y[8] * X[11]);
}
DI void iso_mul(const double* A, const double* B, double* C) {
  mat3mul(A, B, C);
#pragma unroll
  for (int i = 0; i < 3; ++i) C[9 + i] = A[i * 3] * B[9] + A[i * 3 + 1] * B[10] + A[i * 3 + 2] * B[11] + A[9 + i];
}
// toCompactQuaternion (isometry3d_mappings.cpp:80-85): normalized, w >= 0
DI void compact_quat(const double* R, double* v) {
  double q[4];
  R_to_quat(R, q);
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  double s = 1.0 / n;
  if (q[3] < 0) s = -s;
  v[0] = q[0] / n * (q[3] < 0 ? -1.0 : 1.0);
  v[1] = q[1] / n * (q[3] < 0 ? -1.0 : 1.0);
  v[2] = q[2] / n * (q[3] < 0 ? -1.0 : 1.0);
  (void)s;
}

// dq/dR for the (x,y,z) of the w>=0 quaternion, column-major entries of R (dquat2mat.cpp:63-86).
// Rr is row-major; out[3][9].
DI void dq_dR(const double* Rr, double* out) {
  const double r00 = Rr[0], r01 = Rr[1], r02 = Rr[2];
  const double r10 = Rr[3], r11 = Rr[4], r12 = Rr[5];
  const double r20 = Rr[6], r21 = Rr[7], r22 = Rr[8];
  enum { I00 = 0, I10 = 1, I20 = 2, I01 = 3, I11 = 4, I21 = 5, I02 = 6, I12 = 7, I22 = 8 };
#pragma unroll
  for (int i = 0; i < 27; ++i) out[i] = 0.0;
  const double tr = r00 + r11 + r22;
  double qw;
  if (tr > 0) {
    const double S = sqrt(tr + 1.0) * 2;
    qw = 0.25 * S;
    const double iw = 1.0 / qw, iw3 = iw * iw * iw;
    const double a0 = r21 - r12, a1 = r02 - r20, a2 = r10 - r01;
    const double d0 = -0.03125 * a0 * iw3, d1 = -0.03125 * a1 * iw3, d2 = -0.03125 * a2 * iw3;
    out[I00] = d0; out[I11] = d0; out[I22] = d0;
    out[9 + I00] = d1; out[9 + I11] = d1; out[9 + I22] = d1;
    out[18 + I00] = d2; out[18 + I11] = d2; out[18 + I22] = d2;
    out[I21] = 0.25 * iw; out[I12] = -0.25 * iw;
    out[9 + I02] = 0.25 * iw; out[9 + I20] = -0.25 * iw;
    out[18 + I10] = 0.25 * iw; out[18 + I01] = -0.25 * iw;
  } else if ((r00 > r11) & (r00 > r22)) {
    const double S = sqrt(1.0 + r00 - r11 - r22) * 2;
    qw = (r21 - r12) / S;
    const double ix = 1.0 / (0.25 * S), ix3 = ix * ix * ix;
    const double sg[3] = {1.0, -1.0, -1.0};
    const int dg[3] = {I00, I11, I22};
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      out[dg[m]] = sg[m] * 0.125 * ix;
      out[9 + dg[m]] = -0.03125 * (r01 + r10) * sg[m] * ix3;
      out[18 + dg[m]] = -0.03125 * (r02 + r20) * sg[m] * ix3;
    }
    out[9 + I01] = 0.25 * ix; out[9 + I10] = 0.25 * ix;
    out[18 + I02] = 0.25 * ix; out[18 + I20] = 0.25 * ix;
  } else if (r11 > r22) {
    const double S = sqrt(1.0 + r11 - r00 - r22) * 2;
    qw = (r02 - r20) / S;
    const double iy = 1.0 / (0.25 * S), iy3 = iy * iy * iy;
    const double sg[3] = {-1.0, 1.0, -1.0};
    const int dg[3] = {I00, I11, I22};
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      out[9 + dg[m]] = sg[m] * 0.125 * iy;
      out[dg[m]] = -0.03125 * (r01 + r10) * sg[m] * iy3;
      out[18 + dg[m]] = -0.03125 * (r12 + r21) * sg[m] * iy3;
    }
    out[I01] = 0.25 * iy; out[I10] = 0.25 * iy;
    out[18 + I12] = 0.25 * iy; out[18 + I21] = 0.25 * iy;
  } else {
    const double S = sqrt(1.0 + r22 - r00 - r11) * 2;
    qw = (r10 - r01) / S;
    const double iz = 1.0 / (0.25 * S), iz3 = iz * iz * iz;
    const double sg[3] = {-1.0, -1.0, 1.0};
    const int dg[3] = {I00, I11, I22};
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      out[18 + dg[m]] = sg[m] * 0.125 * iz;
      out[dg[m]] = -0.03125 * (r02 + r20) * sg[m] * iz3;
      out[9 + dg[m]] = -0.03125 * (r12 + r21) * sg[m] * iz3;
    }
    out[I02] = 0.25 * iz; out[I20] = 0.25 * iz;
    out[9 + I12] = 0.25 * iz; out[9 + I21] = 0.25 * iz;
  }
  if (qw <= 0) {
#pragma unroll
    for (int i = 0; i < 27; ++i) out[i] = -out[i];
  }
}

DI double normalize_theta(double theta) {  // stuff/misc.h:114-127
  const double pi = 3.14159265358979323846;
  if (theta >= -pi && theta < pi) return theta;
  const double m = floor(theta / (2 * pi));
  theta = theta - m * 2 * pi;
  if (theta >= pi) theta -= 2 * pi;
  if (theta < -pi) theta += 2 * pi;
  return theta;
}

// ================================================================ edge families
// Each family: D (error dim), DI_/DJ (vertex dims), meas/info loads, error, Jacobians.

struct EdgeData {
  const int* v0;            // local index of vertex 0 (in its type's state array)
  const int* v1;
  const double* meas;       // per-edge measurement payload (family-specific stride; host-J: e | Ji | Jj)
  const double* info;       // packed upper information (family-specific stride)
  const double* params;     // BA intrinsics [4] (stereo: [5], + bf), slam3d inverse offset [12] (+ fx fy cx cy) or nullptr
  const double* s0;         // state array of vertex-0 type
  const double* s1;         // state array of vertex-1 type
  int rk;                   // robust kernel of the edge set (G2OHIP_RK_*), 0 none
  double rk_delta;          // RobustKernel::delta
  int ue = 0;               // uniform records: bit 0 one information record for every edge, bit 1 one intrinsics record;
                            // bit 2: the Edge_V_V_GICP set is plane-to-plane (params = cov0 | cov1, Omega from the state)
};
// an edge's packed information / intrinsics record (a single shared record when the edge group's are all equal)
DI const double* info_rec(const EdgeData& d, int e, int stride) {
  return d.info + ((d.ue & 1) ? 0 : (size_t)e * stride);
}
DI const double* param_rec(const EdgeData& d, int e, int stride) {
  return d.params + ((d.ue & 2) ? 0 : (size_t)e * stride);
}

// RobustKernel*::robustify (robust_kernel_impl.cpp:65-200): rho[0] = rho(e2), rho[1] = rho'(e2) (rho'' is not
// used on this path: base_edge.h:117-123 builds the weighted information from rho' only)
DI void robustify(int kind, double delta, double e2, double& r0, double& r1) {
  switch (kind) {
    case 1: {  // Huber
      const double dsqr = delta * delta;
      if (e2 <= dsqr) { r0 = e2; r1 = 1.0; }
      else { const double sq = sqrt(e2); r0 = 2 * sq * delta - dsqr; r1 = delta / sq; }
      break;
    }
    case 2: {  // PseudoHuber
      const double dsqr = delta * delta, aux1 = (1. / dsqr) * e2 + 1.0, aux2 = sqrt(aux1);
      r0 = 2 * dsqr * (aux2 - 1);
      r1 = 1. / aux2;
      break;
    }
    case 3: {  // Cauchy
      const double dsqr = delta * delta, aux = (1. / dsqr) * e2 + 1.0;
      r0 = dsqr * log(aux);
      r1 = 1. / aux;
      break;
    }
    case 4: {  // GemanMcClure
      const double aux = delta / (delta + e2);
      r0 = e2 * aux;
      r1 = aux * aux;
      break;
    }
    case 5: {  // Welsch
      const double dsqr = delta * delta, aux2 = exp(-(e2 / dsqr));
      r0 = dsqr * (1. - aux2);
      r1 = aux2;
      break;
    }
    case 6: {  // Fair
      const double aux = sqrt(e2) / delta;
      r0 = 2. * delta * delta * (aux - log(1. + aux));
      r1 = 1. / (1. + aux);
      break;
    }
    case 7: {  // Tukey
      const double e = sqrt(e2), delta2 = delta * delta;
      if (e <= delta) {
        const double aux = 1. - e2 / delta2;
        r0 = delta2 * (1. - aux * aux * aux) / 3.;
        r1 = aux * aux;
      } else {
        r0 = delta2 / 3.;
        r1 = 0;
      }
      break;
    }
    case 8: {  // Saturated
      const double dsqr = delta * delta;
      if (e2 <= dsqr) { r0 = e2; r1 = 1.; }
      else { r0 = dsqr; r1 = 0.; }
      break;
    }
    case 9: {  // DCS (delta = phi)
      double scale = (2.0 * delta) / (delta + e2);
      if (scale >= 1.0) scale = 1.0;
      r0 = scale * e2 * scale;
      r1 = scale * scale;
      break;
    }
    default: r0 = e2; r1 = 1.0; break;
  }
}

DI int up_idx(int r, int c) { return c * (c + 1) / 2 + r; }  // packed upper, r <= c

template <int D>
DI void load_info(const double* p, double* Om) {  // packed upper -> full row-major
  int k = 0;
#pragma unroll
  for (int c = 0; c < D; ++c)
#pragma unroll
    for (int r = 0; r <= c; ++r) {
      const double v = p[k++];
      Om[r * D + c] = v;
      Om[c * D + r] = v;
    }
}

// The information of an edge, full row-major. A family whose information depends on the state (Edge_V_V_GICP in
// plane-to-plane mode) forms it in F::information(d, e, Om); every other family reads its packed record. Every kernel
// that needs a binary or unary family's Omega takes it from here.
template <class F, class = void>
struct has_information : std::false_type {};
template <class F>
struct has_information<F, std::void_t<decltype(&F::information)>> : std::true_type {};
template <class F>
DI void family_info(const EdgeData& d, int e, double* Om) {
  if constexpr (has_information<F>::value) F::information(d, e, Om);
  else load_info<F::D>(info_rec(d, e, F::INFO), Om);
}

// Eigen's fixed-size 3x3 inverse (compute_inverse_size3: cofactors over the determinant expanded along column 0), as
// k_schur_prep restates it; a and out row-major
DI void inv3_cofactor(const double* a, double* out) {
  auto m = [&](int r, int c) { return a[r * 3 + c]; };
  const double c00 = m(1, 1) * m(2, 2) - m(1, 2) * m(2, 1);
  const double c10 = m(0, 2) * m(2, 1) - m(0, 1) * m(2, 2);
  const double c20 = m(0, 1) * m(1, 2) - m(0, 2) * m(1, 1);
  const double det = c00 * m(0, 0) + c10 * m(1, 0) + c20 * m(2, 0);
  const double inv = 1.0 / det;
  out[0] = c00 * inv; out[1] = c10 * inv; out[2] = c20 * inv;
  out[3] = (m(1, 2) * m(2, 0) - m(1, 0) * m(2, 2)) * inv;
  out[4] = (m(0, 0) * m(2, 2) - m(0, 2) * m(2, 0)) * inv;
  out[5] = (m(0, 2) * m(1, 0) - m(0, 0) * m(1, 2)) * inv;
  out[6] = (m(1, 0) * m(2, 1) - m(1, 1) * m(2, 0)) * inv;
  out[7] = (m(0, 1) * m(2, 0) - m(0, 0) * m(2, 1)) * inv;
  out[8] = (m(0, 0) * m(1, 1) - m(0, 1) * m(1, 0)) * inv;
}

// ---- EdgeSE3ProjectXYZ: v0 = point (3), v1 = camera SE3Quat (6) ----
struct FamilyBA {
  static constexpr int D = 2, DA = 3, DB = 6, MEAS = 2, INFO = 3, PAR = 4;
  static constexpr int SA = 8 /*unused*/, S0 = 3, S1 = 8;  // state strides
  // the error, and the point's z in the camera frame (isDepthPositive, types_six_dof_expmap.h:218-222)
  DI static double depth(const EdgeData& d, int e, double* err) {
    const double* c = d.s1 + (size_t)d.v1[e] * 8;
    const double* p = d.s0 + (size_t)d.v0[e] * 3;
    double pc[3];
    const double q[4] = {c[3], c[4], c[5], c[6]};
    const double pv[3] = {p[0], p[1], p[2]};
    qrot(q, pv, pc);
    pc[0] += c[0]; pc[1] += c[1]; pc[2] += c[2];
    const double* K = param_rec(d, e, 4);
    err[0] = d.meas[(size_t)e * 2 + 0] - (pc[0] / pc[2] * K[0] + K[2]);
    err[1] = d.meas[(size_t)e * 2 + 1] - (pc[1] / pc[2] * K[1] + K[3]);
    return pc[2];
  }
  DI static void error(const EdgeData& d, int e, double* err) { depth(d, e, err); }
  DI static void linearize(const EdgeData& d, int e, double* err, double* A, double* B) {
    double pc[3];
    linearize(d, e, err, A, B, pc);
  }
  // ... and the point in the camera frame (x, y, z): the camera Jacobian is B = diag(fx, fy) Bt(x/z, y/z, 1/z)
  DI static void linearize(const EdgeData& d, int e, double* err, double* A, double* B, double* pc) {
    linearize_at(d, e, d.v0[e], d.v1[e], err, A, B, pc);
  }
  // the same with the edge's vertex indices given (a caller that prefetched them: no dependent index load); NT: the
  // measurement (streamed once per pass) is read nontemporally, so it does not push the reused landmark lines out of L2
  template <bool NT = false>
  DI static void linearize_at(const EdgeData& d, int e, int v0, int v1, double* err, double* A, double* B, double* pc) {
    const double* c = d.s1 + (size_t)v1 * 8;
    const double* p = d.s0 + (size_t)v0 * 3;
    const double q[4] = {c[3], c[4], c[5], c[6]};
    const double pv[3] = {p[0], p[1], p[2]};
    qrot(q, pv, pc);
    pc[0] += c[0]; pc[1] += c[1]; pc[2] += c[2];
    const double* K = param_rec(d, e, 4);
    const double fx = K[0], fy = K[1];
    const double x = pc[0], y = pc[1], z = pc[2], z2 = z * z;
    const double m0 = NT ? __builtin_nontemporal_load(d.meas + (size_t)e * 2) : d.meas[(size_t)e * 2 + 0];
    const double m1 = NT ? __builtin_nontemporal_load(d.meas + (size_t)e * 2 + 1) : d.meas[(size_t)e * 2 + 1];
    err[0] = m0 - (x / z * fx + K[2]);
    err[1] = m1 - (y / z * fy + K[3]);
    double R[9];
    quat_to_R(q[0], q[1], q[2], q[3], R);
    const double iz = -1. / z;
    const double t00 = iz * fx, t02 = iz * (-x / z * fx);
    const double t11 = iz * fy, t12 = iz * (-y / z * fy);
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) {
      A[cc] = t00 * R[cc] + t02 * R[6 + cc];
      A[3 + cc] = t11 * R[3 + cc] + t12 * R[6 + cc];
    }
    B[0] = x * y / z2 * fx;
    B[1] = -(1 + (x * x / z2)) * fx;
    B[2] = y / z * fx;
    B[3] = -1. / z * fx;
    B[4] = 0;
    B[5] = x / z2 * fx;
    B[6] = (1 + y * y / z2) * fy;
    B[7] = -x * y / z2 * fy;
    B[8] = -x / z * fy;
    B[9] = 0;
    B[10] = -1. / z * fy;
    B[11] = y / z2 * fy;
  }
};

// ---- EdgeStereoSE3ProjectXYZ: v0 = point (3), v1 = camera SE3Quat (6); meas u_l v u_r, info packed upper 6,
// intrinsics fx fy cx cy bf (stride 5) ----
// UVU: EdgeProjectXYZ2UVU on a CameraParameters (types_six_dof_expmap.h:178-198): meas u v u_r, the record
// f f cx cy b (the host expands focal_length cx cy baseline). Its error is stereocam_uvu_map's, all doubles. The
// reference has no linearizeOplus for it (commented out, types_six_dof_expmap.h:196) and differentiates numerically;
// here the Jacobians are the exact first derivatives: rows 0-1 EdgeProjectXYZ2UV's analytic forms
// (types_six_dof_expmap.cpp:295-333), row 2 = -(f/z, 0, -f (x - b)/z^2) applied to R (point) and to [-[pc]x | I]
// (camera, (omega, upsilon) order), which is the stereo edge's row 2 with bf = f * b.
template <bool UVU>
struct FamilyStereoT {
  static constexpr int D = 3, DA = 3, DB = 6, MEAS = 3, INFO = 6, PAR = 5;
  static constexpr int S0 = 3, S1 = 8;  // state strides
  // the point in the camera frame (SE3Quat::map)
  DI static void to_camera(const EdgeData& d, int v0, int v1, double* q, double* pc) {
    const double* c = d.s1 + (size_t)v1 * 8;
    const double* p = d.s0 + (size_t)v0 * 3;
    q[0] = c[3]; q[1] = c[4]; q[2] = c[5]; q[3] = c[6];
    const double pv[3] = {p[0], p[1], p[2]};
    qrot(q, pv, pc);
    pc[0] += c[0]; pc[1] += c[1]; pc[2] += c[2];
  }
  // obs - cam_project (types_six_dof_expmap.cpp:457-464), in its operation order. cam_project takes bf as
  // `const float&` (types_six_dof_expmap.h:287): the error sees bf rounded to float, the Jacobians the double.
  // No contraction here: the projection rounds as the reference's does, operation by operation.
  DI static void residual(const double* K, const double* pc, double m0, double m1, double m2, double* err) {
#pragma clang fp contract(off)
    if constexpr (UVU) {  // obs - stereocam_uvu_map (types_six_dof_expmap.cpp:74-87): no float bf, (x - b) / z * f + cx
      const double u = pc[0] / pc[2] * K[0] + K[2];
      const double v = pc[1] / pc[2] * K[1] + K[3];
      const double ur = (pc[0] - K[4]) / pc[2] * K[0] + K[2];
      err[0] = m0 - u;
      err[1] = m1 - v;
      err[2] = m2 - ur;
    } else {
      const double invz = 1.0 / pc[2];
      const double bf_f = (double)(float)K[4];
      const double u = pc[0] * invz * K[0] + K[2];
      const double v = pc[1] * invz * K[1] + K[3];
      const double ur = u - bf_f * invz;
      err[0] = m0 - u;
      err[1] = m1 - v;
      err[2] = m2 - ur;
    }
  }
  // the factor of row 2's baseline terms: bf as given, or f * b of the CameraParameters record
  DI static double bf_of(const double* K) { return UVU ? K[0] * K[4] : K[4]; }
  // the error, and the point's z in the camera frame (isDepthPositive, types_six_dof_expmap.h:279-283)
  DI static double depth(const EdgeData& d, int e, double* err) {
    double q[4], pc[3];
    to_camera(d, d.v0[e], d.v1[e], q, pc);
    const double* m = d.meas + (size_t)e * 3;
    residual(param_rec(d, e, PAR), pc, m[0], m[1], m[2], err);
    return pc[2];
  }
  DI static void error(const EdgeData& d, int e, double* err) { depth(d, e, err); }
  DI static void linearize(const EdgeData& d, int e, double* err, double* A, double* B) {
    double pc[3];
    linearize(d, e, err, A, B, pc);
  }
  DI static void linearize(const EdgeData& d, int e, double* err, double* A, double* B, double* pc) {
    linearize_at(d, e, d.v0[e], d.v1[e], err, A, B, pc);
  }
  // the edge's vertex indices given; NT: the measurement is read nontemporally (as FamilyBA::linearize_at)
  template <bool NT = false>
  DI static void linearize_at(const EdgeData& d, int e, int v0, int v1, double* err, double* A, double* B, double* pc) {
    double q[4];
    to_camera(d, v0, v1, q, pc);
    const double* K = param_rec(d, e, PAR);
    const double* mp = d.meas + (size_t)e * 3;
    const double m0 = NT ? __builtin_nontemporal_load(mp) : mp[0];
    const double m1 = NT ? __builtin_nontemporal_load(mp + 1) : mp[1];
    const double m2 = NT ? __builtin_nontemporal_load(mp + 2) : mp[2];
    residual(K, pc, m0, m1, m2, err);
    const double fx = K[0], fy = K[1], bf = bf_of(K);
    const double x = pc[0], y = pc[1], z = pc[2], z_2 = z * z;
    double R[9];
    quat_to_R(q[0], q[1], q[2], q[3], R);
    // linearizeOplus, types_six_dof_expmap.cpp:509-540, in its expression forms
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) {
      A[cc] = -fx * R[cc] / z + fx * x * R[6 + cc] / z_2;
      A[3 + cc] = -fy * R[3 + cc] / z + fy * y * R[6 + cc] / z_2;
      A[6 + cc] = A[cc] - bf * R[6 + cc] / z_2;
    }
    B[0] = x * y / z_2 * fx;
    B[1] = -(1 + (x * x / z_2)) * fx;
    B[2] = y / z * fx;
    B[3] = -1. / z * fx;
    B[4] = 0;
    B[5] = x / z_2 * fx;
    B[6] = (1 + y * y / z_2) * fy;
    B[7] = -x * y / z_2 * fy;
    B[8] = -x / z * fy;
    B[9] = 0;
    B[10] = -1. / z * fy;
    B[11] = y / z_2 * fy;
    B[12] = B[0] - bf * y / z_2;
    B[13] = B[1] + bf * x / z_2;
    B[14] = B[2];
    B[15] = B[3];
    B[16] = 0;
    B[17] = B[5] - bf / z_2;
  }
};
using FamilyStereo = FamilyStereoT<false>;
using FamilyUVU = FamilyStereoT<true>;

// ---- EdgeSE3 (Isometry3): meas payload = Zinv [12], info packed upper 21 ----
struct FamilySE3 {
  static constexpr int D = 6, DA = 6, DB = 6, MEAS = 12, INFO = 21, PAR = 0;
  DI static void error(const EdgeData& d, int e, double* err) {
    const double* Xi = d.s0 + (size_t)d.v0[e] * 12;
    const double* Xj = d.s1 + (size_t)d.v1[e] * 12;
    const double* Zi = d.meas + (size_t)e * 12;
    double Xii[12], T[12], E[12], a[12], b[12], z[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) { a[k] = Xi[k]; b[k] = Xj[k]; z[k] = Zi[k]; }
    iso_inv(a, Xii);
    iso_mul(z, Xii, T);
    iso_mul(T, b, E);
    err[0] = E[9]; err[1] = E[10]; err[2] = E[11];
    compact_quat(E, err + 3);
  }
  DI static void linearize(const EdgeData& d, int e, double* err, double* Ji, double* Jj) {
    const double* Xi = d.s0 + (size_t)d.v0[e] * 12;
    const double* Xj = d.s1 + (size_t)d.v1[e] * 12;
    const double* Zi = d.meas + (size_t)e * 12;
    double a[12], b[12], A[12], Xii[12], Bm[12], E[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) { a[k] = Xi[k]; b[k] = Xj[k]; A[k] = Zi[k]; }
    {  // error exactly as computeError (association (Zinv*Xi^-1)*Xj)
      double T[12], Ee[12];
      iso_inv(a, Xii);
      iso_mul(A, Xii, T);
      iso_mul(T, b, Ee);
      err[0] = Ee[9]; err[1] = Ee[10]; err[2] = Ee[11];
      compact_quat(Ee, err + 3);
    }
    iso_mul(Xii, b, Bm);  // B = Xi^-1 Xj
    iso_mul(A, Bm, E);    // E = A B
    const double* Re = E;
    const double* Ra = A;
    const double* Rb = Bm;
    double dq[27];
    dq_dR(Re, dq);
#pragma unroll
    for (int k = 0; k < 36; ++k) { Ji[k] = 0; Jj[k] = 0; }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        Ji[r * 6 + c] = -Ra[r * 3 + c];
        Jj[r * 6 + c] = Re[r * 3 + c];
      }
    {  // dte/dqi = Ra * skewT(tb)
      const double X = 2 * Bm[9], Y = 2 * Bm[10], Z = 2 * Bm[11];
      const double S[9] = {0, -Z, Y, Z, 0, -X, -Y, X, 0};
      double M[9];
      mat3mul(Ra, S, M);
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) Ji[r * 6 + 3 + c] = M[r * 3 + c];
    }
    // dre/dqi = dq * [vec(Ra*Sxt) vec(Ra*Syt) vec(Ra*Szt)], skewT of Rb
    {
      const double r11 = 2 * Rb[0], r12 = 2 * Rb[1], r13 = 2 * Rb[2];
      const double r21 = 2 * Rb[3], r22 = 2 * Rb[4], r23 = 2 * Rb[5];
      const double r31 = 2 * Rb[6], r32 = 2 * Rb[7], r33 = 2 * Rb[8];
      const double Sx[9] = {0, 0, 0, r31, r32, r33, -r21, -r22, -r23};
      const double Sy[9] = {-r31, -r32, -r33, 0, 0, 0, r11, r12, r13};
      const double Sz[9] = {r21, r22, r23, -r11, -r12, -r13, 0, 0, 0};
      double Mx[9], My[9], Mz[9];
      mat3mul(Ra, Sx, Mx);
      mat3mul(Ra, Sy, My);
      mat3mul(Ra, Sz, Mz);
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        double s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
        for (int k = 0; k < 9; ++k) {  // k: column-major index of the 3x3 -> (k%3, k/3)
          const int rr = k % 3, cc = k / 3;
          s0 += dq[r * 9 + k] * Mx[rr * 3 + cc];
          s1 += dq[r * 9 + k] * My[rr * 3 + cc];
          s2 += dq[r * 9 + k] * Mz[rr * 3 + cc];
        }
        Ji[(3 + r) * 6 + 3] = s0; Ji[(3 + r) * 6 + 4] = s1; Ji[(3 + r) * 6 + 5] = s2;
      }
    }
    // dre/dqj = dq * [vec(Re*Sx) ...] with skew(I) (non-transposed form, entries 2)
    {
      const double Sx[9] = {0, 0, 0, 0, 0, -2, 0, 2, 0};
      const double Sy[9] = {0, 0, 2, 0, 0, 0, -2, 0, 0};
      const double Sz[9] = {0, -2, 0, 2, 0, 0, 0, 0, 0};
      double Mx[9], My[9], Mz[9];
      mat3mul(Re, Sx, Mx);
      mat3mul(Re, Sy, My);
      mat3mul(Re, Sz, Mz);
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        double s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          const int rr = k % 3, cc = k / 3;
          s0 += dq[r * 9 + k] * Mx[rr * 3 + cc];
          s1 += dq[r * 9 + k] * My[rr * 3 + cc];
          s2 += dq[r * 9 + k] * Mz[rr * 3 + cc];
        }
        Jj[(3 + r) * 6 + 3] = s0; Jj[(3 + r) * 6 + 4] = s1; Jj[(3 + r) * 6 + 5] = s2;
      }
    }
  }
};

// ---- EdgeSE2: meas payload = inverse measurement (x y theta), info packed 6 ----
struct FamilySE2 {
  static constexpr int D = 3, DA = 3, DB = 3, MEAS = 3, INFO = 6, PAR = 0;
  DI static void compose(const double* a, const double* b, double* o) {
    const double c = cos(a[2]), s = sin(a[2]);
    o[0] = a[0] + (c * b[0] - s * b[1]);
    o[1] = a[1] + (s * b[0] + c * b[1]);
    o[2] = normalize_theta(a[2] + b[2]);
  }
  DI static void inverse(const double* a, double* o) {
    o[2] = normalize_theta(-a[2]);
    const double c = cos(o[2]), s = sin(o[2]);
    o[0] = c * (-a[0]) - s * (-a[1]);
    o[1] = s * (-a[0]) + c * (-a[1]);
  }
  DI static void error(const EdgeData& d, int e, double* err) {
    const double* xi = d.s0 + (size_t)d.v0[e] * 3;
    const double* xj = d.s1 + (size_t)d.v1[e] * 3;
    const double* mi = d.meas + (size_t)e * 3;
    double a[3] = {xi[0], xi[1], xi[2]}, b[3] = {xj[0], xj[1], xj[2]}, m[3] = {mi[0], mi[1], mi[2]};
    double ai[3], t[3];
    inverse(a, ai);
    compose(ai, b, t);
    compose(m, t, err);
  }
  DI static void linearize(const EdgeData& d, int e, double* err, double* Ji, double* Jj) {
    error(d, e, err);
    const double* xi = d.s0 + (size_t)d.v0[e] * 3;
    const double* xj = d.s1 + (size_t)d.v1[e] * 3;
    const double* mi = d.meas + (size_t)e * 3;
    const double thetai = xi[2];
    const double dtx = xj[0] - xi[0], dty = xj[1] - xi[1];
    const double si = sin(thetai), ci = cos(thetai);
    const double A[9] = {-ci, -si, -si * dtx + ci * dty, si, -ci, -ci * dtx - si * dty, 0, 0, -1};
    const double B[9] = {ci, si, 0, -si, ci, 0, 0, 0, 1};
    const double rc = cos(mi[2]), rs = sin(mi[2]);
    const double Z[9] = {rc, -rs, 0, rs, rc, 0, 0, 0, 1};
    mat3mul(Z, A, Ji);
    mat3mul(Z, B, Jj);
  }
};

// ---- EdgeSE2PointXY (BlockSolver_3_2 landmark edge): v0 = SE2 pose (3), v1 = XY point (2); meas x y, info packed 3.
// error = v0^-1 * l - z (edge_se2_pointxy.h:44-49, SE2::inverse se2.h:82-87, SE2 * Vector2 = t + R v se2.h:77-80),
// Jacobians edge_se2_pointxy.cpp:63-87 ----
struct FamilySE2XY {
  static constexpr int D = 2, DA = 3, DB = 2, MEAS = 2, INFO = 3, PAR = 0;
  DI static void error(const EdgeData& d, int e, double* err) {
    const double* xi = d.s0 + (size_t)d.v0[e] * 3;
    const double* l = d.s1 + (size_t)d.v1[e] * 2;
    const double* m = d.meas + (size_t)e * 2;
    const double a[3] = {xi[0], xi[1], xi[2]};
    double ai[3];
    FamilySE2::inverse(a, ai);
    const double c = cos(ai[2]), s = sin(ai[2]), l0 = l[0], l1 = l[1];
    err[0] = (ai[0] + (c * l0 - s * l1)) - m[0];
    err[1] = (ai[1] + (s * l0 + c * l1)) - m[1];
  }
  DI static void linearize(const EdgeData& d, int e, double* err, double* Ji, double* Jj) {
    error(d, e, err);
    const double* xi = d.s0 + (size_t)d.v0[e] * 3;
    const double* l = d.s1 + (size_t)d.v1[e] * 2;
    const double x1 = xi[0], y1 = xi[1], x2 = l[0], y2 = l[1];
    const double c = cos(xi[2]), s = sin(xi[2]);
    Ji[0] = -c;
    Ji[1] = -s;
    Ji[2] = c * y2 - c * y1 - s * x2 + s * x1;
    Ji[3] = s;
    Ji[4] = -c;
    Ji[5] = -s * y2 + s * y1 - c * x2 + c * x1;
    Jj[0] = c;
    Jj[1] = s;
    Jj[2] = -s;
    Jj[3] = c;
  }
};

// ---- slam3d landmark edges: v0 = VertexSE3 pose (Isometry3 [12], dim 6), v1 = point (3); meas 3, info packed 6.
//   EdgeSE3PointXYZ           types/slam3d/edge_se3_pointxyz.cpp:100-135            meas x y z (sensor frame)
//   EdgeSE3PointXYZDepth      types/slam3d/edge_se3_pointxyz_depth.cpp:91-138       meas u v depth
//   EdgeSE3PointXYZDisparity  types/slam3d/edge_se3_pointxyz_disparity.cpp          meas u v 1/depth
// With X = (R, t) the pose, P = (Rp, tp) the sensor offset and p the point: Zc = R^T (p - t) (the cache's w2l),
// pn = Rp^T (Zc - tp) (w2n). Under VertexSE3's oplus X * (dt, dq), rotation ~ I + 2 [dq]x,
//   d Zc = [ -I | 2 [Zc]x | R^T ] (dt, dq, dp)   (3 x 9, the last three columns the point's).
// XYZ: e = pn - z, J = Rp^T dZc. Depth: pi = K pn, e = (pi.x / pi.z, pi.y / pi.z, pi.z) - z; with J' = K Rp^T dZc the
// rows 0-1 are (J'_01 pi.z - pi.xy J'_2) / pi.z^2 and row 2 is J'_2. Disparity: as Depth with e.z = 1 / pi.z - z.z and
// row 2 = -J'_2 / pi.z^2.
// Parameter record (params, one shared record when EdgeData::ue bit 1 is set: the usual graph has one sensor for all
// its edges): the inverse offset P^-1 as an isometry [Rp^T row-major (9) | -Rp^T tp (3)], made on the host; Depth and
// Disparity append fx fy cx cy (16 doubles). ----
enum { SLAM3D_XYZ = 0, SLAM3D_DEPTH = 1, SLAM3D_DISPARITY = 2 };
template <int MODE>
struct FamilySlam3d {
  static constexpr int D = 3, DA = 6, DB = 3, MEAS = 3, INFO = 6, PAR = MODE == SLAM3D_XYZ ? 12 : 16;
  // Zc and the sensor-frame point pn
  DI static void to_sensor(const double* X, const double* p, const double* Pi, double* Zc, double* pn) {
    const double d0 = p[0] - X[9], d1 = p[1] - X[10], d2 = p[2] - X[11];
#pragma unroll
    for (int i = 0; i < 3; ++i) Zc[i] = X[i] * d0 + X[3 + i] * d1 + X[6 + i] * d2;
#pragma unroll
    for (int i = 0; i < 3; ++i) pn[i] = Pi[i * 3] * Zc[0] + Pi[i * 3 + 1] * Zc[1] + Pi[i * 3 + 2] * Zc[2] + Pi[9 + i];
  }
  // the error from pn; pi = K pn for the camera modes (pi = pn for XYZ)
  DI static void residual(const double* Pi, const double* pn, const double* m, double* pi, double* err) {
    if (MODE == SLAM3D_XYZ) {
      pi[0] = pn[0]; pi[1] = pn[1]; pi[2] = pn[2];
      err[0] = pn[0] - m[0]; err[1] = pn[1] - m[1]; err[2] = pn[2] - m[2];
    } else {
      const double fx = Pi[12], fy = Pi[13], cx = Pi[14], cy = Pi[15];
      pi[0] = fx * pn[0] + cx * pn[2];
      pi[1] = fy * pn[1] + cy * pn[2];
      pi[2] = pn[2];
      err[0] = pi[0] / pi[2] - m[0];
      err[1] = pi[1] / pi[2] - m[1];
      err[2] = (MODE == SLAM3D_DEPTH ? pi[2] : 1.0 / pi[2]) - m[2];
    }
  }
  DI static void error(const EdgeData& d, int e, double* err) {
    const double* x = d.s0 + (size_t)d.v0[e] * 12;
    const double* pt = d.s1 + (size_t)d.v1[e] * 3;
    const double* Pi = param_rec(d, e, PAR);
    const double* mp = d.meas + (size_t)e * 3;
    double X[12], Zc[3], pn[3], pi[3];
#pragma unroll
    for (int k = 0; k < 12; ++k) X[k] = x[k];
    const double p[3] = {pt[0], pt[1], pt[2]}, m[3] = {mp[0], mp[1], mp[2]};
    to_sensor(X, p, Pi, Zc, pn);
    residual(Pi, pn, m, pi, err);
  }
  DI static void linearize(const EdgeData& d, int e, double* err, double* Ji, double* Jj) {
    const double* x = d.s0 + (size_t)d.v0[e] * 12;
    const double* pt = d.s1 + (size_t)d.v1[e] * 3;
    const double* Pi = param_rec(d, e, PAR);
    const double* mp = d.meas + (size_t)e * 3;
    double X[12], Zc[3], pn[3], pi[3];
#pragma unroll
    for (int k = 0; k < 12; ++k) X[k] = x[k];
    const double p[3] = {pt[0], pt[1], pt[2]}, m[3] = {mp[0], mp[1], mp[2]};
    to_sensor(X, p, Pi, Zc, pn);
    residual(Pi, pn, m, pi, err);
    // M = Rp^T (XYZ) or K Rp^T (camera modes), then J' = M [ -I | 2 [Zc]x | R^T ]
    double M[9];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (MODE == SLAM3D_XYZ) {
        M[c] = Pi[c]; M[3 + c] = Pi[3 + c];
      } else {
        M[c] = Pi[12] * Pi[c] + Pi[14] * Pi[6 + c];
        M[3 + c] = Pi[13] * Pi[3 + c] + Pi[15] * Pi[6 + c];
      }
      M[6 + c] = Pi[6 + c];
    }
    double Jp[27];  // 3 x 9 row-major
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const double m0 = M[r * 3], m1 = M[r * 3 + 1], m2 = M[r * 3 + 2];
      Jp[r * 9 + 0] = -m0; Jp[r * 9 + 1] = -m1; Jp[r * 9 + 2] = -m2;
      Jp[r * 9 + 3] = 2 * (m1 * Zc[2] - m2 * Zc[1]);  // row of M times [Zc]x = m x Zc
      Jp[r * 9 + 4] = 2 * (m2 * Zc[0] - m0 * Zc[2]);
      Jp[r * 9 + 5] = 2 * (m0 * Zc[1] - m1 * Zc[0]);
#pragma unroll
      for (int c = 0; c < 3; ++c) Jp[r * 9 + 6 + c] = m0 * X[c * 3] + m1 * X[c * 3 + 1] + m2 * X[c * 3 + 2];
    }
    if (MODE != SLAM3D_XYZ) {
      const double iz2 = 1.0 / (pi[2] * pi[2]);
#pragma unroll
      for (int c = 0; c < 9; ++c) {
        const double j2 = Jp[18 + c];
        Jp[c] = iz2 * (Jp[c] * pi[2] - pi[0] * j2);
        Jp[9 + c] = iz2 * (Jp[9 + c] * pi[2] - pi[1] * j2);
        if (MODE == SLAM3D_DISPARITY) Jp[18 + c] = -j2 * iz2;
      }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 6; ++c) Ji[r * 6 + c] = Jp[r * 9 + c];
#pragma unroll
      for (int c = 0; c < 3; ++c) Jj[r * 3 + c] = Jp[r * 9 + 6 + c];
    }
  }
};
using FamilySE3XYZ = FamilySlam3d<SLAM3D_XYZ>;
using FamilySE3XYZDepth = FamilySlam3d<SLAM3D_DEPTH>;
using FamilySE3XYZDisparity = FamilySlam3d<SLAM3D_DISPARITY>;

// ---- EdgeProjectP2MC / EdgeProjectP2SC (types_sba.h:173-250, types_sba.cpp:249-403): v0 = point (3), v1 = VertexCam,
// an SBACam (sbacam.h:55-175): the camera-to-world pose and the intrinsics in one state record of 12 doubles
//   tx ty tz qx qy qz qw fx fy cx cy baseline
// pc = R^T (pw - t); e = (fx pc.x / pc.z + cx - u, fy pc.y / pc.z + cy - v), projected minus measured; the stereo row
// e2 = fx (pc.x - b) / pc.z + cx - u_r. Under SBACam::update (t += dt, q = q * (dq, sqrt(1 - |dq|^2))) a derivative dp
// of pc gives the rows (pc.z dp.x - pc.x dp.z) fx / pc.z^2, (pc.z dp.y - pc.y dp.z) fy / pc.z^2 and, stereo,
// (pc.z dp.x - (pc.x - b) dp.z) fx / pc.z^2, with dp = column k of R^T for the point, its negative for the camera
// translation and (dRi_k R^T)(pw - t) = dRi_k pc for the camera rotation: dRi_k = -2 [e_k]x, so the three rotation
// columns are 2 (pc x e_k) = (0, 2 pc.z, -2 pc.y), (-2 pc.z, 0, 2 pc.x), (2 pc.y, -2 pc.x, 0). R^T is built once per
// edge; there is no parameter record and no depth test (the reference types have no isDepthPositive). ----
template <bool STEREO>
struct FamilySBA {
  static constexpr int D = STEREO ? 3 : 2, DA = 3, DB = 6, MEAS = D, INFO = D * (D + 1) / 2, PAR = 0;
  static constexpr int S0 = 3, S1 = 12;  // state strides
  // pc = R^T (pw - t); Rt = R^T row-major
  DI static void to_camera(const double* c, const double* p, double* Rt, double* pc) {
    double R[9];
    quat_to_R(c[3], c[4], c[5], c[6], R);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) Rt[i * 3 + j] = R[j * 3 + i];
    const double d0 = p[0] - c[0], d1 = p[1] - c[1], d2 = p[2] - c[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) pc[i] = Rt[i * 3] * d0 + Rt[i * 3 + 1] * d1 + Rt[i * 3 + 2] * d2;
  }
  DI static void residual(const double* c, const double* pc, const double* m, double* err) {
    const double iz = 1.0 / pc[2];
    err[0] = c[7] * pc[0] * iz + c[9] - m[0];
    err[1] = c[8] * pc[1] * iz + c[10] - m[1];
    if (STEREO) err[2] = c[7] * (pc[0] - c[11]) * iz + c[9] - m[2];
  }
  DI static void error(const EdgeData& d, int e, double* err) {
    const double* cp = d.s1 + (size_t)d.v1[e] * 12;
    const double* pp = d.s0 + (size_t)d.v0[e] * 3;
    const double* mp = d.meas + (size_t)e * MEAS;
    double c[12], m[MEAS], Rt[9], pc[3];
#pragma unroll
    for (int k = 0; k < 12; ++k) c[k] = cp[k];
#pragma unroll
    for (int k = 0; k < MEAS; ++k) m[k] = mp[k];
    const double p[3] = {pp[0], pp[1], pp[2]};
    to_camera(c, p, Rt, pc);
    residual(c, pc, m, err);
  }
  DI static void linearize(const EdgeData& d, int e, double* err, double* A, double* B) {
    linearize_at(d, e, d.v0[e], d.v1[e], err, A, B);
  }
  // A (D x 3): the point's Jacobian; B (D x 6): the camera's
  DI static void linearize_at(const EdgeData& d, int e, int v0, int v1, double* err, double* A, double* B) {
    const double* cp = d.s1 + (size_t)v1 * 12;
    const double* pp = d.s0 + (size_t)v0 * 3;
    const double* mp = d.meas + (size_t)e * MEAS;
    double c[12], m[MEAS], Rt[9], pc[3];
#pragma unroll
    for (int k = 0; k < 12; ++k) c[k] = cp[k];
#pragma unroll
    for (int k = 0; k < MEAS; ++k) m[k] = mp[k];
    const double p[3] = {pp[0], pp[1], pp[2]};
    to_camera(c, p, Rt, pc);
    residual(c, pc, m, err);
    const double ipz2 = 1.0 / (pc[2] * pc[2]);
    const double fx2 = ipz2 * c[7], fy2 = ipz2 * c[8];
    const double xs = pc[0] - c[11];  // stereo row numerator
#pragma unroll
    for (int k = 0; k < 3; ++k) {  // dp = column k of R^T; the translation columns are its negative
      const double dx = Rt[k], dy = Rt[3 + k], dz = Rt[6 + k];
      A[k] = (pc[2] * dx - pc[0] * dz) * fx2;
      A[3 + k] = (pc[2] * dy - pc[1] * dz) * fy2;
      if (STEREO) A[6 + k] = (pc[2] * dx - xs * dz) * fx2;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      B[k] = -A[k];
      B[6 + k] = -A[3 + k];
      if (STEREO) B[12 + k] = -A[6 + k];
    }
    // rotation columns: dp_x = (0, 2 z, -2 y), dp_y = (-2 z, 0, 2 x), dp_z = (2 y, -2 x, 0)
    const double x2 = 2 * pc[0], y2 = 2 * pc[1], z2 = 2 * pc[2];
    const double rx[3] = {0.0, -z2, y2}, ry[3] = {z2, 0.0, -x2}, rz[3] = {-y2, x2, 0.0};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      B[3 + k] = (pc[2] * rx[k] - pc[0] * rz[k]) * fx2;
      B[9 + k] = (pc[2] * ry[k] - pc[1] * rz[k]) * fy2;
      if (STEREO) B[15 + k] = (pc[2] * rx[k] - xs * rz[k]) * fx2;
    }
  }
};
using FamilySBAMono = FamilySBA<false>;
using FamilySBAStereo = FamilySBA<true>;

// ---- EdgeSE3Offset (types/slam3d/edge_se3_offset.cpp:102-132, CacheSE3Offset::updateImpl parameter_se3_offset.cpp,
// isometry3d_gradients.h:84-189): a pose constraint between the sensor frames Xi Pi and Xj Pj. meas payload = Z^-1 [12]
// (as FamilySE3), info packed upper 21, parameter record [Pi (12) | Pj (12)], both isometries made on the host (one
// shared record when EdgeData::ue bit 1 is set). error = toVectorMQT((Z^-1 * w2n_i) * n2w_j) with n2w = X P and
// w2n = n2w^-1, computeError's association. Jacobians: the Pi / Pj overload of computeEdgeSE3Gradient, its
// non-__clang__ branch (Ra * Sxt, Ra * Syt, Ra * Szt; the __clang__ branch multiplies Sxt by Rab), which is what
// FamilySE3 restates for identity offsets. With A = Z^-1 Pi^-1, B = Xi^-1 Xj, C = Pj, E = A B C:
//   dte/dti = -Ra, dte/dtj = Rab, dte/dqi = Ra skewT(t_bc), dte/dqj = Rab skew(t_c),
//   dre/dqi = dq_dR(Re) [Ra skewT(Rbc)], dre/dqj = dq_dR(Re) [Rab skew(Rc)].
// The work is ordered so that the temporaries of one part are dead before the next starts: the error first, then the
// translation rows, then the rotation rows, which alone need dq_dR. ----
struct FamilySE3Offset {
  static constexpr int D = 6, DA = 6, DB = 6, MEAS = 12, INFO = 21, PAR = 24;
  // the record of a group whose records are all equal is read at a wave-uniform address (scalar loads where the
  // compiler takes them)
  DI static void load_par(const EdgeData& d, int e, double* Pi, double* Pj) {
    if (d.ue & 2) {
#pragma unroll
      for (int k = 0; k < 12; ++k) { Pi[k] = d.params[k]; Pj[k] = d.params[12 + k]; }
    } else {
      const double* p = d.params + (size_t)e * PAR;
#pragma unroll
      for (int k = 0; k < 12; ++k) { Pi[k] = p[k]; Pj[k] = p[12 + k]; }
    }
  }
  DI static void load(const EdgeData& d, int e, double* Xi, double* Xj, double* Zi) {
    const double* xi = d.s0 + (size_t)d.v0[e] * 12;
    const double* xj = d.s1 + (size_t)d.v1[e] * 12;
    const double* zi = d.meas + (size_t)e * 12;
#pragma unroll
    for (int k = 0; k < 12; ++k) { Xi[k] = xi[k]; Xj[k] = xj[k]; Zi[k] = zi[k]; }
  }
  DI static void error_of(const double* Xi, const double* Xj, const double* Zi, const double* Pi, const double* Pj,
                          double* err) {
    double N[12], W[12], T[12];
    iso_mul(Xi, Pi, N);  // n2w_i
    iso_inv(N, W);       // w2n_i
    iso_mul(Zi, W, T);
    iso_mul(Xj, Pj, N);  // n2w_j
    iso_mul(T, N, W);    // delta
    err[0] = W[9]; err[1] = W[10]; err[2] = W[11];
    compact_quat(W, err + 3);
  }
  DI static void error(const EdgeData& d, int e, double* err) {
    double Xi[12], Xj[12], Zi[12], Pi[12], Pj[12];
    load(d, e, Xi, Xj, Zi);
    load_par(d, e, Pi, Pj);
    error_of(Xi, Xj, Zi, Pi, Pj, err);
  }
  DI static void linearize(const EdgeData& d, int e, double* err, double* Ji, double* Jj) {
    double Xi[12], Xj[12], A[12], Pi[12], Pj[12];  // A holds Z^-1 until the error is done
    load(d, e, Xi, Xj, A);
    load_par(d, e, Pi, Pj);
    error_of(Xi, Xj, A, Pi, Pj, err);
    double AB[12], BC[12];
    {
      double T[12], B[12];
      iso_inv(Pi, T);
      iso_mul(A, T, B);
#pragma unroll
      for (int k = 0; k < 12; ++k) A[k] = B[k];  // A = Z^-1 Pi^-1
      iso_inv(Xi, T);
      iso_mul(T, Xj, B);  // B = Xi^-1 Xj
      iso_mul(A, B, AB);
      iso_mul(B, Pj, BC);
    }
    const double* Ra = A;
    const double* Rab = AB;
#pragma unroll
    for (int k = 0; k < 36; ++k) { Ji[k] = 0; Jj[k] = 0; }
    // ---- translation rows
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        Ji[r * 6 + c] = -Ra[r * 3 + c];
        Jj[r * 6 + c] = Rab[r * 3 + c];
      }
    {  // dte/dqi = Ra * skewT(t_bc)
      const double X = 2 * BC[9], Y = 2 * BC[10], Z = 2 * BC[11];
      const double S[9] = {0, -Z, Y, Z, 0, -X, -Y, X, 0};
      double M[9];
      mat3mul(Ra, S, M);
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) Ji[r * 6 + 3 + c] = M[r * 3 + c];
    }
    {  // dte/dqj = Rab * skew(t_c)
      const double x = 2 * Pj[9], y = 2 * Pj[10], z = 2 * Pj[11];
      const double S[9] = {0, z, -y, -z, 0, x, y, -x, 0};
      double M[9];
      mat3mul(Rab, S, M);
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) Jj[r * 6 + 3 + c] = M[r * 3 + c];
    }
    // ---- rotation rows
    double dq[27];
    {
      double Re[9];
      mat3mul(Rab, Pj, Re);  // E = AB C
      dq_dR(Re, dq);
    }
    {  // dre/dqi = dq * [vec(Ra*Sxt) vec(Ra*Syt) vec(Ra*Szt)], skewT of Rbc
      const double r11 = 2 * BC[0], r12 = 2 * BC[1], r13 = 2 * BC[2];
      const double r21 = 2 * BC[3], r22 = 2 * BC[4], r23 = 2 * BC[5];
      const double r31 = 2 * BC[6], r32 = 2 * BC[7], r33 = 2 * BC[8];
      const double Sx[9] = {0, 0, 0, r31, r32, r33, -r21, -r22, -r23};
      const double Sy[9] = {-r31, -r32, -r33, 0, 0, 0, r11, r12, r13};
      const double Sz[9] = {r21, r22, r23, -r11, -r12, -r13, 0, 0, 0};
      double Mx[9], My[9], Mz[9];
      mat3mul(Ra, Sx, Mx);
      mat3mul(Ra, Sy, My);
      mat3mul(Ra, Sz, Mz);
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        double s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
        for (int k = 0; k < 9; ++k) {  // k: column-major index of the 3x3 -> (k%3, k/3)
          const int rr = k % 3, cc = k / 3;
          s0 += dq[r * 9 + k] * Mx[rr * 3 + cc];
          s1 += dq[r * 9 + k] * My[rr * 3 + cc];
          s2 += dq[r * 9 + k] * Mz[rr * 3 + cc];
        }
        Ji[(3 + r) * 6 + 3] = s0; Ji[(3 + r) * 6 + 4] = s1; Ji[(3 + r) * 6 + 5] = s2;
      }
    }
    {  // dre/dqj = dq * [vec(Rab*Sx) vec(Rab*Sy) vec(Rab*Sz)], skew of Rc
      const double r11 = 2 * Pj[0], r12 = 2 * Pj[1], r13 = 2 * Pj[2];
      const double r21 = 2 * Pj[3], r22 = 2 * Pj[4], r23 = 2 * Pj[5];
      const double r31 = 2 * Pj[6], r32 = 2 * Pj[7], r33 = 2 * Pj[8];
      const double Sx[9] = {0, 0, 0, -r31, -r32, -r33, r21, r22, r23};
      const double Sy[9] = {r31, r32, r33, 0, 0, 0, -r11, -r12, -r13};
      const double Sz[9] = {-r21, -r22, -r23, r11, r12, r13, 0, 0, 0};
      double Mx[9], My[9], Mz[9];
      mat3mul(Rab, Sx, Mx);
      mat3mul(Rab, Sy, My);
      mat3mul(Rab, Sz, Mz);
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        double s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          const int rr = k % 3, cc = k / 3;
          s0 += dq[r * 9 + k] * Mx[rr * 3 + cc];
          s1 += dq[r * 9 + k] * My[rr * 3 + cc];
          s2 += dq[r * 9 + k] * Mz[rr * 3 + cc];
        }
        Jj[(3 + r) * 6 + 3] = s0; Jj[(3 + r) * 6 + 4] = s1; Jj[(3 + r) * 6 + 5] = s2;
      }
    }
  }
};

// ---- EdgeSE2Offset (types/slam2d/edge_se2_offset.cpp:102-106, CacheSE2Offset::updateImpl parameter_se2_offset.cpp:
// 76-86): meas payload = inverse measurement (x y theta, as FamilySE2), info packed 6, parameter record
// [Pi (x y theta) | Pj (x y theta)] (shared when EdgeData::ue bit 1 is set). With Ni = Xi * Pi, Nj = Xj * Pj:
// error = ((Z^-1 * Ni^-1) * Nj) as (x, y, normalised angle), computeError's association. The reference has no analytic
// Jacobian (numeric default); these are the exact ones: FamilySE2's at (Ni, Nj), each times the chain factor of
// N = X * P under VertexSE2's additive oplus, the identity with its last column (R'(theta) p, 1),
// R'(theta) = [[-s, -c], [c, -s]], p the offset's translation. Only the third column of each Jacobian changes. ----
struct FamilySE2Offset {
  static constexpr int D = 3, DA = 3, DB = 3, MEAS = 3, INFO = 6, PAR = 6;
  DI static void error(const EdgeData& d, int e, double* err) {
    double Ji[9], Jj[9];
    eval<false>(d, e, err, Ji, Jj);
  }
  DI static void linearize(const EdgeData& d, int e, double* err, double* Ji, double* Jj) {
    eval<true>(d, e, err, Ji, Jj);
  }
  template <bool JAC>
  DI static void eval(const EdgeData& d, int e, double* err, double* Ji, double* Jj) {
    const double* xi = d.s0 + (size_t)d.v0[e] * 3;
    const double* xj = d.s1 + (size_t)d.v1[e] * 3;
    const double* mi = d.meas + (size_t)e * 3;
    const double* P = param_rec(d, e, PAR);
    const double a[3] = {xi[0], xi[1], xi[2]}, b[3] = {xj[0], xj[1], xj[2]}, m[3] = {mi[0], mi[1], mi[2]};
    const double pi[3] = {P[0], P[1], P[2]}, pj[3] = {P[3], P[4], P[5]};
    // SE2::operator* and SE2::inverse (se2.h:60-87) spelled out: each angle's sine and cosine is taken once and
    // serves the error and the Jacobians (five pairs; through FamilySE2's helpers it would be eleven)
    const double sa = sin(a[2]), ca = cos(a[2]), sb = sin(b[2]), cb = cos(b[2]);
    const double ni[3] = {a[0] + (ca * pi[0] - sa * pi[1]), a[1] + (sa * pi[0] + ca * pi[1]), normalize_theta(a[2] + pi[2])};
    const double nj[3] = {b[0] + (cb * pj[0] - sb * pj[1]), b[1] + (sb * pj[0] + cb * pj[1]), normalize_theta(b[2] + pj[2])};
    const double si = sin(ni[2]), ci = cos(ni[2]);
    // w = Ni^-1: the angle -theta, t = R(-theta) (-t)
    const double w[3] = {ci * (-ni[0]) + si * (-ni[1]), -si * (-ni[0]) + ci * (-ni[1]), normalize_theta(-ni[2])};
    const double rc = cos(m[2]), rs = sin(m[2]);
    const double t[3] = {m[0] + (rc * w[0] - rs * w[1]), m[1] + (rs * w[0] + rc * w[1]), normalize_theta(m[2] + w[2])};
    const double st = sin(t[2]), ct = cos(t[2]);
    err[0] = t[0] + (ct * nj[0] - st * nj[1]);
    err[1] = t[1] + (st * nj[0] + ct * nj[1]);
    err[2] = normalize_theta(t[2] + nj[2]);
    if (JAC) {
      const double dtx = nj[0] - ni[0], dty = nj[1] - ni[1];
      const double A[9] = {-ci, -si, -si * dtx + ci * dty, si, -ci, -ci * dtx - si * dty, 0, 0, -1};
      const double B[9] = {ci, si, 0, -si, ci, 0, 0, 0, 1};
      const double Z[9] = {rc, -rs, 0, rs, rc, 0, 0, 0, 1};
      mat3mul(Z, A, Ji);
      mat3mul(Z, B, Jj);
      // chain factors: column 2 += columns 0-1 times R'(theta) p
      const double ui = -sa * pi[0] - ca * pi[1], vi = ca * pi[0] - sa * pi[1];
      const double uj = -sb * pj[0] - cb * pj[1], vj = cb * pj[0] - sb * pj[1];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        Ji[r * 3 + 2] += Ji[r * 3] * ui + Ji[r * 3 + 1] * vi;
        Jj[r * 3 + 2] += Jj[r * 3] * uj + Jj[r * 3 + 1] * vj;
      }
    }
  }
};

// ---- EdgeSE2PointXYBearing (types/slam2d/edge_se2_pointxy_bearing.h:43-50): v0 = SE2 pose (3), v1 = XY point (2);
// meas one angle, info one scalar, no parameter record. d = v0^-1 * l (SE2::inverse, then t + R v, as FamilySE2XY),
// error = normalize_theta(z - atan2(d.y, d.x)). The reference has no analytic Jacobian; these are the exact ones: with
// g = (-d.y, d.x) / |d|^2, Ji = [ g R(theta)^T | 1 ], Jj = -g R(theta)^T. Singular at d = 0, as the reference. ----
struct FamilySE2XYBearing {
  static constexpr int D = 1, DA = 3, DB = 2, MEAS = 1, INFO = 1, PAR = 0;
  // d = v0^-1 * l
  DI static void to_sensor(const double* xi, const double* l, double* dd) {
    const double a[3] = {xi[0], xi[1], xi[2]};
    double ai[3];
    FamilySE2::inverse(a, ai);
    const double c = cos(ai[2]), s = sin(ai[2]), l0 = l[0], l1 = l[1];
    dd[0] = ai[0] + (c * l0 - s * l1);
    dd[1] = ai[1] + (s * l0 + c * l1);
  }
  // Jj = -g R^T (1 x 2); the pose's is [-Jj | 1]
  DI static void point_jacobian(double theta, const double* dd, double* Jj) {
    const double n2 = dd[0] * dd[0] + dd[1] * dd[1];
    const double g0 = -dd[1] / n2, g1 = dd[0] / n2;
    const double c = cos(theta), s = sin(theta);
    Jj[0] = -(g0 * c - g1 * s);  // g R^T = (g0 c - g1 s, g0 s + g1 c)
    Jj[1] = -(g0 * s + g1 * c);
  }
  DI static void error(const EdgeData& d, int e, double* err) {
    double dd[2];
    to_sensor(d.s0 + (size_t)d.v0[e] * 3, d.s1 + (size_t)d.v1[e] * 2, dd);
    err[0] = normalize_theta(d.meas[e] - atan2(dd[1], dd[0]));
  }
  DI static void linearize(const EdgeData& d, int e, double* err, double* Ji, double* Jj) {
    const double* xi = d.s0 + (size_t)d.v0[e] * 3;
    double dd[2];
    to_sensor(xi, d.s1 + (size_t)d.v1[e] * 2, dd);
    err[0] = normalize_theta(d.meas[e] - atan2(dd[1], dd[0]));
    point_jacobian(xi[2], dd, Jj);
    Ji[0] = -Jj[0];
    Ji[1] = -Jj[1];
    Ji[2] = 1.0;
  }
};

// ---- Edge_V_V_GICP (types/icp/types_icp.h:161-238, types_icp.cpp:163-203): two VertexSE3 (Isometry3 states). meas
// payload = pos0 | pos1 [6] (the normals stay on the host), info packed upper 6 (the point-to-plane information).
// error = T0^-1 * (T1 * pos1) - pos0 in computeError's association. The reference's analytic Jacobians
// (GICP_ANALYTIC_JACOBIANS): Ji = [-I | dRidx p1t, dRidy p1t, dRidz p1t] with p1t = (T0^-1 T1) pos1,
// Jj = [R01 | R01 dRidx^T pos1, R01 dRidy^T pos1, R01 dRidz^T pos1] with R01 = R0^T R1; the three constant matrices
// (types_icp.cpp:49-57, antisymmetric with entries +-2) are written out as their products with a vector.
// Plane-to-plane (EdgeData::ue bit 2, the whole edge set; the reference keeps pl_pl per edge): the parameter record is
// cov0 | cov1, each packed upper 6, and Omega = (cov0 + R01 cov1 R01^T)^-1 at the current state
// (types_icp.h:220-226), Eigen's 3x3 cofactor inverse. The Jacobians ignore Omega's dependence on the state, as the
// reference's do. ----
struct FamilyGICP {
  static constexpr int D = 3, DA = 6, DB = 6, MEAS = 6, INFO = 6, PAR = 12;
  // W = T0^-1 (inverse first, as Isometry3::inverse), X1 = T1
  DI static void load(const EdgeData& d, int e, double* W, double* X1) {
    const double* x0 = d.s0 + (size_t)d.v0[e] * 12;
    const double* x1 = d.s1 + (size_t)d.v1[e] * 12;
    double X0[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) { X0[k] = x0[k]; X1[k] = x1[k]; }
    iso_inv(X0, W);
  }
  DI static void apply(const double* T, const double* p, double* o) {  // linear() * p + translation()
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = T[i * 3] * p[0] + T[i * 3 + 1] * p[1] + T[i * 3 + 2] * p[2] + T[9 + i];
  }
  DI static void error_of(const EdgeData& d, int e, const double* W, const double* X1, double* p1, double* err) {
    const double* m = d.meas + (size_t)e * MEAS;
    p1[0] = m[3]; p1[1] = m[4]; p1[2] = m[5];
    double pw[3], pl[3];
    apply(X1, p1, pw);
    apply(W, pw, pl);
    err[0] = pl[0] - m[0]; err[1] = pl[1] - m[1]; err[2] = pl[2] - m[2];
  }
  DI static void error(const EdgeData& d, int e, double* err) {
    double W[12], X1[12], p1[3];
    load(d, e, W, X1);
    error_of(d, e, W, X1, p1, err);
  }
  DI static void linearize(const EdgeData& d, int e, double* err, double* Ji, double* Jj) {
    double W[12], X1[12], p1[3], T01[12], pt[3];
    load(d, e, W, X1);
    error_of(d, e, W, X1, p1, err);
    iso_mul(W, X1, T01);
    apply(T01, p1, pt);
    const double x = 2 * pt[0], y = 2 * pt[1], z = 2 * pt[2];
    // dRidx p = (0, 2 pz, -2 py), dRidy p = (-2 pz, 0, 2 px), dRidz p = (2 py, -2 px, 0)
    const double ci[9] = {0, -z, y, z, 0, -x, -y, x, 0};  // row r: (dRidx p, dRidy p, dRidz p)[r]
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        Ji[r * 6 + c] = r == c ? -1.0 : 0.0;
        Ji[r * 6 + 3 + c] = ci[r * 3 + c];
        Jj[r * 6 + c] = T01[r * 3 + c];
      }
    // dRid{x,y,z}^T pos1 = -(dRid{x,y,z} pos1): the columns of -[2 pos1]x ordered as above
    const double X = 2 * p1[0], Y = 2 * p1[1], Z = 2 * p1[2];
    const double cj[9] = {0, Z, -Y, -Z, 0, X, Y, -X, 0};
    double M[9];
    mat3mul(T01, cj, M);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) Jj[r * 6 + 3 + c] = M[r * 3 + c];
  }
  DI static void information(const EdgeData& d, int e, double* Om) {
    if (!(d.ue & 4)) {  // point-to-plane: the caller's record
      load_info<3>(info_rec(d, e, INFO), Om);
      return;
    }
    double W[12], X1[12], R[9], C0[9], C1[9], T[9], S[9];
    load(d, e, W, X1);
    mat3mul(W, X1, R);  // R01
    const double* c = param_rec(d, e, PAR);
    load_info<3>(c, C0);
    load_info<3>(c + 6, C1);
    mat3mul(R, C1, T);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j)  // cov0 + (R cov1) R^T
        S[i * 3 + j] = C0[i * 3 + j] + (T[i * 3] * R[j * 3] + T[i * 3 + 1] * R[j * 3 + 1] + T[i * 3 + 2] * R[j * 3 + 2]);
    inv3_cofactor(S, Om);
  }
};

// ---- Edge_XYZ_VSC (types/icp/types_icp.h:247-407): v0 = point (3), v1 = VertexSCam, a VertexSE3 (Isometry3 state,
// camera-to-world) whose cached w2n / w2i are recomputed here from the state. meas u v u_r, info packed upper 6, the
// parameter record fx fy cx cy baseline (VertexSCam's static Kcam and baseline; one shared record when EdgeData::ue
// bit 1 is set). error = mapPoint(point) - measurement in mapPoint's order: w2n = T^-1, w2i = Kcam w2n formed first,
// (u, v) = (w2i pt)_01 / (w2i pt)_2, u_r from Kcam (w2n pt - (b, 0, 0)). The reference differentiates numerically
// (SCAM_ANALYTIC_JACOBIANS is commented out); these are the exact first derivatives: with pc = w2n pt and P the
// projection's 3x3 derivative at pc, A = P R^T (point) and B = P [-I | 2 [pc]x] (VertexSE3's oplus: the translation,
// then the quaternion's x y z). ----
struct FamilyVSC {
  static constexpr int D = 3, DA = 3, DB = 6, MEAS = 3, INFO = 6, PAR = 5;
  // X: the camera's isometry, K: fx fy cx cy baseline, p: the point, m: the measurement
  template <bool JA, bool JB>
  DI static void core(const double* X, const double* K, const double* p, const double* m, double* err, double* A,
                      double* B) {
    double W[12];
    iso_inv(X, W);  // w2n = [R^T | -R^T t]
    const double fx = K[0], fy = K[1], cx = K[2], cy = K[3], bl = K[4];
    // w2i = Kcam * w2n, rows 0 and 1 (row 2 is w2n's)
    double I0[4], I1[4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      I0[c] = fx * W[c] + cx * W[6 + c];
      I1[c] = fy * W[3 + c] + cy * W[6 + c];
    }
    I0[3] = fx * W[9] + cx * W[11];
    I1[3] = fy * W[10] + cy * W[11];
    const double px = p[0], py = p[1], pz = p[2];
    const double p1x = I0[0] * px + I0[1] * py + I0[2] * pz + I0[3];
    const double p1y = I1[0] * px + I1[1] * py + I1[2] * pz + I1[3];
    const double x = W[0] * px + W[1] * py + W[2] * pz + W[9];
    const double y = W[3] * px + W[4] * py + W[5] * pz + W[10];
    const double z = W[6] * px + W[7] * py + W[8] * pz + W[11];
    const double invp1 = 1.0 / z;
    err[0] = p1x * invp1 - m[0];
    err[1] = p1y * invp1 - m[1];
    err[2] = (fx * (x - bl) + cx * z) / z - m[2];
    if (JA || JB) {
      const double iz2 = invp1 * invp1;
      const double P[9] = {fx * invp1, 0, -fx * x * iz2, 0, fy * invp1, -fy * y * iz2, fx * invp1, 0, -fx * (x - bl) * iz2};
      if (JA) mat3mul(P, W, A);
      if (JB) {
        const double S[9] = {0, -2 * z, 2 * y, 2 * z, 0, -2 * x, -2 * y, 2 * x, 0};  // 2 [pc]x
        double M[9];
        mat3mul(P, S, M);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            B[r * 6 + c] = -P[r * 3 + c];
            B[r * 6 + 3 + c] = M[r * 3 + c];
          }
      }
    }
  }
  template <bool JAC>
  DI static void eval(const EdgeData& d, int e, double* err, double* A, double* B) {
    const double* pp = d.s0 + (size_t)d.v0[e] * 3;
    const double* xp = d.s1 + (size_t)d.v1[e] * 12;
    const double* mp = d.meas + (size_t)e * MEAS;
    const double* Kp = param_rec(d, e, PAR);
    double X[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) X[k] = xp[k];
    const double p[3] = {pp[0], pp[1], pp[2]}, m[3] = {mp[0], mp[1], mp[2]};
    const double K[5] = {Kp[0], Kp[1], Kp[2], Kp[3], Kp[4]};
    core<JAC, JAC>(X, K, p, m, err, A, B);
  }
  DI static void error(const EdgeData& d, int e, double* err) {
    double A[9], B[18];
    eval<false>(d, e, err, A, B);
  }
  DI static void linearize(const EdgeData& d, int e, double* err, double* A, double* B) { eval<true>(d, e, err, A, B); }
};

// ---- host-Jacobian edges (an edge type the device does not know): the host's linearizeOplus
// (base_binary_edge.hpp:198-266 numeric, or the type's own analytic one) supplies, per edge, the error and
// both Jacobians row-major in the meas payload: [e (D) | Ji (D x DA) | Jj (D x DB)] ----
template <int D_, int DA_, int DB_>
struct FamilyHostJ {
  static constexpr int D = D_, DA = DA_, DB = DB_, INFO = D * (D + 1) / 2, P = D + D * DA + D * DB;
  DI static void error(const EdgeData& d, int e, double* err) {
    const double* p = d.meas + (size_t)e * P;
#pragma unroll
    for (int i = 0; i < D; ++i) err[i] = p[i];
  }
  DI static void linearize(const EdgeData& d, int e, double* err, double* A, double* B) {
    const double* p = d.meas + (size_t)e * P;
#pragma unroll
    for (int i = 0; i < D; ++i) err[i] = p[i];
#pragma unroll
    for (int i = 0; i < D * DA; ++i) A[i] = p[D + i];
#pragma unroll
    for (int i = 0; i < D * DB; ++i) B[i] = p[D + D * DA + i];
  }
};

// ================================================================ unary edge families (BaseUnaryEdge, v0 only)
// Each family: D, DA, MEAS (payload doubles per edge), INFO, error(d, e, err), linearize(d, e, err, A) with A the
// Jacobian row-major (D x DA). v1 / s1 are not read.

// ---- EdgeSE2Prior (edge_se2_prior.h:39-77): meas payload = inverse measurement (x y theta), info packed 6.
// error = (Z^-1 * x).toVector(); J = [R(Z^-1) 0; 0 1] ----
struct FamilyUnarySE2 {
  static constexpr int D = 3, DA = 3, MEAS = 3, INFO = 6, PAR = 0;
  DI static void error(const EdgeData& d, int e, double* err) {
    const double* xi = d.s0 + (size_t)d.v0[e] * 3;
    const double* mi = d.meas + (size_t)e * 3;
    const double a[3] = {xi[0], xi[1], xi[2]}, m[3] = {mi[0], mi[1], mi[2]};
    FamilySE2::compose(m, a, err);
  }
  DI static void linearize(const EdgeData& d, int e, double* err, double* A) {
    error(d, e, err);
    const double th = d.meas[(size_t)e * 3 + 2];
    const double rc = cos(th), rs = sin(th);
    A[0] = rc; A[1] = -rs; A[2] = 0;
    A[3] = rs; A[4] = rc;  A[5] = 0;
    A[6] = 0;  A[7] = 0;   A[8] = 1.;
  }
};

// ---- EdgeSE2XYPrior (edge_se2_xyprior.h:39-71, .cpp:60-63): error = translation - z, J = [I 0] ----
struct FamilyUnarySE2XY {
  static constexpr int D = 2, DA = 3, MEAS = 2, INFO = 3, PAR = 0;
  DI static void error(const EdgeData& d, int e, double* err) {
    const double* xi = d.s0 + (size_t)d.v0[e] * 3;
    const double* m = d.meas + (size_t)e * 2;
    err[0] = xi[0] - m[0];
    err[1] = xi[1] - m[1];
  }
  DI static void linearize(const EdgeData& d, int e, double* err, double* A) {
    error(d, e, err);
    A[0] = 1; A[1] = 0; A[2] = 0;
    A[3] = 0; A[4] = 1; A[5] = 0;
  }
};

// ---- EdgeXYPrior (edge_xy_prior.h, .cpp) on a VertexPointXY, EdgeXYZPrior (edge_xyz_prior.cpp:63-70) on a point:
// error = estimate - z, J = I ----
template <int N>
struct FamilyUnaryPoint {
  static constexpr int D = N, DA = N, MEAS = N, INFO = N * (N + 1) / 2, PAR = 0;
  DI static void error(const EdgeData& d, int e, double* err) {
    const double* p = d.s0 + (size_t)d.v0[e] * N;
    const double* m = d.meas + (size_t)e * N;
#pragma unroll
    for (int i = 0; i < N; ++i) err[i] = p[i] - m[i];
  }
  DI static void linearize(const EdgeData& d, int e, double* err, double* A) {
    error(d, e, err);
#pragma unroll
    for (int i = 0; i < N * N; ++i) A[i] = (i % (N + 1) == 0) ? 1.0 : 0.0;
  }
};
using FamilyUnaryXY = FamilyUnaryPoint<2>;
using FamilyUnaryXYZ = FamilyUnaryPoint<3>;

// ---- EdgeSE3Prior (edge_se3_prior.cpp:89-102): meas payload = [Z^-1 (12) | offset P (12)], info packed 21.
// error = toVectorMQT(Z^-1 * (X * P)) (the cache's n2w = X * P); Jacobian computeEdgeSE3PriorGradient
// (isometry3d_gradients.h:265-325, the gcc branch): A = Z^-1 X, B = P, E = A B ----
struct FamilyUnarySE3 {
  static constexpr int D = 6, DA = 6, MEAS = 24, INFO = 21, PAR = 0;
  DI static void load(const EdgeData& d, int e, double* X, double* Zi, double* P) {
    const double* x = d.s0 + (size_t)d.v0[e] * 12;
    const double* m = d.meas + (size_t)e * 24;
#pragma unroll
    for (int k = 0; k < 12; ++k) { X[k] = x[k]; Zi[k] = m[k]; P[k] = m[12 + k]; }
  }
  DI static void error_of(const double* X, const double* Zi, const double* P, double* err) {
    double T[12], E[12];
    iso_mul(X, P, T);
    iso_mul(Zi, T, E);
    err[0] = E[9]; err[1] = E[10]; err[2] = E[11];
    compact_quat(E, err + 3);
  }
  DI static void error(const EdgeData& d, int e, double* err) {
    double X[12], Zi[12], P[12];
    load(d, e, X, Zi, P);
    error_of(X, Zi, P, err);
  }
  DI static void linearize(const EdgeData& d, int e, double* err, double* J) {
    double X[12], Zi[12], P[12], A[12], E[12];
    load(d, e, X, Zi, P);
    error_of(X, Zi, P, err);
    iso_mul(Zi, X, A);
    iso_mul(A, P, E);
    const double* Ra = A;
    const double* Rb = P;
    double dq[27];
    dq_dR(E, dq);
#pragma unroll
    for (int k = 0; k < 36; ++k) J[k] = 0;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) J[r * 6 + c] = Ra[r * 3 + c];
    {  // dte/dq = Ra * skew(tb)
      const double x = 2 * P[9], y = 2 * P[10], z = 2 * P[11];
      const double S[9] = {0, z, -y, -z, 0, x, y, -x, 0};
      double M[9];
      mat3mul(Ra, S, M);
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) J[r * 6 + 3 + c] = M[r * 3 + c];
    }
    {  // dre/dq = dq * [vec(Ra*Sx) vec(Ra*Sy) vec(Ra*Sz)], skew of Rb
      const double r11 = 2 * Rb[0], r12 = 2 * Rb[1], r13 = 2 * Rb[2];
      const double r21 = 2 * Rb[3], r22 = 2 * Rb[4], r23 = 2 * Rb[5];
      const double r31 = 2 * Rb[6], r32 = 2 * Rb[7], r33 = 2 * Rb[8];
      const double Sx[9] = {0, 0, 0, -r31, -r32, -r33, r21, r22, r23};
      const double Sy[9] = {r31, r32, r33, 0, 0, 0, -r11, -r12, -r13};
      const double Sz[9] = {-r21, -r22, -r23, r11, r12, r13, 0, 0, 0};
      double Mx[9], My[9], Mz[9];
      mat3mul(Ra, Sx, Mx);
      mat3mul(Ra, Sy, My);
      mat3mul(Ra, Sz, Mz);
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        double s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
        for (int k = 0; k < 9; ++k) {  // k: column-major index of the 3x3 -> (k%3, k/3)
          const int rr = k % 3, cc = k / 3;
          s0 += dq[r * 9 + k] * Mx[rr * 3 + cc];
          s1 += dq[r * 9 + k] * My[rr * 3 + cc];
          s2 += dq[r * 9 + k] * Mz[rr * 3 + cc];
        }
        J[(3 + r) * 6 + 3] = s0; J[(3 + r) * 6 + 4] = s1; J[(3 + r) * 6 + 5] = s2;
      }
    }
  }
};

// ---- host-Jacobian unary edges (any other BaseUnaryEdge<D, E, V>): per edge [e (D) | Ji (D x DA)] row-major in the
// meas payload, from the host's linearizeOplus (base_unary_edge.hpp:87-129 numeric, or the type's own) ----
template <int D_, int DA_>
struct FamilyHostJUnary {
  static constexpr int D = D_, DA = DA_, INFO = D * (D + 1) / 2, P = D + D * DA, MEAS = P;
  DI static void error(const EdgeData& d, int e, double* err) {
    const double* p = d.meas + (size_t)e * P;
#pragma unroll
    for (int i = 0; i < D; ++i) err[i] = p[i];
  }
  DI static void linearize(const EdgeData& d, int e, double* err, double* A) {
    const double* p = d.meas + (size_t)e * P;
#pragma unroll
    for (int i = 0; i < D; ++i) err[i] = p[i];
#pragma unroll
    for (int i = 0; i < D * DA; ++i) A[i] = p[D + i];
  }
};

// ================================================================ the other edges on VertexSE3Expmap
// (types/sba/types_six_dof_expmap.*): EdgeSE3Expmap between two cameras, and the two pose-only projections.

// ---- SE3Quat as (q = x y z w, t) ----
// SE3Quat::inverse (se3quat.h:118-123): r' = conj(r), t' = r' * (-t); no normalisation
DI void se3q_inv(const double* q, const double* t, double* qo, double* to) {
  qo[0] = -q[0]; qo[1] = -q[1]; qo[2] = -q[2]; qo[3] = q[3];
  const double nt[3] = {t[0] * -1., t[1] * -1., t[2] * -1.};
  qrot(qo, nt, to);
}
// SE3Quat::operator* (se3quat.h:99-105): t = ta + ra * tb, r = ra * rb, then normalizeRotation (w >= 0, unit norm)
DI void se3q_mul(const double* qa, const double* ta, const double* qb, const double* tb, double* qo, double* to) {
  double rt[3];
  qrot(qa, tb, rt);
  to[0] = ta[0] + rt[0]; to[1] = ta[1] + rt[1]; to[2] = ta[2] + rt[2];
  qmul(qa, qb, qo);
  qnormalize_pos(qo);
}
// SE3Quat::log (se3quat.h:173-210): out = (omega, upsilon). Both branches: d > 0.99999 takes omega = deltaR / 2 and
// the series V^-1, otherwise acos and tan.
DI void se3q_log(const double* q, const double* t, double* out) {
  double R[9];
  quat_to_R(q[0], q[1], q[2], q[3], R);
  const double d = 0.5 * (R[0] + R[4] + R[8] - 1);
  const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
  double w[3], c;  // V^-1 = I - 0.5 Omega + c Omega^2
  if (d > 0.99999) {
    w[0] = 0.5 * dR[0]; w[1] = 0.5 * dR[1]; w[2] = 0.5 * dR[2];
    c = 1. / 12.;
  } else {
    const double theta = acos(d);
    const double s = theta / (2 * sqrt(1 - d * d));
    w[0] = s * dR[0]; w[1] = s * dR[1]; w[2] = s * dR[2];
    c = (1 - theta / (2 * tan(theta / 2))) / (theta * theta);
  }
  const double Om[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
  double Om2[9];
  mat3mul(Om, Om, Om2);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    double s = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) s += (((r == k) ? 1.0 : 0.0) - 0.5 * Om[r * 3 + k] + c * Om2[r * 3 + k]) * t[k];
    out[r] = w[r];
    out[3 + r] = s;
  }
}
// SE3Quat::adj (se3quat.h:259-268) times sgn, row-major 6 x 6: [[R, 0], [skew(t) R, R]]
DI void se3q_adj(const double* q, const double* t, double sgn, double* J) {
  double R[9];
  quat_to_R(q[0], q[1], q[2], q[3], R);
  const double S[9] = {0, -t[2], t[1], t[2], 0, -t[0], -t[1], t[0], 0};
  double SR[9];
  mat3mul(S, R, SR);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      J[r * 6 + c] = sgn * R[r * 3 + c];
      J[r * 6 + 3 + c] = 0;
      J[(3 + r) * 6 + c] = sgn * SR[r * 3 + c];
      J[(3 + r) * 6 + 3 + c] = sgn * R[r * 3 + c];
    }
}

// ---- EdgeSE3Expmap (types_six_dof_expmap.h:117-124, .cpp:278-293): v0 = Ti, v1 = Tj, both SE3Quat cameras [8];
// meas payload = the measurement C as stored [8] (tx ty tz qx qy qz qw pad), info packed upper 21.
// error = log(Tj^-1 * C * Ti) in (omega, upsilon) order; Ji = adj(Tj^-1 * C), Jj = -adj(Ti^-1 * C^-1): the reference's
// Jacobians, exact at zero error only. The error is finished before the Jacobians start, so that the temporaries of
// the log and of the two adjoints are not live together. ----
struct FamilyExpmap {
  static constexpr int D = 6, DA = 6, DB = 6, MEAS = 8, INFO = 21, PAR = 0;
  DI static void load(const double* p, double* q, double* t) {
    t[0] = p[0]; t[1] = p[1]; t[2] = p[2];
    q[0] = p[3]; q[1] = p[4]; q[2] = p[5]; q[3] = p[6];
  }
  // A = Tj^-1 * C
  DI static void invTj_C(const EdgeData& d, int e, double* qa, double* ta) {
    double qj[4], tj[3], qc[4], tc[3], qi[4], ti[3];
    load(d.s1 + (size_t)d.v1[e] * 8, qj, tj);
    load(d.meas + (size_t)e * 8, qc, tc);
    se3q_inv(qj, tj, qi, ti);
    se3q_mul(qi, ti, qc, tc, qa, ta);
  }
  DI static void error(const EdgeData& d, int e, double* err) {
    double qa[4], ta[3], qi[4], ti[3], qe[4], te[3];
    invTj_C(d, e, qa, ta);
    load(d.s0 + (size_t)d.v0[e] * 8, qi, ti);
    se3q_mul(qa, ta, qi, ti, qe, te);
    se3q_log(qe, te, err);
  }
  DI static void linearize(const EdgeData& d, int e, double* err, double* Ji, double* Jj) {
    error(d, e, err);
    {
      double qa[4], ta[3];
      invTj_C(d, e, qa, ta);
      se3q_adj(qa, ta, 1.0, Ji);
    }
    {
      double qi[4], ti[3], qc[4], tc[3], qx[4], tx[3], qy[4], ty[3], qb[4], tb[3];
      load(d.s0 + (size_t)d.v0[e] * 8, qi, ti);
      load(d.meas + (size_t)e * 8, qc, tc);
      se3q_inv(qi, ti, qx, tx);
      se3q_inv(qc, tc, qy, ty);
      se3q_mul(qx, tx, qy, ty, qb, tb);
      se3q_adj(qb, tb, -1.0, Jj);
    }
  }
};

// ================================================================ types/sim3: VertexSim3Expmap, EdgeSim3
// A similarity g = (q = x y z w, t, s) acts as x -> s R(q) x + t. State and measurement records are [8]:
// tx ty tz qx qy qz qw s (one 64-B line). Tangent vectors are (omega, upsilon, sigma).
DI void sim3_load(const double* p, double* q, double* t, double& s) {
  t[0] = p[0]; t[1] = p[1]; t[2] = p[2];
  q[0] = p[3]; q[1] = p[4]; q[2] = p[5]; q[3] = p[6];
  s = p[7];
}
// Sim3::operator* (sim3.h:255-261): r = ra * rb, t = sa (ra * tb) + ta, s = sa sb; nothing is normalised
DI void sim3_mul(const double* qa, const double* ta, double sa, const double* qb, const double* tb, double sb,
                 double* qo, double* to, double& so) {
  double rt[3];
  qrot(qa, tb, rt);
  to[0] = sa * rt[0] + ta[0]; to[1] = sa * rt[1] + ta[1]; to[2] = sa * rt[2] + ta[2];
  qmul(qa, qb, qo);
  so = sa * sb;
}
// Sim3::inverse (sim3.h:223-226): Sim3(conj r, conj r * ((-1 / s) t), 1 / s), whose constructor normalises the rotation
DI void sim3_inv(const double* q, const double* t, double s, double* qo, double* to, double& so) {
  qo[0] = -q[0]; qo[1] = -q[1]; qo[2] = -q[2]; qo[3] = q[3];
  const double f = -1 / s;
  const double v[3] = {f * t[0], f * t[1], f * t[2]};
  qrot(qo, v, to);
  so = 1 / s;
  qnormalize_pos(qo);
}
// The coefficients of W = A Omega + B Omega^2 + C I in the four branches of sim3.h:86-128 / 154-205 (|sigma| < eps or
// not, small_t: theta < eps in exp, d > 1 - eps in log). With DERIV the derivatives of each branch's own formula in
// theta and sigma: dc = A_th B_th A_s B_s C_s, zero where the branch takes a constant.
template <bool DERIV>
DI void sim3_coef(double theta, double sigma, double s, bool small_t, double& A, double& B, double& C, double* dc) {
  const double eps = 0.00001;
  if (DERIV) { dc[0] = dc[1] = dc[2] = dc[3] = dc[4] = 0; }
  if (fabs(sigma) < eps) {
    C = 1;
    if (small_t) {
      A = 1. / 2.;
      B = 1. / 6.;
    } else {
      const double theta2 = theta * theta, sn = sin(theta), cs = cos(theta);
      A = (1 - cs) / theta2;
      B = (theta - sn) / (theta2 * theta);
      if (DERIV) {
        dc[0] = sn / theta2 - 2 * A / theta;
        dc[1] = A / theta - 3 * B / theta;
      }
    }
  } else {
    C = (s - 1) / sigma;
    const double Cs = (s - C) / sigma;
    if (DERIV) dc[4] = Cs;
    const double sigma2 = sigma * sigma;
    if (small_t) {
      A = ((sigma - 1) * s + 1) / sigma2;
      B = ((0.5 * sigma2 - sigma + 1) * s - 1) / (sigma2 * sigma);
      if (DERIV) {
        dc[2] = (s - 2 * A) / sigma;
        dc[3] = (0.5 * s - 3 * B) / sigma;
      }
    } else {
      const double a = s * sin(theta), b = s * cos(theta);
      const double theta2 = theta * theta, c = theta2 + sigma2;
      A = (a * sigma + (1 - b) * theta) / (theta * c);
      const double G = ((b - 1) * sigma + a * theta) / c;
      B = (C - G) * 1 / theta2;
      if (DERIV) {
        const double itc = 1 / (theta * c), ic = 1 / c;
        dc[0] = (b * sigma + a * theta + (1 - b)) * itc - A * (c + 2 * theta2) * itc;
        dc[2] = (a + a * sigma - b * theta) * itc - A * 2 * sigma * ic;
        const double Gt = (-a * sigma + b * theta + a) * ic - G * 2 * theta * ic;
        const double Gs = (b * sigma + (b - 1) + a * theta) * ic - G * 2 * sigma * ic;
        dc[1] = -Gt / theta2 - 2 * B / theta;
        dc[3] = (Cs - Gs) / theta2;
      }
    }
  }
}
// Sim3(Vector7) (sim3.h:66-135): the exponential; R through Eigen's Quaternion(Matrix3), not normalised
DI void sim3_exp(const double* u, double* q, double* t, double& s) {
  const double w0 = u[0], w1 = u[1], w2 = u[2], sigma = u[6];
  const double theta = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
  const double Om[9] = {0, -w2, w1, w2, 0, -w0, -w1, w0, 0};
  double Om2[9];
  mat3mul(Om, Om, Om2);
  s = exp(sigma);
  const bool small_t = theta < 0.00001;
  double A, B, C;
  sim3_coef<false>(theta, sigma, s, small_t, A, B, C, nullptr);
  double ra = 1, rb = 0.5;  // R = I + ra Omega + rb Omega^2
  if (!small_t) {
    ra = sin(theta) / theta;
    rb = (1 - cos(theta)) / (theta * theta);
  }
  double R[9], W[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const double I = (k % 4 == 0) ? 1.0 : 0.0;
    R[k] = I + ra * Om[k] + rb * Om2[k];
    W[k] = A * Om[k] + B * Om2[k] + C * I;
  }
  R_to_quat(R, q);
#pragma unroll
  for (int r = 0; r < 3; ++r) t[r] = W[r * 3] * u[3] + W[r * 3 + 1] * u[4] + W[r * 3 + 2] * u[5];
}
// The pieces of M = d log(exp(d) g) / d d at 0, the first derivatives of the closed-form log below:
//   M = [[Jw, 0, 0], [Q, Wi, m], [0, 0, 1]]  (3x3 blocks row-major, m a column)
struct Sim3LogJac {
  double Jw[9], Q[9], Wi[9], m[3];
};
// Sim3::log (sim3.h:141-220) of (R = toRotationMatrix(q), t, s), all four branches: e = (omega, upsilon, sigma).
// upsilon = W^-1 t by the cofactor inverse (the reference solves by LU). With DERIV also L:
//   omega = k(d) deltaR: d deltaR / d dw = tr(R) I - R, d d / d dw = -deltaR^T / 2, so
//   Jw = k (tr(R) I - R) - k'(d) / 2 deltaR deltaR^T, k = 1 / 2 (k' = 0) or theta / (2 sin theta)
//   W upsilon = t: d upsilon = W^-1 (dt - dW upsilon), dt = [-[t]x | I | t] d, dW upsilon = P d omega + ps d sigma,
//   P = (A_th O u + B_th O^2 u) omega^T / theta - A [u]x - B ([O u]x + O [u]x), ps = A_s O u + B_s O^2 u + C_s u
//   Q = Wi (-[t]x - P Jw), m = upsilon - Wi ps
template <bool DERIV>
DI void sim3_log(const double* R, const double* t, double s, double* e, Sim3LogJac* L) {
  const double sigma = log(s);
  const double tr = R[0] + R[4] + R[8];
  const double d = 0.5 * (tr - 1);
  const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
  const bool small_t = d > 1 - 0.00001;
  double theta = 0, k = 0.5, kp = 0;
  if (!small_t) {
    theta = acos(d);
    const double sn = sqrt(1 - d * d);
    k = theta / (2 * sn);
    if (DERIV) kp = (d * theta / sn - 1) / (2 * sn * sn);
  }
  const double w[3] = {k * dR[0], k * dR[1], k * dR[2]};
  double A, B, C, dc[5];
  sim3_coef<DERIV>(theta, sigma, s, small_t, A, B, C, dc);
  const double Om[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
  double Om2[9], W[9];
  mat3mul(Om, Om, Om2);
#pragma unroll
  for (int i = 0; i < 9; ++i) W[i] = A * Om[i] + B * Om2[i] + ((i % 4 == 0) ? C : 0.0);
  double Wi_[9];
  double* Wi = DERIV ? L->Wi : Wi_;
  inv3_cofactor(W, Wi);
  double u[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) u[r] = Wi[r * 3] * t[0] + Wi[r * 3 + 1] * t[1] + Wi[r * 3 + 2] * t[2];
  e[0] = w[0]; e[1] = w[1]; e[2] = w[2];
  e[3] = u[0]; e[4] = u[1]; e[5] = u[2];
  e[6] = sigma;
  if (!DERIV) return;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      L->Jw[r * 3 + c] = k * ((r == c ? tr : 0.0) - R[r * 3 + c]) - 0.5 * kp * dR[r] * dR[c];
  double Ou[3], O2u[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) Ou[r] = Om[r * 3] * u[0] + Om[r * 3 + 1] * u[1] + Om[r * 3 + 2] * u[2];
#pragma unroll
  for (int r = 0; r < 3; ++r) O2u[r] = Om[r * 3] * Ou[0] + Om[r * 3 + 1] * Ou[1] + Om[r * 3 + 2] * Ou[2];
  const double ith = small_t ? 0.0 : 1 / theta;  // (dc[0], dc[1] are zero in the small-angle branches)
  const double Su[9] = {0, -u[2], u[1], u[2], 0, -u[0], -u[1], u[0], 0};
  const double SOu[9] = {0, -Ou[2], Ou[1], Ou[2], 0, -Ou[0], -Ou[1], Ou[0], 0};
  double OSu[9], P[9];
  mat3mul(Om, Su, OSu);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      P[r * 3 + c] = (dc[0] * Ou[r] + dc[1] * O2u[r]) * (w[c] * ith) - A * Su[r * 3 + c] -
                     B * (SOu[r * 3 + c] + OSu[r * 3 + c]);
  double PJ[9];
  mat3mul(P, L->Jw, PJ);
  const double St[9] = {0, -t[2], t[1], t[2], 0, -t[0], -t[1], t[0], 0};
#pragma unroll
  for (int i = 0; i < 9; ++i) PJ[i] = -St[i] - PJ[i];
  mat3mul(Wi, PJ, L->Q);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double ps[3] = {dc[2] * Ou[0] + dc[3] * O2u[0] + dc[4] * u[0], dc[2] * Ou[1] + dc[3] * O2u[1] + dc[4] * u[1],
                          dc[2] * Ou[2] + dc[3] * O2u[2] + dc[4] * u[2]};
    L->m[r] = u[r] - (Wi[r * 3] * ps[0] + Wi[r * 3 + 1] * ps[1] + Wi[r * 3 + 2] * ps[2]);
  }
}
// column j of M, and M^T v
DI void sim3_M_col(const Sim3LogJac& L, int j, double* c) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    c[r] = j < 3 ? L.Jw[r * 3 + (j < 3 ? j : 0)] : 0.0;
    c[3 + r] = j < 3 ? L.Q[r * 3 + (j < 3 ? j : 0)] : (j < 6 ? L.Wi[r * 3 + (j < 6 ? j - 3 : 0)] : L.m[r]);
  }
  c[6] = j == 6 ? 1.0 : 0.0;
}
// Ad(g) = [[R, 0, 0], [[t]x R, s R, -t], [0, 0, 1]] of g = (R, t, s), applied without forming it: column j, and Ad^T v
DI void sim3_ad_col(const double* R, const double* t, double s, int j, double* c) {
  if (j < 3) {
    const double r0 = R[j], r1 = R[3 + j], r2 = R[6 + j];
    c[0] = r0; c[1] = r1; c[2] = r2;
    c[3] = t[1] * r2 - t[2] * r1;
    c[4] = t[2] * r0 - t[0] * r2;
    c[5] = t[0] * r1 - t[1] * r0;
    c[6] = 0;
  } else if (j < 6) {
    c[0] = c[1] = c[2] = 0;
    c[3] = s * R[j - 3]; c[4] = s * R[3 + j - 3]; c[5] = s * R[6 + j - 3];
    c[6] = 0;
  } else {
    c[0] = c[1] = c[2] = 0;
    c[3] = -t[0]; c[4] = -t[1]; c[5] = -t[2];
    c[6] = 1;
  }
}
DI void sim3_adT_apply(const double* R, const double* t, double s, const double* v, double* o) {
  // omega: R^T (v_w - t x v_u); upsilon: s R^T v_u; sigma: v_s - t . v_u
  const double a[3] = {v[0] - (t[1] * v[5] - t[2] * v[4]), v[1] - (t[2] * v[3] - t[0] * v[5]),
                       v[2] - (t[0] * v[4] - t[1] * v[3])};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    o[c] = R[c] * a[0] + R[3 + c] * a[1] + R[6 + c] * a[2];
    o[3 + c] = s * (R[c] * v[3] + R[3 + c] * v[4] + R[6 + c] * v[5]);
  }
  o[6] = v[6] - (t[0] * v[3] + t[1] * v[4] + t[2] * v[5]);
}

// ---- EdgeSim3 (types_seven_dof_expmap.h:110-137): v0 = S0, v1 = S1, both Sim3 [8]; meas payload = the measurement C
// as stored [8] (rotation normalised, w >= 0), info packed upper 28 in (omega, upsilon, sigma) order.
// error = log(C * S0 * S1^-1). The family has no linearize(): its Jacobians Ji = M Ad(C), Jj = -M Ad(E) are never formed,
// k_linearize_sim3 (kernels.hip) builds the quadratic form from M^T Omega M and the two adjoints. EdgeData::ue bit 3:
// the vertices' _fix_scale (column 6 of both Jacobians is zero). ----
struct FamilySim3 {
  static constexpr int D = 7, DA = 7, DB = 7, MEAS = 8, INFO = 28, PAR = 0;
  // E = C * S0 * S1^-1 as (R_E, t_E, s_E); with WANT_C also C as (R_C, t_C, s_C)
  template <bool WANT_C>
  DI static void error_transform(const EdgeData& d, int e, double* RE, double* tE, double& sE, double* RC, double* tC,
                                 double& sC) {
    double qc[4], tc[3], sc, q0[4], t0[3], s0, q1[4], t1[3], s1;
    sim3_load(d.meas + (size_t)e * 8, qc, tc, sc);
    sim3_load(d.s0 + (size_t)d.v0[e] * 8, q0, t0, s0);
    sim3_load(d.s1 + (size_t)d.v1[e] * 8, q1, t1, s1);
    double qa[4], ta[3], sa, qi[4], ti[3], si, qe[4];
    sim3_mul(qc, tc, sc, q0, t0, s0, qa, ta, sa);
    sim3_inv(q1, t1, s1, qi, ti, si);
    sim3_mul(qa, ta, sa, qi, ti, si, qe, tE, sE);
    quat_to_R(qe[0], qe[1], qe[2], qe[3], RE);
    if (WANT_C) {
      quat_to_R(qc[0], qc[1], qc[2], qc[3], RC);
      tC[0] = tc[0]; tC[1] = tc[1]; tC[2] = tc[2];
      sC = sc;
    }
  }
  DI static void error(const EdgeData& d, int e, double* err) {
    double RE[9], tE[3], sE, sC;
    error_transform<false>(d, e, RE, tE, sE, nullptr, nullptr, sC);
    sim3_log<false>(RE, tE, sE, err, nullptr);
  }
};

// ---- EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ (types_seven_dof_expmap.h:141-180): v0 = the point [3], v1 = S, a
// Sim3 [8]; meas u v, info packed 3, params fx fy cx cy = camera 1 (INV: camera 2) of the edge's Sim3 vertex as the host
// holds it (one shared record when EdgeData::ue bit 1 is set). With g = S (INV: S.inverse(), the constructor's
// normalising inverse = sim3_inv) and x = g.map(p) = s (r p) + t: error = obs - (x.xy / x.z * f + c), rounded operation by
// operation as the reference's. The family has no linearize(): the point is fixed in every graph that initialises, so
// k_linearize_sim3_project (kernels.hip) takes jac_pose alone, the exact first derivatives under oplus exp(u) S with
// P = [[fx/z, 0, -fx x/z^2], [0, fy/z, -fy y/z^2]] at x and R = toRotationMatrix(q_g):
//   forward  Jj = -P [ -[x]x | I | x ]        inverse  Jj = -P s R [ [p]x | -I | -p ]
// EdgeData::ue bit 3: the vertices' _fix_scale (column 6 of Jj is zero; applied by the kernel). ----
template <bool INV>
struct FamilySim3Project {
  static constexpr int D = 2, DA = 3, DB = 7, MEAS = 2, INFO = 3, PAR = 4;
  // g as (q, s) and the mapped point x; pv: the point
  DI static void map(const EdgeData& d, int e, double* q, double& s, double* pv, double* x) {
#pragma clang fp contract(off)
    double t[3];
    if (INV) {
      double qs[4], ts[3], ss;
      sim3_load(d.s1 + (size_t)d.v1[e] * 8, qs, ts, ss);
      sim3_inv(qs, ts, ss, q, t, s);
    } else {
      sim3_load(d.s1 + (size_t)d.v1[e] * 8, q, t, s);
    }
    const double* p = d.s0 + (size_t)d.v0[e] * 3;
    pv[0] = p[0]; pv[1] = p[1]; pv[2] = p[2];
    double rp[3];
    qrot(q, pv, rp);
    x[0] = s * rp[0] + t[0]; x[1] = s * rp[1] + t[1]; x[2] = s * rp[2] + t[2];
  }
  DI static void residual(const double* K, const double* x, const double* m, double* err) {
#pragma clang fp contract(off)
    err[0] = m[0] - (x[0] / x[2] * K[0] + K[2]);
    err[1] = m[1] - (x[1] / x[2] * K[1] + K[3]);
  }
  DI static void error(const EdgeData& d, int e, double* err) {
    double q[4], s, pv[3], x[3];
    map(d, e, q, s, pv, x);
    residual(param_rec(d, e, PAR), x, d.meas + (size_t)e * MEAS, err);
  }
  // the error and B = Jj, 2 x 7 row-major in (omega, upsilon, sigma) order
  DI static void jac_pose(const EdgeData& d, int e, double* err, double* B) {
    double q[4], s, pv[3], x[3];
    map(d, e, q, s, pv, x);
    const double* K = param_rec(d, e, PAR);
    residual(K, x, d.meas + (size_t)e * MEAS, err);
    const double iz = 1.0 / x[2];
    // -P, rows (a0, 0, a2) and (0, b1, b2)
    const double a0 = -K[0] * iz, a2 = K[0] * x[0] * iz * iz, b1 = -K[1] * iz, b2 = K[1] * x[1] * iz * iz;
    double G[21];  // d x / d u, 3 x 7 row-major
    if (INV) {
      double R[9];
      quat_to_R(q[0], q[1], q[2], q[3], R);
      // [ [p]x | -I | -p ], then s R in front
      const double C[21] = {0,      -pv[2], pv[1],  -1, 0,  0,  -pv[0],
                            pv[2],  0,      -pv[0], 0,  -1, 0,  -pv[1],
                            -pv[1], pv[0],  0,      0,  0,  -1, -pv[2]};
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 7; ++c)
          G[r * 7 + c] = s * (R[r * 3] * C[c] + R[r * 3 + 1] * C[7 + c] + R[r * 3 + 2] * C[14 + c]);
    } else {
      const double C[21] = {0,     x[2],  -x[1], 1, 0, 0, x[0],
                            -x[2], 0,     x[0],  0, 1, 0, x[1],
                            x[1],  -x[0], 0,     0, 0, 1, x[2]};
#pragma unroll
      for (int i = 0; i < 21; ++i) G[i] = C[i];
    }
#pragma unroll
    for (int c = 0; c < 7; ++c) {
      B[c] = a0 * G[c] + a2 * G[14 + c];
      B[7 + c] = b1 * G[7 + c] + b2 * G[14 + c];
    }
  }
};

// ---- EdgeObservationBAL (examples/bal/bal_example.cpp:156-281): v0 = VertexCameraBAL [9] rx ry rz tx ty tz f k1 k2 (an
// angle-axis rotation, world to camera), v1 = point (3); meas u v, info packed 3, no parameter record, no depth test.
// With w = est[0:3], th = |w|: P = X cos th + (v x X) sin th + v (v.X)(1 - cos th), v = w / th (th == 0: P = X + w x X),
// P += t, p = -P.xy / P.z, r2 = p.p, rp = 1 + k1 r2 + k2 r2 r2, e = f rp p - z, in the reference's operation order. The
// reference differentiates this with ceres autodiff, which gives the exact first derivatives of the expression as
// written, branch by branch; so does this:
//   dE = f (rp I + (2 k1 + 4 k2 r2) p p^T), dp/dP = [[-1/Pz, 0, Px/Pz^2], [0, -1/Pz, Py/Pz^2]], M = dE dp/dP (2 x 3),
//   Ji = [ M dP/dw | M | rp p | f r2 p | f r2^2 p ],  Jj = M dP/dX (the Rodrigues matrix of the branch).
// dP/dw_k for th > 0 goes term by term through th, v, sin and cos, with dth/dw_k = v_k, dv/dw_k = (e_k - v v_k) / th:
//   -X sin th v_k + (dv x X) sin th + (v x X) cos th v_k + dv (v.X)(1 - cos th) + v (dv.X)(1 - cos th) + v (v.X) sin th v_k
// (no closed form that divides differences by th^2: such a form loses digits for small th, where autodiff does not);
// th == 0: dP/dw = -[X]x, dP/dX = I + [w]x. ----
struct FamilyBAL {
  static constexpr int D = 2, DA = 9, DB = 3, MEAS = 2, INFO = 3, PAR = 0;
  // P (before the translation), and with JAC the 3 x 3 row-major dP/dw and dP/dX
  template <bool JAC>
  DI static void rotate(const double* w, const double* X, double* P, double* dPw, double* dPX) {
    const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    if (th > 0) {
      const double v[3] = {w[0] / th, w[1] / th, w[2] / th};
      const double c = cos(th), s = sin(th);
      const double vX[3] = {v[1] * X[2] - v[2] * X[1], v[2] * X[0] - v[0] * X[2], v[0] * X[1] - v[1] * X[0]};
      const double vd = v[0] * X[0] + v[1] * X[1] + v[2] * X[2];
      const double omc = 1.0 - c;
#pragma unroll
      for (int i = 0; i < 3; ++i) P[i] = X[i] * c + vX[i] * s + v[i] * vd * omc;
      if (JAC) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          double dv[3];
#pragma unroll
          for (int i = 0; i < 3; ++i) dv[i] = ((i == k ? 1.0 : 0.0) - v[i] * v[k]) / th;
          const double dvX[3] = {dv[1] * X[2] - dv[2] * X[1], dv[2] * X[0] - dv[0] * X[2], dv[0] * X[1] - dv[1] * X[0]};
          const double dvd = dv[0] * X[0] + dv[1] * X[1] + dv[2] * X[2];
          const double dc = -s * v[k], ds = c * v[k];  // d cos th, d sin th
#pragma unroll
          for (int i = 0; i < 3; ++i)
            dPw[i * 3 + k] = X[i] * dc + dvX[i] * s + vX[i] * ds + dv[i] * vd * omc + v[i] * dvd * omc - v[i] * vd * dc;
        }
        // dP/dX = c I + s [v]x + (1 - c) v v^T
        const double R[9] = {c + omc * v[0] * v[0],        -s * v[2] + omc * v[0] * v[1], s * v[1] + omc * v[0] * v[2],
                             s * v[2] + omc * v[1] * v[0], c + omc * v[1] * v[1],         -s * v[0] + omc * v[1] * v[2],
                             -s * v[1] + omc * v[2] * v[0], s * v[0] + omc * v[2] * v[1], c + omc * v[2] * v[2]};
#pragma unroll
        for (int i = 0; i < 9; ++i) dPX[i] = R[i];
      }
    } else {  // the reference's Taylor branch, taken at th == 0 exactly
      P[0] = X[0] + (w[1] * X[2] - w[2] * X[1]);
      P[1] = X[1] + (w[2] * X[0] - w[0] * X[2]);
      P[2] = X[2] + (w[0] * X[1] - w[1] * X[0]);
      if (JAC) {
        const double A[9] = {0, X[2], -X[1], -X[2], 0, X[0], X[1], -X[0], 0};       // -[X]x
        const double R[9] = {1, -w[2], w[1], w[2], 1, -w[0], -w[1], w[0], 1};       // I + [w]x
#pragma unroll
        for (int i = 0; i < 9; ++i) { dPw[i] = A[i]; dPX[i] = R[i]; }
      }
    }
  }
  DI static void load(const EdgeData& d, int e, double* cam, double* X) {
    const double* c = d.s0 + (size_t)d.v0[e] * 9;
    const double* x = d.s1 + (size_t)d.v1[e] * 3;
#pragma unroll
    for (int k = 0; k < 9; ++k) cam[k] = c[k];
    X[0] = x[0]; X[1] = x[1]; X[2] = x[2];
  }
  DI static void error(const EdgeData& d, int e, double* err) {
    double cam[9], X[3], P[3];
    load(d, e, cam, X);
    rotate<false>(cam, X, P, nullptr, nullptr);
    P[0] += cam[3]; P[1] += cam[4]; P[2] += cam[5];
    const double* m = d.meas + (size_t)e * 2;
    const double p0 = -P[0] / P[2], p1 = -P[1] / P[2];
    const double r2 = p0 * p0 + p1 * p1;
    const double rp = 1.0 + cam[7] * r2 + cam[8] * r2 * r2;
    err[0] = cam[6] * rp * p0 - m[0];
    err[1] = cam[6] * rp * p1 - m[1];
  }
  DI static void linearize(const EdgeData& d, int e, double* err, double* Ji, double* Jj) {
    double cam[9], X[3], P[3], dPw[9], dPX[9];
    load(d, e, cam, X);
    rotate<true>(cam, X, P, dPw, dPX);
    P[0] += cam[3]; P[1] += cam[4]; P[2] += cam[5];
    const double* m = d.meas + (size_t)e * 2;
    const double p0 = -P[0] / P[2], p1 = -P[1] / P[2];
    const double r2 = p0 * p0 + p1 * p1;
    const double f = cam[6], k1 = cam[7], k2 = cam[8];
    const double rp = 1.0 + k1 * r2 + k2 * r2 * r2;
    err[0] = f * rp * p0 - m[0];
    err[1] = f * rp * p1 - m[1];
    const double g = 2 * k1 + 4 * k2 * r2;
    const double dE[4] = {f * (rp + g * p0 * p0), f * (g * p0 * p1), f * (g * p0 * p1), f * (rp + g * p1 * p1)};
    const double iz = 1.0 / P[2];
    const double dp[6] = {-iz, 0, P[0] * iz * iz, 0, -iz, P[1] * iz * iz};
    double M[6];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) M[r * 3 + c] = dE[r * 2] * dp[c] + dE[r * 2 + 1] * dp[3 + c];
    const double pr[2] = {p0, p1};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        Ji[r * 9 + c] = M[r * 3] * dPw[c] + M[r * 3 + 1] * dPw[3 + c] + M[r * 3 + 2] * dPw[6 + c];
        Ji[r * 9 + 3 + c] = M[r * 3 + c];
        Jj[r * 3 + c] = M[r * 3] * dPX[c] + M[r * 3 + 1] * dPX[3 + c] + M[r * 3 + 2] * dPX[6 + c];
      }
      Ji[r * 9 + 6] = rp * pr[r];
      Ji[r * 9 + 7] = f * r2 * pr[r];
      Ji[r * 9 + 8] = f * r2 * r2 * pr[r];
    }
  }
};

// ---- EdgeSE3ProjectXYZOnlyPose (types_six_dof_expmap.h:242-246, .cpp:569-599), unary: v0 = camera SE3Quat [8];
// meas payload u v | Xw (5), info packed 3, params fx fy cx cy (one shared record when EdgeData::ue bit 1 is set).
// error = obs - cam_project(T.map(Xw)); the Jacobian in the reference's invz / invz_2 products ----
struct FamilyPoseOnly {
  static constexpr int D = 2, DA = 6, MEAS = 5, INFO = 3, PAR = 4;
  DI static void to_camera(const EdgeData& d, int e, const double* m, double* pc) {
    const double* c = d.s0 + (size_t)d.v0[e] * 8;
    const double q[4] = {c[3], c[4], c[5], c[6]};
    const double pv[3] = {m[0], m[1], m[2]};
    qrot(q, pv, pc);
    pc[0] += c[0]; pc[1] += c[1]; pc[2] += c[2];
  }
  // rows 0-1 of the pose Jacobian (shared with the stereo type, .cpp:645-657)
  DI static void jac_uv(const double* K, const double* pc, double invz, double invz_2, double* A) {
    const double fx = K[0], fy = K[1], x = pc[0], y = pc[1];
    A[0] = x * y * invz_2 * fx;
    A[1] = -(1 + (x * x * invz_2)) * fx;
    A[2] = y * invz * fx;
    A[3] = -invz * fx;
    A[4] = 0;
    A[5] = x * invz_2 * fx;
    A[6] = (1 + y * y * invz_2) * fy;
    A[7] = -x * y * invz_2 * fy;
    A[8] = -x * invz * fy;
    A[9] = 0;
    A[10] = -invz * fy;
    A[11] = y * invz_2 * fy;
  }
  DI static void residual(const double* K, const double* pc, const double* m, double* err) {
    err[0] = m[0] - (pc[0] / pc[2] * K[0] + K[2]);
    err[1] = m[1] - (pc[1] / pc[2] * K[1] + K[3]);
  }
  // the error, and the point's z in the camera frame (isDepthPositive, types_six_dof_expmap.h:248-251)
  DI static double depth(const EdgeData& d, int e, double* err) {
    const double* m = d.meas + (size_t)e * MEAS;
    double pc[3];
    to_camera(d, e, m + 2, pc);
    residual(param_rec(d, e, PAR), pc, m, err);
    return pc[2];
  }
  DI static void error(const EdgeData& d, int e, double* err) { depth(d, e, err); }
  DI static void linearize(const EdgeData& d, int e, double* err, double* A) {
    const double* m = d.meas + (size_t)e * MEAS;
    const double* K = param_rec(d, e, PAR);
    double pc[3];
    to_camera(d, e, m + 2, pc);
    residual(K, pc, m, err);
    const double invz = 1.0 / pc[2], invz_2 = invz * invz;
    jac_uv(K, pc, invz, invz_2, A);
  }
};

// ---- EdgeStereoSE3ProjectXYZOnlyPose (types_six_dof_expmap.h:303-307, .cpp:601-608, 636-665), unary: meas payload
// u_l v u_r | Xw (6), info packed 6, params fx fy cx cy bf. cam_project holds 1/z in a float (`const float invz`), so
// all three error components see it rounded; bf stays a double here. The Jacobian uses the double 1/z. ----
struct FamilyStereoPoseOnly {
  static constexpr int D = 3, DA = 6, MEAS = 6, INFO = 6, PAR = 5;
  // No contraction: the projection rounds as the reference's does, operation by operation (as FamilyStereo::residual)
  DI static void residual(const double* K, const double* pc, const double* m, double* err) {
#pragma clang fp contract(off)
    const double invz = (double)(float)(1.0 / pc[2]);
    const double u = pc[0] * invz * K[0] + K[2];
    const double v = pc[1] * invz * K[1] + K[3];
    const double ur = u - K[4] * invz;
    err[0] = m[0] - u;
    err[1] = m[1] - v;
    err[2] = m[2] - ur;
  }
  // the error, and the point's z in the camera frame (isDepthPositive, types_six_dof_expmap.h:309-312)
  DI static double depth(const EdgeData& d, int e, double* err) {
    const double* m = d.meas + (size_t)e * MEAS;
    double pc[3];
    FamilyPoseOnly::to_camera(d, e, m + 3, pc);
    residual(param_rec(d, e, PAR), pc, m, err);
    return pc[2];
  }
  DI static void error(const EdgeData& d, int e, double* err) { depth(d, e, err); }
  DI static void linearize(const EdgeData& d, int e, double* err, double* A) {
    const double* m = d.meas + (size_t)e * MEAS;
    const double* K = param_rec(d, e, PAR);
    double pc[3];
    FamilyPoseOnly::to_camera(d, e, m + 3, pc);
    residual(K, pc, m, err);
    const double invz = 1.0 / pc[2], invz_2 = invz * invz, bf = K[4];
    FamilyPoseOnly::jac_uv(K, pc, invz, invz_2, A);
    A[12] = A[0] - bf * pc[1] * invz_2;
    A[13] = A[1] + bf * pc[0] * invz_2;
    A[14] = A[2];
    A[15] = A[3];
    A[16] = 0;
    A[17] = A[5] - bf * invz_2;
  }
};

}  // namespace dev
}  // namespace g2ohip
