// StructureOnlySolver<PointDoF>::calc on the device (g2o/solvers/structure_only/structure_only_solver.h:72-212): with
// every other vertex held fixed each landmark is its own small Levenberg-Marquardt problem, so one launch runs all
// iterations and all trials of every selected landmark.
//
// Layout: SO_WIDTH (8) lanes per landmark, 32 landmarks per 256-thread block. A lane walks the landmark's (group, edge)
// list with stride 8 and accumulates chi2, the packed upper H = sum A^T (rho' Omega) A and b = -sum A^T (rho' Omega) e
// of its share in list order; the eight shares meet in a three-step xor butterfly (IEEE addition commutes, so every
// lane of the group ends with the same bits and takes the same branches). mu, nu, chi2, the estimate and its saved copy
// (:161, :186) stay in registers; lane 0 stores the estimate once, at the end. Only the landmark's Jacobian is formed.
// Nothing but the point array is written, no atomics, no waiting on another workgroup; every loop is bounded by
// num_iters x num_max_trials.
#include <hip/hip_runtime.h>

#include "../../include/g2o_hip.h"
#include "device_types.hpp"
#include "kernels.hpp"
#include "structure_only.hpp"
#include "common.hpp"

namespace g2ohip {
namespace {
using namespace dev;
using launch::SoCall;
using launch::SoGroup;
using launch::SO_BLOCK;
using launch::SO_COUNTS;
using launch::SO_LMS;
using launch::SO_WIDTH;

DI const double* so_info(const SoGroup& g, int e, int stride) { return g.info + ((g.ue & 1) ? 0 : (size_t)e * stride); }
DI const double* so_param(const SoGroup& g, int e, int stride) { return g.params + ((g.ue & 2) ? 0 : (size_t)e * stride); }

// ---- point-only linearisation of each family with a landmark end: the error and, with JAC, the landmark's Jacobian A
// (D x LD, row-major) at the point p, in the operation order of the family's own linearize (device_types.hpp). The
// camera / pose Jacobian is never formed.
template <int FAM>
struct PointEdge;

template <>
struct PointEdge<FAM_BA> {  // FamilyBA::linearize_at
  static constexpr int D = 2, LD = 3;
  template <bool JAC>
  DI static void eval(const SoGroup& g, int e, const double* p, double* err, double* A) {
    const double* c = g.so + (size_t)g.vo[e] * 8;
    const double q[4] = {c[3], c[4], c[5], c[6]};
    double pc[3];
    qrot(q, p, pc);
    pc[0] += c[0]; pc[1] += c[1]; pc[2] += c[2];
    const double* K = so_param(g, e, 4);
    const double fx = K[0], fy = K[1];
    const double x = pc[0], y = pc[1], z = pc[2];
    err[0] = g.meas[(size_t)e * 2 + 0] - (x / z * fx + K[2]);
    err[1] = g.meas[(size_t)e * 2 + 1] - (y / z * fy + K[3]);
    if (JAC) {
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
    }
  }
};

template <bool UVU>
struct PointStereo {  // FamilyStereoT<UVU>::linearize_at
  using F = FamilyStereoT<UVU>;
  static constexpr int D = 3, LD = 3;
  template <bool JAC>
  DI static void eval(const SoGroup& g, int e, const double* p, double* err, double* A) {
    const double* c = g.so + (size_t)g.vo[e] * 8;
    const double q[4] = {c[3], c[4], c[5], c[6]};
    double pc[3];
    qrot(q, p, pc);
    pc[0] += c[0]; pc[1] += c[1]; pc[2] += c[2];
    const double* K = so_param(g, e, 5);
    const double* m = g.meas + (size_t)e * 3;
    F::residual(K, pc, m[0], m[1], m[2], err);
    if (JAC) {
      const double fx = K[0], fy = K[1], bf = F::bf_of(K);
      const double x = pc[0], y = pc[1], z = pc[2], z_2 = z * z;
      double R[9];
      quat_to_R(q[0], q[1], q[2], q[3], R);
#pragma unroll
      for (int cc = 0; cc < 3; ++cc) {
        A[cc] = -fx * R[cc] / z + fx * x * R[6 + cc] / z_2;
        A[3 + cc] = -fy * R[3 + cc] / z + fy * y * R[6 + cc] / z_2;
        A[6 + cc] = A[cc] - bf * R[6 + cc] / z_2;
      }
    }
  }
};
template <> struct PointEdge<FAM_BA_STEREO> : PointStereo<false> {};
template <> struct PointEdge<FAM_BA_UVU> : PointStereo<true> {};  // EdgeProjectXYZ2UVU (EdgeProjectXYZ2UV is FAM_BA)

template <int MODE>
struct PointSlam3d {  // FamilySlam3d<MODE>::linearize, the last three columns of J'
  static constexpr int D = 3, LD = 3;
  using F = FamilySlam3d<MODE>;
  template <bool JAC>
  DI static void eval(const SoGroup& g, int e, const double* p, double* err, double* A) {
    const double* x = g.so + (size_t)g.vo[e] * 12;
    const double* Pi = so_param(g, e, F::PAR);
    const double* mp = g.meas + (size_t)e * 3;
    double X[12], Zc[3], pn[3], pi[3];
#pragma unroll
    for (int k = 0; k < 12; ++k) X[k] = x[k];
    const double m[3] = {mp[0], mp[1], mp[2]};
    F::to_sensor(X, p, Pi, Zc, pn);
    F::residual(Pi, pn, m, pi, err);
    if (JAC) {
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        double m0, m1, m2;  // row r of M = Rp^T (XYZ) or K Rp^T (camera modes)
        if (MODE == SLAM3D_XYZ || r == 2) {
          m0 = Pi[r * 3]; m1 = Pi[r * 3 + 1]; m2 = Pi[r * 3 + 2];
        } else {
          const double f = Pi[12 + r], cc = Pi[14 + r];
          m0 = f * Pi[r * 3] + cc * Pi[6]; m1 = f * Pi[r * 3 + 1] + cc * Pi[7]; m2 = f * Pi[r * 3 + 2] + cc * Pi[8];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) A[r * 3 + c] = m0 * X[c * 3] + m1 * X[c * 3 + 1] + m2 * X[c * 3 + 2];
      }
      if (MODE != SLAM3D_XYZ) {
        const double iz2 = 1.0 / (pi[2] * pi[2]);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double j2 = A[6 + c];
          A[c] = iz2 * (A[c] * pi[2] - pi[0] * j2);
          A[3 + c] = iz2 * (A[3 + c] * pi[2] - pi[1] * j2);
          if (MODE == SLAM3D_DISPARITY) A[6 + c] = -j2 * iz2;
        }
      }
    }
  }
};
template <> struct PointEdge<FAM_SE3_XYZ> : PointSlam3d<SLAM3D_XYZ> {};
template <> struct PointEdge<FAM_SE3_XYZ_DEPTH> : PointSlam3d<SLAM3D_DEPTH> {};
template <> struct PointEdge<FAM_SE3_XYZ_DISPARITY> : PointSlam3d<SLAM3D_DISPARITY> {};

template <bool STEREO>
struct PointSBA {  // FamilySBA<STEREO>::linearize_at, the point's Jacobian alone
  static constexpr int D = STEREO ? 3 : 2, LD = 3;
  using F = FamilySBA<STEREO>;
  template <bool JAC>
  DI static void eval(const SoGroup& g, int e, const double* p, double* err, double* A) {
    const double* cp = g.so + (size_t)g.vo[e] * 12;
    const double* mp = g.meas + (size_t)e * D;
    double c[12], m[D], Rt[9], pc[3];
#pragma unroll
    for (int k = 0; k < 12; ++k) c[k] = cp[k];
#pragma unroll
    for (int k = 0; k < D; ++k) m[k] = mp[k];
    F::to_camera(c, p, Rt, pc);
    F::residual(c, pc, m, err);
    if (JAC) {
      const double ipz2 = 1.0 / (pc[2] * pc[2]);
      const double fx2 = ipz2 * c[7], fy2 = ipz2 * c[8];
      const double xs = pc[0] - c[11];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double dx = Rt[k], dy = Rt[3 + k], dz = Rt[6 + k];
        A[k] = (pc[2] * dx - pc[0] * dz) * fx2;
        A[3 + k] = (pc[2] * dy - pc[1] * dz) * fy2;
        if (STEREO) A[6 + k] = (pc[2] * dx - xs * dz) * fx2;
      }
    }
  }
};
template <> struct PointEdge<FAM_SBA_MONO> : PointSBA<false> {};
template <> struct PointEdge<FAM_SBA_STEREO> : PointSBA<true> {};

template <>
struct PointEdge<FAM_VSC> {  // FamilyVSC::core, the point's Jacobian alone
  static constexpr int D = 3, LD = 3;
  template <bool JAC>
  DI static void eval(const SoGroup& g, int e, const double* p, double* err, double* A) {
    const double* xp = g.so + (size_t)g.vo[e] * 12;
    const double* mp = g.meas + (size_t)e * 3;
    const double* Kp = so_param(g, e, 5);
    double X[12], B[18];
#pragma unroll
    for (int k = 0; k < 12; ++k) X[k] = xp[k];
    const double m[3] = {mp[0], mp[1], mp[2]}, K[5] = {Kp[0], Kp[1], Kp[2], Kp[3], Kp[4]};
    FamilyVSC::core<JAC, false>(X, K, p, m, err, A, B);
  }
};

template <>
struct PointEdge<FAM_SE2XY> {  // FamilySE2XY::linearize, Jj
  static constexpr int D = 2, LD = 2;
  template <bool JAC>
  DI static void eval(const SoGroup& g, int e, const double* p, double* err, double* A) {
    const double* xi = g.so + (size_t)g.vo[e] * 3;
    const double* m = g.meas + (size_t)e * 2;
    const double a[3] = {xi[0], xi[1], xi[2]};
    double ai[3];
    FamilySE2::inverse(a, ai);
    const double c = cos(ai[2]), s = sin(ai[2]);
    err[0] = (ai[0] + (c * p[0] - s * p[1])) - m[0];
    err[1] = (ai[1] + (s * p[0] + c * p[1])) - m[1];
    if (JAC) {
      const double cj = cos(a[2]), sj = sin(a[2]);
      A[0] = cj; A[1] = sj;
      A[2] = -sj; A[3] = cj;
    }
  }
};

template <>
struct PointEdge<FAM_SE2XY_BEARING> {  // FamilySE2XYBearing::linearize, Jj
  static constexpr int D = 1, LD = 2;
  template <bool JAC>
  DI static void eval(const SoGroup& g, int e, const double* p, double* err, double* A) {
    const double* xi = g.so + (size_t)g.vo[e] * 3;
    double dd[2];
    FamilySE2XYBearing::to_sensor(xi, p, dd);
    err[0] = normalize_theta(g.meas[e] - atan2(dd[1], dd[0]));
    if (JAC) FamilySE2XYBearing::point_jacobian(xi[2], dd, A);
  }
};

template <int N>
struct PointPrior {  // FamilyUnaryPoint<N>: error = estimate - z, J = I
  static constexpr int D = N, LD = N;
  template <bool JAC>
  DI static void eval(const SoGroup& g, int e, const double* p, double* err, double* A) {
    const double* m = g.meas + (size_t)e * N;
#pragma unroll
    for (int i = 0; i < N; ++i) err[i] = p[i] - m[i];
    if (JAC) {
#pragma unroll
      for (int i = 0; i < N * N; ++i) A[i] = (i % (N + 1) == 0) ? 1.0 : 0.0;
    }
  }
};
template <> struct PointEdge<FAM_U_XYZ> : PointPrior<3> {};
template <> struct PointEdge<FAM_U_XY> : PointPrior<2> {};

// one edge's share: chi += rho(e^T Omega e) (:92-101, :167-176); with JAC H += A^T (rho' Omega) A and
// b -= A^T (rho' Omega) e (constructQuadraticForm, base_binary_edge.hpp / base_unary_edge.hpp; robustInformation is
// rho' Omega, base_edge.h:117-123)
template <int FAM, bool JAC>
DI void edge_term(const SoGroup& g, int e, const double* p, double& chi, double* H, double* b) {
  using P = PointEdge<FAM>;
  constexpr int D = P::D, LD = P::LD;
  double err[D], A[D * LD];
  P::template eval<JAC>(g, e, p, err, A);
  double Om[D * D], w[D];
  load_info<D>(so_info(g, e, D * (D + 1) / 2), Om);
  double e2 = 0;
#pragma unroll
  for (int i = 0; i < D; ++i) {
    double s = 0;
#pragma unroll
    for (int j = 0; j < D; ++j) s += Om[i * D + j] * err[j];
    w[i] = s;
    e2 += err[i] * s;
  }
  double r0, r1;
  robustify(g.rk, g.rk_delta, e2, r0, r1);
  chi += r0;
  if (JAC) {
    double WA[D * LD];  // Omega A
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int c = 0; c < LD; ++c) {
        double s = 0;
#pragma unroll
        for (int j = 0; j < D; ++j) s += Om[i * D + j] * A[j * LD + c];
        WA[i * LD + c] = s;
      }
#pragma unroll
    for (int c = 0; c < LD; ++c) {
#pragma unroll
      for (int r = 0; r <= c; ++r) {
        double s = 0;
#pragma unroll
        for (int i = 0; i < D; ++i) s += A[i * LD + r] * WA[i * LD + c];
        H[up_idx(r, c)] += r1 * s;
      }
      double t = 0;
#pragma unroll
      for (int i = 0; i < D; ++i) t += A[i * LD + c] * w[i];
      b[c] -= r1 * t;
    }
  }
}

// FAM >= 0: every entry is of that family; FAM < 0: dispatch on the entry's group
template <int LD, int FAM, bool JAC>
DI void edge_any(const SoGroup* groups, int2 en, const double* p, double& chi, double* H, double* b) {
  const SoGroup& g = groups[en.x];
  if constexpr (FAM >= 0) {
    edge_term<(FAM >= 0 ? FAM : (LD == 3 ? FAM_BA : FAM_SE2XY)), JAC>(g, en.y, p, chi, H, b);
  } else if constexpr (LD == 3) {
    switch (g.family) {
      case FAM_BA: edge_term<FAM_BA, JAC>(g, en.y, p, chi, H, b); break;
      case FAM_BA_STEREO: edge_term<FAM_BA_STEREO, JAC>(g, en.y, p, chi, H, b); break;
      case FAM_BA_UVU: edge_term<FAM_BA_UVU, JAC>(g, en.y, p, chi, H, b); break;
      case FAM_SE3_XYZ: edge_term<FAM_SE3_XYZ, JAC>(g, en.y, p, chi, H, b); break;
      case FAM_SE3_XYZ_DEPTH: edge_term<FAM_SE3_XYZ_DEPTH, JAC>(g, en.y, p, chi, H, b); break;
      case FAM_SE3_XYZ_DISPARITY: edge_term<FAM_SE3_XYZ_DISPARITY, JAC>(g, en.y, p, chi, H, b); break;
      case FAM_SBA_MONO: edge_term<FAM_SBA_MONO, JAC>(g, en.y, p, chi, H, b); break;
      case FAM_SBA_STEREO: edge_term<FAM_SBA_STEREO, JAC>(g, en.y, p, chi, H, b); break;
      case FAM_VSC: edge_term<FAM_VSC, JAC>(g, en.y, p, chi, H, b); break;
      default: edge_term<FAM_U_XYZ, JAC>(g, en.y, p, chi, H, b); break;
    }
  } else {
    if (g.family == FAM_SE2XY) edge_term<FAM_SE2XY, JAC>(g, en.y, p, chi, H, b);
    else if (g.family == FAM_SE2XY_BEARING) edge_term<FAM_SE2XY_BEARING, JAC>(g, en.y, p, chi, H, b);
    else edge_term<FAM_U_XY, JAC>(g, en.y, p, chi, H, b);
  }
}

// the eight lanes' shares in a fixed tree; every lane of the group receives the same bits
DI double group_sum(double v) {
  v += __shfl_xor(v, 4, SO_WIDTH);
  v += __shfl_xor(v, 2, SO_WIDTH);
  v += __shfl_xor(v, 1, SO_WIDTH);
  return v;
}

// (H + mu I) x = b by LDL^T in registers (:155-160). Positive as Eigen's LDLT::isPositive: no negative pivot; a NaN
// pivot fails the trial; a zero pivot contributes nothing to the solution (Eigen's solve drops it)
DI double pivot_div(double v, double d) { return d != 0 ? v / d : 0.0; }  // true divisions: a pivot equal to v gives 1
template <int LD>
DI bool solve_damped(const double* H, double mu, const double* b, double* x);
template <>
DI bool solve_damped<3>(const double* H, double mu, const double* b, double* x) {
  const double a00 = H[0] + mu, a01 = H[1], a11 = H[2] + mu, a02 = H[3], a12 = H[4], a22 = H[5] + mu;
  const double d0 = a00;
  if (!(d0 >= 0)) return false;
  const double l10 = pivot_div(a01, d0), l20 = pivot_div(a02, d0);
  const double d1 = a11 - l10 * a01;
  if (!(d1 >= 0)) return false;
  const double t = a12 - l20 * a01;
  const double l21 = pivot_div(t, d1);
  const double d2 = a22 - l20 * a02 - l21 * t;
  if (!(d2 >= 0)) return false;
  const double y0 = b[0], y1 = b[1] - l10 * y0, y2 = b[2] - l20 * y0 - l21 * y1;
  x[2] = pivot_div(y2, d2);
  x[1] = pivot_div(y1, d1) - l21 * x[2];
  x[0] = pivot_div(y0, d0) - l10 * x[1] - l20 * x[2];
  return true;
}
template <>
DI bool solve_damped<2>(const double* H, double mu, const double* b, double* x) {
  const double a00 = H[0] + mu, a01 = H[1], a11 = H[2] + mu;
  const double d0 = a00;
  if (!(d0 >= 0)) return false;
  const double l10 = pivot_div(a01, d0);
  const double d1 = a11 - l10 * a01;
  if (!(d1 >= 0)) return false;
  const double y0 = b[0], y1 = b[1] - l10 * y0;
  x[1] = pivot_div(y1, d1);
  x[0] = pivot_div(y0, d0) - l10 * x[1];
  return true;
}

template <int LD, int FAM>
__global__ void __launch_bounds__(SO_BLOCK) k_structure_only(SoCall c) {
  constexpr int NH = LD * (LD + 1) / 2;
  __shared__ int sh_cnt[SO_LMS * SO_COUNTS];
  const int lane = threadIdx.x & (SO_WIDTH - 1), gl = threadIdx.x / SO_WIDTH;
  const long long j = (long long)blockIdx.x * SO_LMS + gl;
  int cnt[SO_COUNTS] = {0, 0, 0, 0, 0};
  if (j < c.nsel) {
    const int l = c.sel ? c.sel[j] : (int)j;
    if (c.lm_fixed[l]) {
      cnt[4] = 1;  // :104 (the reference computes the fixed point's chi2 and drops it)
    } else {
      const int e0 = c.lm_ptr[l], e1 = c.lm_ptr[l + 1];
      double* pp = c.pts + (size_t)c.lm_local[l] * LD;
      double p[LD], H[NH], b[LD];
#pragma unroll
      for (int i = 0; i < LD; ++i) p[i] = pp[i];
      double mu = 0.01, nu = 2;  // :86-87, fresh per point and per call
      double chi = 0;            // :89-102
      for (int k = e0 + lane; k < e1; k += SO_WIDTH) edge_any<LD, FAM, false>(c.groups, c.ent[k], p, chi, H, b);
      chi = group_sum(chi);
      bool moved = false;
      for (int it = 0; it < c.num_iters; ++it) {  // :108
#pragma unroll
        for (int i = 0; i < NH; ++i) H[i] = 0;
#pragma unroll
        for (int i = 0; i < LD; ++i) b[i] = 0;
        double dummy = 0;
        for (int k = e0 + lane; k < e1; k += SO_WIDTH) edge_any<LD, FAM, true>(c.groups, c.ent[k], p, dummy, H, b);
#pragma unroll
        for (int i = 0; i < NH; ++i) H[i] = group_sum(H[i]);
        double bn = 0;
#pragma unroll
        for (int i = 0; i < LD; ++i) {
          b[i] = group_sum(b[i]);
          bn += b[i] * b[i];
        }
        if (sqrt(bn) < 0.001) {  // :148
          cnt[2] = 1;
          break;
        }
        bool stop = false;
        int trial = 0;
        for (;;) {  // :154-205; leaves by an accepted step or after max_trials failures
          double dx[LD], pn[LD];
          bool good = false;
          if (solve_damped<LD>(H, mu, b, dx)) {  // :159
#pragma unroll
            for (int i = 0; i < LD; ++i) pn[i] = p[i] + dx[i];  // :161-162 (the saved estimate is p)
            double nchi = 0;
            for (int k = e0 + lane; k < e1; k += SO_WIDTH) edge_any<LD, FAM, false>(c.groups, c.ent[k], pn, nchi, H, b);
            nchi = group_sum(nchi);
            if (chi - nchi > 0 && isfinite(nchi)) {  // :179-183
              good = true;
              chi = nchi;
#pragma unroll
              for (int i = 0; i < LD; ++i) p[i] = pn[i];
              moved = true;
            }
          }
          if (good) {  // :191-195
            mu *= 1. / 3.;
            nu = 2.;
            ++cnt[0];
            break;
          }
          mu *= nu;  // :197-203
          nu *= 2.;
          ++cnt[1];
          if (++trial >= c.max_trials) {
            stop = true;
            cnt[3] = 1;
            break;
          }
        }
        if (stop) break;  // :206-207
      }
      if (moved && lane == 0) {
#pragma unroll
        for (int i = 0; i < LD; ++i) pp[i] = p[i];
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < SO_COUNTS; ++k) sh_cnt[gl * SO_COUNTS + k] = cnt[k];
  }
  __syncthreads();
  if (threadIdx.x < SO_COUNTS) {  // the block's landmarks in order
    long long s = 0;
    for (int g = 0; g < SO_LMS; ++g) s += sh_cnt[g * SO_COUNTS + threadIdx.x];
    c.part[(size_t)blockIdx.x * SO_COUNTS + threadIdx.x] = s;
  }
}
}  // namespace

namespace launch {
void structure_only(int ld, int single_family, const SoCall& c, hipStream_t s) {
  if (c.nsel <= 0) return;
  const dim3 grid(so_blocks(c.nsel)), block(SO_BLOCK);
  if (ld == 3 && single_family == FAM_BA) k_structure_only<3, FAM_BA><<<grid, block, 0, s>>>(c);
  else if (ld == 3) k_structure_only<3, -1><<<grid, block, 0, s>>>(c);
  else if (ld == 2 && single_family == FAM_SE2XY) k_structure_only<2, FAM_SE2XY><<<grid, block, 0, s>>>(c);
  else if (ld == 2) k_structure_only<2, -1><<<grid, block, 0, s>>>(c);
  else throw StatusError(G2OHIP_ERR_UNSUPPORTED, "structure-only: landmark dimension " + std::to_string(ld));
  KERNEL_CHECK();
}
}  // namespace launch
}  // namespace g2ohip
