// Runtime family code -> the device family type, for the launchers of kernels.hip and classify.hip: fn is called with a
// value of the family (fn(FamilyBA{}), ...) and launches the kernel instantiated for it. Each mapping is checked against
// the family's rows of EDGE_TYPES (edge_types.hpp) at compile time: the host fills the measurement and parameter
// buffers with the rows' strides, the kernels index them with F::MEAS and F::PAR.
#pragma once
#include <stdexcept>
#include <type_traits>

#include "device_types.hpp"
#include "kernels.hpp"

namespace g2ohip {
namespace launch {
using namespace dev;

template <class F, class = void> struct family_db : std::integral_constant<int, 0> {};  // unary families: no DB
template <class F> struct family_db<F, std::void_t<decltype(F::DB)>> : std::integral_constant<int, F::DB> {};

// F{} for the family code FAM, once EDGE_TYPES' rows of FAM are known to describe F
template <Family FAM, class F>
constexpr F checked() {
  static_assert(family_rows_have(FAM, row_D, F::D), "EDGE_TYPES: a row's D is not the family's F::D");
  static_assert(family_rows_have(FAM, row_dev_meas, F::MEAS), "EDGE_TYPES: a row's dev_meas is not the family's F::MEAS");
  static_assert(family_rows_have(FAM, row_dev_par, F::PAR), "EDGE_TYPES: a row's dev_par is not the family's F::PAR");
  static_assert(family_rows_have(FAM, row_DA, F::DA), "EDGE_TYPES: vertex_dim of a row's vtA is not the family's F::DA");
  static_assert(family_rows_have(FAM, row_DB, family_db<F>::value),
                "EDGE_TYPES: vertex_dim of a row's vtB is not the family's F::DB (0: unary)");
  return F{};
}

// the host-Jacobian families (any D, DA, DB): callers whose kernel does not exist for them guard with if constexpr
template <class F> struct is_hostj_type : std::false_type {};
template <int D, int DA, int DB> struct is_hostj_type<FamilyHostJ<D, DA, DB>> : std::true_type {};
template <int D, int DA> struct is_hostj_type<FamilyHostJUnary<D, DA>> : std::true_type {};

// the Sim3 projection families: no F::linearize (k_linearize_sim3_project takes F::jac_pose)
template <class F> struct is_sim3_project_type : std::false_type {};
template <bool INV> struct is_sim3_project_type<FamilySim3Project<INV>> : std::true_type {};

// host-Jacobian families: runtime (D, DA, DB) -> FamilyHostJ<D, DA, DB> (vertex dims 2, 3, 6 or 7, D = 1..7)
template <int D, int DA, class Fn>
static void hj_b(int DB, Fn& fn) {
  if (DB == 2) fn(FamilyHostJ<D, DA, 2>{});
  else if (DB == 3) fn(FamilyHostJ<D, DA, 3>{});
  else if (DB == 6) fn(FamilyHostJ<D, DA, 6>{});
  else if (DB == 7) fn(FamilyHostJ<D, DA, 7>{});
  else throw std::runtime_error("host-Jacobian edge: vertex dimension must be 2, 3, 6 or 7");
}
template <int D, class Fn>
static void hj_a(int DA, int DB, Fn& fn) {
  if (DA == 2) hj_b<D, 2>(DB, fn);
  else if (DA == 3) hj_b<D, 3>(DB, fn);
  else if (DA == 6) hj_b<D, 6>(DB, fn);
  else if (DA == 7) hj_b<D, 7>(DB, fn);
  else throw std::runtime_error("host-Jacobian edge: vertex dimension must be 2, 3, 6 or 7");
}
// unary families; host-Jacobian ones: runtime (D, DA) -> FamilyHostJUnary<D, DA>
template <int D, class Fn>
static void hju_a(int DA, Fn& fn) {
  if (DA == 2) fn(FamilyHostJUnary<D, 2>{});
  else if (DA == 3) fn(FamilyHostJUnary<D, 3>{});
  else if (DA == 6) fn(FamilyHostJUnary<D, 6>{});
  else if (DA == 7) fn(FamilyHostJUnary<D, 7>{});
  else throw std::runtime_error("host-Jacobian unary edge: vertex dimension must be 2, 3, 6 or 7");
}
template <class Fn>
static void unary_dispatch(int family, const EdgeArgs& a, Fn&& fn) {
  switch (family) {
    case FAM_U_SE2: fn(checked<FAM_U_SE2, FamilyUnarySE2>()); break;
    case FAM_U_SE2XY: fn(checked<FAM_U_SE2XY, FamilyUnarySE2XY>()); break;
    case FAM_U_XY: fn(checked<FAM_U_XY, FamilyUnaryXY>()); break;
    case FAM_U_SE3: fn(checked<FAM_U_SE3, FamilyUnarySE3>()); break;
    case FAM_U_XYZ: fn(checked<FAM_U_XYZ, FamilyUnaryXYZ>()); break;
    case FAM_U_POSE_ONLY: fn(checked<FAM_U_POSE_ONLY, FamilyPoseOnly>()); break;
    case FAM_U_STEREO_POSE_ONLY: fn(checked<FAM_U_STEREO_POSE_ONLY, FamilyStereoPoseOnly>()); break;
    case FAM_U_HOSTJ:
      switch (a.D) {
        case 1: hju_a<1>(a.DA, fn); break;
        case 2: hju_a<2>(a.DA, fn); break;
        case 3: hju_a<3>(a.DA, fn); break;
        case 4: hju_a<4>(a.DA, fn); break;
        case 5: hju_a<5>(a.DA, fn); break;
        case 6: hju_a<6>(a.DA, fn); break;
        case 7: hju_a<7>(a.DA, fn); break;
        default: throw std::runtime_error("host-Jacobian unary edge: error dimension must be 1..7");
      }
      break;
    default: throw std::runtime_error("unknown unary edge family");
  }
}
template <class Fn>
static void binary_dispatch(int family, const EdgeArgs& a, Fn&& fn);
// every family, for the kernels that only need F::error (chi2): binary or unary
template <class Fn>
static void family_dispatch(int family, const EdgeArgs& a, Fn&& fn) {
  if (is_unary_family(family)) unary_dispatch(family, a, fn);
  else binary_dispatch(family, a, fn);
}
template <class Fn>
static void binary_dispatch(int family, const EdgeArgs& a, Fn&& fn) {
  switch (family) {
    case FAM_BA: fn(checked<FAM_BA, FamilyBA>()); break;
    case FAM_BA_STEREO: fn(checked<FAM_BA_STEREO, FamilyStereo>()); break;
    case FAM_BA_UVU: fn(checked<FAM_BA_UVU, FamilyUVU>()); break;
    case FAM_SE3: fn(checked<FAM_SE3, FamilySE3>()); break;
    case FAM_SE2: fn(checked<FAM_SE2, FamilySE2>()); break;
    case FAM_SE2XY: fn(checked<FAM_SE2XY, FamilySE2XY>()); break;
    case FAM_SE3_XYZ: fn(checked<FAM_SE3_XYZ, FamilySE3XYZ>()); break;
    case FAM_SE3_XYZ_DEPTH: fn(checked<FAM_SE3_XYZ_DEPTH, FamilySE3XYZDepth>()); break;
    case FAM_SE3_XYZ_DISPARITY: fn(checked<FAM_SE3_XYZ_DISPARITY, FamilySE3XYZDisparity>()); break;
    case FAM_EXPMAP: fn(checked<FAM_EXPMAP, FamilyExpmap>()); break;
    case FAM_SBA_MONO: fn(checked<FAM_SBA_MONO, FamilySBAMono>()); break;
    case FAM_SBA_STEREO: fn(checked<FAM_SBA_STEREO, FamilySBAStereo>()); break;
    case FAM_SE3_OFFSET: fn(checked<FAM_SE3_OFFSET, FamilySE3Offset>()); break;
    case FAM_SE2_OFFSET: fn(checked<FAM_SE2_OFFSET, FamilySE2Offset>()); break;
    case FAM_SE2XY_BEARING: fn(checked<FAM_SE2XY_BEARING, FamilySE2XYBearing>()); break;
    case FAM_GICP: fn(checked<FAM_GICP, FamilyGICP>()); break;
    case FAM_VSC: fn(checked<FAM_VSC, FamilyVSC>()); break;
    case FAM_SIM3: fn(checked<FAM_SIM3, FamilySim3>()); break;
    case FAM_SIM3_PROJECT: fn(checked<FAM_SIM3_PROJECT, FamilySim3Project<false>>()); break;
    case FAM_SIM3_PROJECT_INVERSE: fn(checked<FAM_SIM3_PROJECT_INVERSE, FamilySim3Project<true>>()); break;
    case FAM_BAL: fn(checked<FAM_BAL, FamilyBAL>()); break;
    case FAM_HOSTJ:
      switch (a.D) {
        case 1: hj_a<1>(a.DA, a.DB, fn); break;
        case 2: hj_a<2>(a.DA, a.DB, fn); break;
        case 3: hj_a<3>(a.DA, a.DB, fn); break;
        case 4: hj_a<4>(a.DA, a.DB, fn); break;
        case 5: hj_a<5>(a.DA, a.DB, fn); break;
        case 6: hj_a<6>(a.DA, a.DB, fn); break;
        case 7: hj_a<7>(a.DA, a.DB, fn); break;
        default: throw std::runtime_error("host-Jacobian edge: error dimension must be 1..7");
      }
      break;
    default: throw std::runtime_error("unknown edge family");
  }
}

}  // namespace launch
}  // namespace g2ohip
