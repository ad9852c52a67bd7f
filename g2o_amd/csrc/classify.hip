// Per-edge chi2, depth test and outlier classification of every edge of one type (Edge::chi2, isDepthPositive and
// setLevel of the pose-optimisation / local-BA loops, DESIGN.md "Edge levels"):
//
//   k_classify        one lane per edge over the set's all-edges view (insertion order, inactive edges included):
//                     F::error, the raw quadratic form e^T Omega e in k_error's operation order (no robustify), the
//                     camera-frame z of the projection families, and with classification on the edge's new level and
//                     the block's three counts (wave ballots and popcounts, the waves summed in order).
//   k_classify_final  the per-block counts into the three totals. No atomics: levels and counts repeat run to run.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <type_traits>

#include "../../include/g2o_hip.h"
#include "common.hpp"
#include "device_types.hpp"
#include "family_dispatch.hpp"
#include "kernels.hpp"

namespace g2ohip {
using namespace dev;

namespace {
// the families with isDepthPositive (types_six_dof_expmap.h): their depth(d, e, err) returns z beside the error
template <class F> struct has_depth : std::false_type {};
template <> struct has_depth<FamilyBA> : std::true_type {};
template <> struct has_depth<FamilyStereo> : std::true_type {};
template <> struct has_depth<FamilyPoseOnly> : std::true_type {};
template <> struct has_depth<FamilyStereoPoseOnly> : std::true_type {};

constexpr int CL_BLOCK = 256, CL_WAVES = CL_BLOCK / 64;
}  // namespace

template <class F>
__global__ void __launch_bounds__(CL_BLOCK) k_classify(EdgeData d, int ne, launch::ClassifyArgs c) {
  const int e = blockIdx.x * CL_BLOCK + threadIdx.x;
  const bool valid = e < ne;
  double s = 0, z = 1;
  if (valid) {
    double err[F::D];
    if constexpr (has_depth<F>::value) z = F::depth(d, e, err);
    else F::error(d, e, err);
    double Om[F::D * F::D];
    family_info<F>(d, e, Om);
#pragma unroll
    for (int i = 0; i < F::D; ++i) {
      double r = 0;
#pragma unroll
      for (int j = 0; j < F::D; ++j) r += Om[i * F::D + j] * err[j];
      s += err[i] * r;
    }
    c.chi[e] = s;
    if (c.depth) c.depth[e] = z > 0 ? 1 : 0;
  }
  if (!c.level) return;  // (uniform: edge_chi2 alone)
  // the callers' test as they write it: a NaN chi2 is not above the threshold
  const bool over = valid && s > c.chi_max;
  const bool behind = valid && c.check_depth && !(z > 0);
  const bool bad = over || behind;
  if (valid) {
    const int nl = bad ? c.outlier : c.inlier;
    if (nl != G2OHIP_LEVEL_KEEP) c.level[e] = nl;
  }
  __shared__ int cnt[CL_WAVES][3];
  const int n0 = __popcll(__ballot(over)), n1 = __popcll(__ballot(behind)), n2 = __popcll(__ballot(bad));
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    cnt[wave][0] = n0;
    cnt[wave][1] = n1;
    cnt[wave][2] = n2;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    long long t = 0;
#pragma unroll
    for (int w = 0; w < CL_WAVES; ++w) t += cnt[w][threadIdx.x];
    c.part[(size_t)blockIdx.x * 3 + threadIdx.x] = t;
  }
}

// counts[k] = sum over the blocks of part[3 b + k]: thread t takes blocks t, t + 256, ..., then a tree over the threads
__global__ void __launch_bounds__(CL_BLOCK) k_classify_final(const long long* __restrict__ part, int nb,
                                                              long long* __restrict__ counts) {
  __shared__ long long sh[3][CL_BLOCK];
  long long t[3] = {0, 0, 0};
  for (int b = threadIdx.x; b < nb; b += CL_BLOCK)
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] += part[(size_t)b * 3 + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) sh[k][threadIdx.x] = t[k];
  __syncthreads();
  for (int m = CL_BLOCK / 2; m > 0; m >>= 1) {
    if ((int)threadIdx.x < m)
#pragma unroll
      for (int k = 0; k < 3; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + m];
    __syncthreads();
  }
  if (threadIdx.x < 3) counts[threadIdx.x] = sh[threadIdx.x][0];
}

namespace launch {
int classify_blocks(int ne) { return (int)grid_for((size_t)(ne > 0 ? ne : 1), CL_BLOCK); }

void classify(int family, const EdgeArgs& a, int ne, const ClassifyArgs& c, hipStream_t s) {
  if (ne <= 0) {
    if (c.level) HIP_CHECK(hipMemsetAsync(c.counts, 0, sizeof(long long) * 3, s));
    return;
  }
  if (c.level && (!c.part || !c.counts)) throw std::runtime_error("classify: no count buffers");
  const EdgeData d{a.v0, a.v1, a.meas, a.info, a.params, a.s0, a.s1, 0, 1.0, a.ue};  // raw chi2: no robust kernel
  auto go = [&](auto fam) {
    using F = decltype(fam);
    if constexpr (is_hostj_type<F>::value) {  // (no k_classify exists for them)
      throw std::runtime_error("classify: no device family (host-Jacobian edges hold their errors on the host)");
    } else {
      if ((c.depth || c.check_depth) && !has_depth<F>::value)
        throw std::runtime_error("classify: the edge family has no depth test");
      hipLaunchKernelGGL(k_classify<F>, classify_blocks(ne), CL_BLOCK, 0, s, d, ne, c);
    }
  };
  // (the binary families first: the order the kernels are instantiated in, and so laid out in the code object)
  if (!is_unary_family(family)) binary_dispatch(family, a, go);
  else unary_dispatch(family, a, go);
  KERNEL_CHECK();
  if (c.level) {
    hipLaunchKernelGGL(k_classify_final, 1, CL_BLOCK, 0, s, c.part, classify_blocks(ne), c.counts);
    KERNEL_CHECK();
  }
}
}  // namespace launch
}  // namespace g2ohip
