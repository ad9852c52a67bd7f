// Pair-major assembly for registration graphs (Edge_V_V_GICP): a handful of poses, 10^4..10^6 edges per pose pair.
//
//   k_linearize_pairs  one wave per chunk (<= 64 edges of one vertex pair), one lane per edge. The lane linearizes its
//                      edge as k_linearize does (same family code, same rho' weighting), stages its contribution to the
//                      pair's first side (27 doubles), to the pair's 6x6 off-diagonal block (36) and to the second
//                      side (27) in the wave's LDS image, one after the other; after each staging lane k sums entry k
//                      over the chunk's rows in row order. One 90-double partial per chunk leaves the wave, with
//                      coalesced stores: 720 B per 64 edges where the slot path writes 720 B per edge.
//   k_pair_reduce      one workgroup (16 waves) per pair: each wave sums a contiguous run of the pair's chunk
//                      partials in order, the wave sums are added in wave order. The off-diagonal block goes straight
//                      into Hpp's block storage, the two side sums into the pair's two slots, which
//                      k_vertex_reduce(_wide) then sums per vertex exactly as it sums per-edge slots.
// Every sum has one owner and a fixed order (no atomics): two runs are bitwise equal.
#include <hip/hip_runtime.h>

#include <stdexcept>

#include "common.hpp"
#include "device_types.hpp"
#include "device_util.hpp"
#include "kernels.hpp"

namespace g2ohip {
using namespace dev;

namespace {
// order one wave's LDS writes before its reads of another lane's words (as in kernels.hip)
__device__ __forceinline__ void pair_wave_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}
// lane k (< n) sums entry k of the image's rows 0..cnt-1 in row order and stores it
__device__ __forceinline__ void pair_rows_sum(const double* sw, int stride, int n, int cnt, int lane,
                                              double* __restrict__ out) {
  if (lane < n) {
    double s = 0;
#pragma unroll 8
    for (int r = 0; r < cnt; ++r) s += sw[r * stride + lane];
    out[lane] = s;
  }
}
}  // namespace

// chunks: (first edge, edges, pair, flags); flags bit 0: both ends of the pair are free (else exactly one is, and the
// pair has a first side only). The pair's first side is the end with the smaller hessian index (the row of its block
// in Hpp's upper triangle), or its only free end. An edge may name the pair's ends in either order: `swp` lanes take
// the first side from their vertex 1.
template <class F>
__global__ void __launch_bounds__(256)
    k_linearize_pairs(EdgeData d, int nchunks, const int4* __restrict__ chunks, const int* __restrict__ h0,
                      const int* __restrict__ h1, double* __restrict__ partial) {
  constexpr int D = F::D, DA = F::DA, DB = F::DB;
  static_assert(DA == DB, "a pair's two ends have one dimension");
  constexpr int SA = DA * (DA + 1) / 2 + DA, SH = DA * DB, SP = 2 * SA + SH;
  static_assert(SH <= 64 && SA <= 64, "one lane per entry");
  __shared__ __attribute__((aligned(16))) double stage[4][64 * SH];
  const int tid = threadIdx.x, lane = tid & 63;
  const int c = blockIdx.x * 4 + (tid >> 6);
  if (c >= nchunks) return;  // wave-uniform
  const int4 ch = chunks[c];
  const int cnt = ch.y, e = ch.x + lane;
  const bool in = lane < cnt, both = (ch.w & 1) != 0;
  double* sw = stage[tid >> 6];
  double* out = partial + (size_t)c * SP;
  double err[D], P[D * DA], Q[D * DB], Om[D * D];
  if (in) {
    const int hA = h0[d.v0[e]], hB = h1[d.v1[e]];
    const bool swp = both ? hA > hB : hA < 0;
    double A[D * DA], B[D * DB];
    F::linearize(d, e, err, A, B);
    family_info<F>(d, e, Om);
    if (d.rk) {  // as k_linearize: Omega and omega_r scaled by rho'
      double chi = 0;
#pragma unroll
      for (int i = 0; i < D; ++i) {
        double r = 0;
#pragma unroll
        for (int j = 0; j < D; ++j) r += Om[i * D + j] * err[j];
        chi += err[i] * r;
      }
      double r0, r1;
      robustify(d.rk, d.rk_delta, chi, r0, r1);
#pragma unroll
      for (int i = 0; i < D * D; ++i) Om[i] *= r1;
    }
#pragma unroll
    for (int k = 0; k < D * DA; ++k) {
      P[k] = swp ? B[k] : A[k];
      Q[k] = swp ? A[k] : B[k];
    }
  }
  double wr[D];
#pragma unroll
  for (int r = 0; r < D; ++r) {
    double s = 0;
#pragma unroll
    for (int cc = 0; cc < D; ++cc) s += Om[r * D + cc] * err[cc];
    wr[r] = -s;
  }
  double PtO[DA * D];  // P^T Omega
#pragma unroll
  for (int i = 0; i < DA; ++i)
#pragma unroll
    for (int cc = 0; cc < D; ++cc) {
      double s = 0;
#pragma unroll
      for (int r = 0; r < D; ++r) s += P[r * DA + i] * Om[r * D + cc];
      PtO[i * D + cc] = s;
    }
  // first side: packed upper col-major P^T Omega P, then P^T (-Omega e)
  if (in) {
    double* o = sw + lane * SA;
    int k = 0;
#pragma unroll
    for (int cc = 0; cc < DA; ++cc)
#pragma unroll
      for (int r = 0; r <= cc; ++r) {
        double s = 0;
#pragma unroll
        for (int t = 0; t < D; ++t) s += PtO[r * D + t] * P[t * DA + cc];
        o[k++] = s;
      }
#pragma unroll
    for (int i = 0; i < DA; ++i) {
      double s = 0;
#pragma unroll
      for (int r = 0; r < D; ++r) s += P[r * DA + i] * wr[r];
      o[k++] = s;
    }
  }
  pair_wave_sync();
  pair_rows_sum(sw, SA, SA, cnt, lane, out);
  if (!both) return;  // wave-uniform: the other end is fixed, neither its side nor the block is formed
  pair_wave_sync();
  if (in) {  // the block (first side, second side), DA x DB col-major
    double* H = sw + lane * SH;
#pragma unroll
    for (int j = 0; j < DB; ++j)
#pragma unroll
      for (int i = 0; i < DA; ++i) {
        double s = 0;
#pragma unroll
        for (int r = 0; r < D; ++r) s += PtO[i * D + r] * Q[r * DB + j];
        H[j * DA + i] = s;
      }
  }
  pair_wave_sync();
  pair_rows_sum(sw, SH, SH, cnt, lane, out + SA);
  pair_wave_sync();
  if (in) {
    double QtO[DB * D];
#pragma unroll
    for (int j = 0; j < DB; ++j)
#pragma unroll
      for (int cc = 0; cc < D; ++cc) {
        double s = 0;
#pragma unroll
        for (int r = 0; r < D; ++r) s += Q[r * DB + j] * Om[r * D + cc];
        QtO[j * D + cc] = s;
      }
    double* o = sw + lane * SA;
    int k = 0;
#pragma unroll
    for (int cc = 0; cc < DB; ++cc)
#pragma unroll
      for (int r = 0; r <= cc; ++r) {
        double s = 0;
#pragma unroll
        for (int t = 0; t < D; ++t) s += QtO[r * D + t] * Q[t * DB + cc];
        o[k++] = s;
      }
#pragma unroll
    for (int j = 0; j < DB; ++j) {
      double s = 0;
#pragma unroll
      for (int r = 0; r < D; ++r) s += Q[r * DB + j] * wr[r];
      o[k++] = s;
    }
  }
  pair_wave_sync();
  pair_rows_sum(sw, SA, SA, cnt, lane, out + SA + SH);
}

// prange[p] = the pair's chunk range; pdst[p] = offset of its block in H, or -1 when one end is fixed (first side only).
// NW waves per workgroup: a pair of 32768 edges has 512 chunks, 32 per wave at NW = 16 (four waves took 128 dependent
// rounds each: 0.079 ms for 32 such pairs, more than their linearize launch)
template <int DIM, int NW>
__global__ void __launch_bounds__(64 * NW)
    k_pair_reduce(int npairs, const int2* __restrict__ prange, const long long* __restrict__ pdst,
                  const double* __restrict__ partial, double* __restrict__ slots, double* __restrict__ H) {
  constexpr int SA = DIM * (DIM + 1) / 2 + DIM, SH = DIM * DIM, SP = 2 * SA + SH;
  static_assert(SP <= 128, "two entries per lane");
  __shared__ double red[NW][SP];
  const int p = blockIdx.x;
  if (p >= npairs) return;  // workgroup-uniform
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int2 rg = prange[p];
  const long long dst = pdst[p];
  const int nent = dst >= 0 ? SP : SA;  // entries that were formed
  const int per = (rg.y - rg.x + NW - 1) / NW;
  const int c0 = min(rg.x + w * per, rg.y), c1 = min(c0 + per, rg.y);
  const int k0 = lane, k1 = lane + 64;
  double a0 = 0, a1 = 0;
#pragma unroll 4  // (the loads of four chunks in flight; the sums stay in chunk order)
  for (int c = c0; c < c1; ++c) {
    const double* q = partial + (size_t)c * SP;
    if (k0 < nent) a0 += q[k0];
    if (k1 < nent) a1 += q[k1];
  }
  if (k0 < SP) red[w][k0] = a0;
  if (k1 < SP) red[w][k1] = a1;
  __syncthreads();
  if (tid >= nent) return;
  double t = red[0][tid];
#pragma unroll
  for (int j = 1; j < NW; ++j) t += red[j][tid];  // wave order
  if (tid < SA) slots[(size_t)(2 * p) * SA + tid] = t;
  else if (tid < SA + SH) H[dst + tid - SA] = t;
  else slots[(size_t)(2 * p + 1) * SA + tid - SA - SH] = t;
}

namespace launch {
void linearize_pairs(int family, const EdgeArgs& a, int nchunks, const int4* chunks, const int* h0, const int* h1,
                     double* partial, hipStream_t s) {
  if (nchunks <= 0) return;
  if (family != FAM_GICP) throw std::runtime_error("linearize_pairs: the pair-major assembly takes Edge_V_V_GICP only");
  const EdgeData d{a.v0, a.v1, a.meas, a.info, a.params, a.s0, a.s1, a.rk, a.rk_delta, a.ue};
  hipLaunchKernelGGL(k_linearize_pairs<FamilyGICP>, (nchunks + 3) / 4, 256, 0, s, d, nchunks, chunks, h0, h1, partial);
  KERNEL_CHECK();
}
void pair_reduce(int dim, int npairs, const int2* prange, const long long* pdst, const double* partial, double* slots,
                 double* H, hipStream_t s) {
  if (npairs <= 0) return;
  if (dim != 6) throw std::runtime_error("pair_reduce: pose blocks must be 6x6");
  hipLaunchKernelGGL((k_pair_reduce<6, 16>), npairs, 1024, 0, s, npairs, prange, pdst, partial, slots, H);
  KERNEL_CHECK();
}
}  // namespace launch
}  // namespace g2ohip
