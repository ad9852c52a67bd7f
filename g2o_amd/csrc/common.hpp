// Shared host helpers for libg2o_hip: HIP error handling and device buffers.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

namespace g2ohip {

struct DeviceError : std::runtime_error {
  using std::runtime_error::runtime_error;
};
// a refusal with a reason: the C entry point returns `code` (G2OHIP_ERR_ARG, G2OHIP_ERR_UNSUPPORTED) and
// g2ohip_last_error the message
struct StatusError : std::runtime_error {
  int code;
  StatusError(int c, const std::string& what) : std::runtime_error(what), code(c) {}
};

#define HIP_CHECK(expr)                                                                                  \
  do {                                                                                                   \
    hipError_t _e = (expr);                                                                              \
    if (_e != hipSuccess)                                                                                \
      throw ::g2ohip::DeviceError(std::string(#expr) + " failed: " + hipGetErrorString(_e) + " @" +     \
                                  __FILE__ + ":" + std::to_string(__LINE__));                           \
  } while (0)

#define KERNEL_CHECK() HIP_CHECK(hipGetLastError())

// RAII device buffer (hipMalloc'd, never host-mapped).
template <typename T>
class DevBuf {
 public:
  DevBuf() = default;
  explicit DevBuf(size_t n) { resize(n); }
  ~DevBuf() { release(); }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { release(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
    return *this;
  }
  void resize(size_t n) {
    if (n == n_) return;
    release();
    if (n) HIP_CHECK(hipMalloc(&p_, n * sizeof(T)));
    n_ = n;
  }
  void release() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
    n_ = 0;
  }
  T* get() const { return p_; }
  size_t size() const { return n_; }
  size_t bytes() const { return n_ * sizeof(T); }
  // structure-time upload: completes before returning (the host source may be a temporary)
  void upload(const T* h, size_t n, hipStream_t s) {
    resize(n);
    if (n) {
      HIP_CHECK(hipMemcpyAsync(p_, h, n * sizeof(T), hipMemcpyHostToDevice, s));
      HIP_CHECK(hipStreamSynchronize(s));
    }
  }
  void upload(const std::vector<T>& v, hipStream_t s) { upload(v.data(), v.size(), s); }
  void download(T* h, size_t n, hipStream_t s) const {
    if (n) HIP_CHECK(hipMemcpyAsync(h, p_, n * sizeof(T), hipMemcpyDeviceToHost, s));
  }
  void zero(hipStream_t s) {
    if (n_) HIP_CHECK(hipMemsetAsync(p_, 0, n_ * sizeof(T), s));
  }

 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};

// A launch-time A/B knob read from the environment: cached per call site, re-read after every structure build
// (Engine::build_structure bumps the epoch), so a process can switch schedules between optimizers (the parity tests
// do) without a getenv per launch.
inline std::atomic<int>& knob_epoch() {
  static std::atomic<int> e{0};
  return e;
}
struct EnvKnob {
  const char* name;
  int dflt;
  // (epoch + 1) << 32 | value in one word, so a reader on another host thread never pairs a new epoch with an old
  // value (0: never read). An unset or EMPTY variable gives the default (not atoi("") = 0).
  std::atomic<unsigned long long> state{0};
  EnvKnob(const char* n, int d) : name(n), dflt(d) {}
  int get() {
    const unsigned long long e = (unsigned long long)(unsigned)knob_epoch().load(std::memory_order_acquire) + 1;
    unsigned long long st = state.load(std::memory_order_acquire);
    if ((st >> 32) != e) {
      const char* v = std::getenv(name);
      const int x = v && *v ? std::atoi(v) : dflt;
      st = e << 32 | (unsigned)x;
      state.store(st, std::memory_order_release);
    }
    return (int)(unsigned)(st & 0xffffffffULL);
  }
};

inline unsigned grid_for(size_t n, unsigned block) { return (unsigned)((n + block - 1) / block); }

// t^3 with the products' rounding errors carried (t^2 = p + e exactly by FMA, t^3 = p t + (fma error + e t)) and one
// final rounding: within ~0.5 ulp of the exact cube. The reference computes std::pow(t, 3) with glibc, which is accurate
// to < 1 ulp but NOT guaranteed correctly rounded, and the device has no glibc pow. So lambda parity with the reference
// is within 1 ulp of the factor per accepted trial, not bitwise (tests/test_host.py::test_lm_scale_factor_matches_pow
// checks the 1-ulp bound; the lambda traces of the full-size tests allow it). What this buys is that the host loop and
// the device decision (k_sum_final2_decide) run the same arithmetic and so take bitwise identical lambda paths.
__host__ __device__ inline double cube_rn(double t) {
  const double p = t * t, e = fma(t, t, -p);
  const double h = p * t, l = fma(p, t, -h) + e * t;
  return h + l;
}
// the accepted LM trial's lambda factor (optimization_algorithm_levenberg.cpp:127-136): alpha = 1 - (2 rho - 1)^3,
// clipped to [goodStepLowerScale, goodStepUpperScale] = [1/3, 2/3]; host loop and device decision share it
__host__ __device__ inline double lm_scale_factor(double rho) {
  double alpha = 1. - cube_rn(2 * rho - 1);
  alpha = alpha < 2. / 3. ? alpha : 2. / 3.;
  return 1. / 3. > alpha ? 1. / 3. : alpha;
}

// OptimizationAlgorithmDogleg's two scalar decisions, shared by the device kernels (k_dl_blend, k_dl_decide) and the
// host (g2ohip_dogleg_blend, g2ohip_dogleg_next_delta). Products and sums are rounded one by one (no contraction into
// FMAs), so host and device take the same branch on the same doubles.
enum DoglegStep { DL_STEP_UNDEFINED = 0, DL_STEP_SD = 1, DL_STEP_GN = 2, DL_STEP_DL = 3 };  // the reference's enum order
// step choice and blend (optimization_algorithm_dogleg.cpp:153-175): hdl = coef[0] hsd + coef[1] hgn from |hgn|, |hsd|,
// hsd.hsd, c = hsd.(hgn - hsd), |hgn - hsd|^2 and delta; hdl = hsd + beta (hgn - hsd) is coef = (1 - beta, beta)
__host__ __device__ inline int dogleg_blend(double hgn_norm, double hsd_norm, double hsd_sq, double c, double bma_sq,
                                            double delta, double coef[2]) {
#pragma clang fp contract(off)
  if (hgn_norm < delta) {  // :153-155
    coef[0] = 0.0;
    coef[1] = 1.0;
    return DL_STEP_GN;
  }
  if (hsd_norm > delta) {  // :157-159
    coef[0] = delta / hsd_norm;
    coef[1] = 0.0;
    return DL_STEP_SD;
  }
  double beta;  // :161-173
  if (c <= 0.) {
    beta = (-c + sqrt(c * c + bma_sq * (delta * delta - hsd_sq))) / bma_sq;
  } else {
    beta = (delta * delta - hsd_sq) / (c + sqrt(c * c + bma_sq * (delta * delta - hsd_sq)));
  }
  coef[0] = 1.0 - beta;
  coef[1] = beta;
  return DL_STEP_DL;
}
// trust-region update (:199-203)
__host__ __device__ inline double dogleg_next_delta(double delta, double rho, double hdl_norm) {
#pragma clang fp contract(off)
  if (rho > 0.75) {
    const double t = 3 * hdl_norm;
    return delta < t ? t : delta;  // std::max(delta, t)
  }
  if (rho < 0.25) return delta * 0.5;
  return delta;
}

}  // namespace g2ohip
