// qt_device_probe.hip — test-only kernels that call the elementary functions
// of csrc/ (qt_math.hpp, qt_device.hpp, qt_crtrig.hpp, qt_glibc.hpp) as they
// are compiled for gfx950, one call per lane (tests/test_gpu_device_math.py).
//
// Built twice from this source by the `probe` target of the package Makefile:
// libqtprobe_exact.so with HIPFLAGS (every kernel source but one) and
// libqtprobe_fast.so with HIPFLAGS + FASTFLAGS (qt_rollout_fast.hip).  It is
// not part of libquadtrack.so.  Nothing is restated here: every value written
// comes out of a production function.
//
// Launchers: (int64_t n, const double* in..., double* out, void* stream) -> int
// (0 ok, -1 invalid argument, -2 launch error).  Arrays are device pointers of
// n doubles; out holds its rows one after another, out[row * n + i].  A lane
// past n calls the function on a benign dummy argument and skips the store,
// so that functions with a wave-uniform branch (any_lane) run on whole waves,
// as they do in the rollout kernels.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qt_device.hpp"

namespace {

constexpr int kBlock = 256;

__device__ __forceinline__ int64_t lane_index() { return (int64_t)blockIdx.x * kBlock + threadIdx.x; }

// the device library's sqrt and the three rsq-based square roots
__global__ __launch_bounds__(kBlock) void k_sqrt(int64_t n, const double* x, double* out) {
  const int64_t i = lane_index();
  const bool live = i < n;
  const double v = live ? x[i] : 1.0;
  const double r0 = sqrt(v), r1 = qt::sqrt_noscale(v), r2 = qt::sqrt_pos(v), r3 = qt::sqrt_sum(v);
  if (!live) return;
  out[i] = r0, out[n + i] = r1, out[2 * n + i] = r2, out[3 * n + i] = r3;
}

// sqrt(s) > r and sqrt(s) <= r on squared values
__global__ __launch_bounds__(kBlock) void k_norm(int64_t n, const double* s, const double* r, double* out) {
  const int64_t i = lane_index();
  const bool live = i < n;
  const double sv = live ? s[i] : 0.0, rv = live ? r[i] : 1.0;
  const bool gt = qt::norm_gt(sv, rv);
  const bool le = qt::norm_le(sv, rv);
  if (!live) return;
  out[i] = gt ? 1.0 : 0.0, out[n + i] = le ? 1.0 : 0.0;
}

// constrain's speed clamp: the velocity after constrain<true> with max_velocity = r,
// and the squared speed dot3_blas forms
__global__ __launch_bounds__(kBlock) void k_constrain(int64_t n, const double* vx, const double* vy,
                                                      const double* vz, const double* r, double* out) {
  const int64_t i = lane_index();
  const bool live = i < n;
  qt_env_params e{};
  e.max_velocity = live ? r[i] : 1.0;
  e.max_angular_velocity = 1.0;
  double x[12] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  x[3] = live ? vx[i] : 0.0, x[4] = live ? vy[i] : 0.0, x[5] = live ? vz[i] : 0.0;
  const double s = qt::dot3_blas(x[3], x[4], x[5]);
  qt::constrain<true>(e, x);
  if (!live) return;
  out[i] = x[3], out[n + i] = x[4], out[2 * n + i] = x[5], out[3 * n + i] = s;
}

// wrap_angles of one lane's three angles, and py_mod_2pi of the first
__global__ __launch_bounds__(kBlock) void k_wrap(int64_t n, const double* a0, const double* a1, const double* a2,
                                                 double* out) {
  const int64_t i = lane_index();
  const bool live = i < n;
  double a[3] = {live ? a0[i] : 0.0, live ? a1[i] : 0.0, live ? a2[i] : 0.0};
  const double m = qt::py_mod_2pi(a[0], qt::kTwoPi);
  qt::wrap_angles(a);
  if (!live) return;
  out[i] = a[0], out[n + i] = a[1], out[2 * n + i] = a[2], out[3 * n + i] = m;
}

__global__ __launch_bounds__(kBlock) void k_clip(int64_t n, const double* v, const double* lo, const double* hi,
                                                 double* out) {
  const int64_t i = lane_index();
  if (i >= n) return;
  out[i] = qt::clipd(v[i], lo[i], hi[i]);
  out[n + i] = qt::clip_num(v[i], lo[i], hi[i]);
}

__global__ __launch_bounds__(kBlock) void k_add_product(int64_t n, const double* a, const double* b,
                                                        const double* c, double* out) {
  const int64_t i = lane_index();
  if (i >= n) return;
  out[i] = qt::add_product_rn(a[i], b[i], c[i]);
}

// the polynomial trig of qt_math.hpp: rows as the columns of the host probe of
// tests/test_math.py (fast s c, py_mod_2pi, small s c, tilt s c, rate s c,
// resid s cm, tiny s cm)
__global__ __launch_bounds__(kBlock) void k_trig(int64_t n, const double* x, double* out) {
  const int64_t i = lane_index();
  if (i >= n) return;
  const double a = x[i];
  double r[13];
  qt::fast_sincos(a, &r[0], &r[1]);
  r[2] = qt::py_mod_2pi(a, 6.283185307179586);
  qt::small_sincos(a, &r[3], &r[4]);
  qt::sincos_tilt(a, &r[5], &r[6]);
  qt::rate_sincos(a, &r[7], &r[8]);
  qt::resid_sincos(a, &r[9], &r[10]);
  qt::tiny_sincos(a, &r[11], &r[12]);
#pragma unroll
  for (int k = 0; k < 13; ++k) out[k * n + i] = r[k];
}

__global__ __launch_bounds__(kBlock) void k_rotate(int64_t n, const double* s0, const double* c0, const double* sd,
                                                   const double* cm, double* out) {
  const int64_t i = lane_index();
  if (i >= n) return;
  double s, c;
  qt::rotate_cm(s0[i], c0[i], sd[i], cm[i], &s, &c);
  out[i] = s, out[n + i] = c;
}

__global__ __launch_bounds__(kBlock) void k_rk4(int64_t n, const double* lam, const double* h, const double* y,
                                                const double* f0, const double* f1, const double* f2,
                                                const double* f3, double* out) {
  const int64_t i = lane_index();
  if (i >= n) return;
  const double f[4] = {f0[i], f1[i], f2[i], f3[i]};
  double o[5];
  qt::rk4_linear(lam[i], h[i], y[i], f, o);
#pragma unroll
  for (int k = 0; k < 5; ++k) out[k * n + i] = o[k];
}

__global__ __launch_bounds__(kBlock) void k_cr(int64_t n, const double* x, double* out) {
  const int64_t i = lane_index();
  if (i >= n) return;
  double s, c;
  qt::cr_sincos(x[i], &s, &c);
  out[i] = s, out[n + i] = c;
}

__global__ __launch_bounds__(kBlock) void k_glibc(int64_t n, const double* x, double* out) {
  const int64_t i = lane_index();
  if (i >= n) return;
  out[i] = qt::glibc::sin(x[i]);
  out[n + i] = qt::glibc::cos(x[i]);
  out[2 * n + i] = qt::glibc::pow2(x[i]);
}

// figure8_recip with center 0: p[0], p[1], v[0], v[1] (amplitude 1 and ct 1 give p[0] = the reciprocal)
__global__ __launch_bounds__(kBlock) void k_figure8(int64_t n, const double* om, const double* st, const double* ct,
                                                    const double* amp, double* out) {
  const int64_t i = lane_index();
  if (i >= n) return;
  qt_env_params e{};
  e.amplitude = amp[i];
  qt::Target o;
  qt::figure8_recip(e, om[i], st[i], ct[i], o);
  out[i] = o.p[0], out[n + i] = o.p[1], out[2 * n + i] = o.v[0], out[3 * n + i] = o.v[1];
}

template <typename K, typename... A>
int launch(K kernel, int64_t n, void* stream, A... args) {
  if (n < 0 || n > (int64_t)1 << 30) return -1;
  if (n == 0) return 0;
  const unsigned grid = (unsigned)((n + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, n, args...);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace

extern "C" {

int qtp_sqrt(int64_t n, const double* x, double* out, void* stream) { return launch(k_sqrt, n, stream, x, out); }
int qtp_norm(int64_t n, const double* s, const double* r, double* out, void* stream) {
  return launch(k_norm, n, stream, s, r, out);
}
int qtp_constrain(int64_t n, const double* vx, const double* vy, const double* vz, const double* r, double* out,
                  void* stream) {
  return launch(k_constrain, n, stream, vx, vy, vz, r, out);
}
int qtp_wrap(int64_t n, const double* a0, const double* a1, const double* a2, double* out, void* stream) {
  return launch(k_wrap, n, stream, a0, a1, a2, out);
}
int qtp_clip(int64_t n, const double* v, const double* lo, const double* hi, double* out, void* stream) {
  return launch(k_clip, n, stream, v, lo, hi, out);
}
int qtp_add_product(int64_t n, const double* a, const double* b, const double* c, double* out, void* stream) {
  return launch(k_add_product, n, stream, a, b, c, out);
}
int qtp_trig(int64_t n, const double* x, double* out, void* stream) { return launch(k_trig, n, stream, x, out); }
int qtp_rotate(int64_t n, const double* s0, const double* c0, const double* sd, const double* cm, double* out,
               void* stream) {
  return launch(k_rotate, n, stream, s0, c0, sd, cm, out);
}
int qtp_rk4(int64_t n, const double* lam, const double* h, const double* y, const double* f0, const double* f1,
            const double* f2, const double* f3, double* out, void* stream) {
  return launch(k_rk4, n, stream, lam, h, y, f0, f1, f2, f3, out);
}
int qtp_cr(int64_t n, const double* x, double* out, void* stream) { return launch(k_cr, n, stream, x, out); }
int qtp_glibc(int64_t n, const double* x, double* out, void* stream) { return launch(k_glibc, n, stream, x, out); }
int qtp_figure8(int64_t n, const double* om, const double* st, const double* ct, const double* amp, double* out,
                void* stream) {
  return launch(k_figure8, n, stream, om, st, ct, amp, out);
}

}  // extern "C"
