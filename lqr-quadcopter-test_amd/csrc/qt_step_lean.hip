// qt_step_lean.hip — the per-step API on lean frames (include/quadtrack.h,
// ABI 10): the kernels of qt_step.hip with the frame cut down to what is
// state.
//
// A full frame (qt_frame_row) is 229 B per episode, and a closed-loop step on
// it moves 462 B per env-step (reads state, target, time, counters; writes
// the frame and the command).  Most of that is derived: the target
// observation and the time are functions of (pattern, step count), the
// tracking error is -reward, the ratio is on / step.  A lean frame
// (qt_lean_row) keeps the 12 state rows, the reward, three int32 counters and
// the flags: 121 B, 286 B per closed-loop env-step.  What a caller asks for
// beyond that is built by lean_expand_kernel into a full frame, once.
//
// Time comes from the step count through one shared table (quadtrack.h "Time
// table"): ttab[step] is bitwise the time the full frame carries, so the
// target formed here at ttab[step] is bitwise the target the full-frame step
// stored at its `t + dt`.  The step body is qt_step.hpp's env_step_into, the
// same source the full frame runs: results are equal bit for bit
// (tests/test_gpu_lean_step.py).
//
// Bound: HBM at large batches.  One lane per episode, every row access a
// coalesced wave access; no LDS, no barriers.  A periodic target is now
// evaluated twice per step (at t for the controller, at t + dt for the
// reward) where the full frame loads six rows instead: arithmetic for bytes.
// The table reads (ttab[step], ttab[step + 1]) wait for the counter load, a
// second memory latency that a small, latency-bound batch pays.
#include "qt_step.hpp"

using namespace qts;

namespace {

struct LeanDev {
  double* f;
  int32_t* c;
  int8_t* b;
};

__device__ __forceinline__ LeanDev lean_of(const void* base, int64_t n) {
  double* f = static_cast<double*>(const_cast<void*>(base));
  int32_t* c = reinterpret_cast<int32_t*>(f + QT_LR_ROWS * n);
  return LeanDev{f, c, reinterpret_cast<int8_t*>(c + QT_FC_ROWS * n)};
}

// An episode that is done and frozen carries its lean frame over unchanged.
__device__ __forceinline__ void copy_column(const LeanDev& I, const LeanDev& O, int64_t n, int64_t ep) {
#pragma unroll
  for (int r = 0; r < QT_LR_ROWS; ++r) O.f[r * n + ep] = I.f[r * n + ep];
#pragma unroll
  for (int r = 0; r < QT_FC_ROWS; ++r) O.c[r * n + ep] = I.c[r * n + ep];
#pragma unroll
  for (int r = 0; r < QT_FB_ROWS; ++r) O.b[r * n + ep] = I.b[r * n + ep];
}

__device__ __forceinline__ Counts load_counts(const LeanDev& I, int64_t n, int64_t ep) {
  return Counts{I.c[QT_FC_STEP * n + ep], I.c[QT_FC_VIOLATIONS * n + ep], I.c[QT_FC_ON_TARGET * n + ep]};
}

// ttab[step], the index clamped into the table (quadtrack.h "Time table").
__device__ __forceinline__ double time_at(const double* __restrict__ ttab, int64_t len, int64_t step) {
  const int64_t i = step < 0 ? 0 : (step < len ? step : len - 1);
  return ttab[i];
}

// env_step_into's stores into the lean frame (qt_step.hpp): the state, the
// reward, the counters and the flags are kept; the target, the time, the
// tracking error and the ratio are not (lean_expand_kernel rebuilds them).
__device__ __forceinline__ void store_early(const LeanDev& O, int64_t n, int64_t ep, const Target&, double,
                                            int64_t step) {
  O.c[QT_FC_STEP * n + ep] = (int32_t)step;
}

__device__ __forceinline__ void store_late(const LeanDev& O, int64_t n, int64_t ep, const double* x, double err,
                                           double, const Counts& k, int term, bool on, bool viol, bool success) {
#pragma unroll
  for (int i = 0; i < 12; ++i) O.f[(QT_LR_X + i) * n + ep] = x[i];
  O.f[QT_LR_REWARD * n + ep] = -err;
  O.c[QT_FC_VIOLATIONS * n + ep] = (int32_t)k.viol;
  O.c[QT_FC_ON_TARGET * n + ep] = (int32_t)k.on;
  O.b[QT_FB_DONE * n + ep] = term != QT_TERM_RUNNING;
  O.b[QT_FB_ON_TARGET * n + ep] = on;
  O.b[QT_FB_VIOLATION * n + ep] = viol;
  O.b[QT_FB_SUCCESS * n + ep] = success;
  O.b[QT_FB_TERM * n + ep] = (int8_t)term;
}

// ------------------------------------------------------------------ reset

__global__ __launch_bounds__(kBlock) void lean_reset_kernel(qt_env_params e, BatchDev b,
                                                            const double* __restrict__ off, void* out) {
  const int64_t ep = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t n = b.n;
  if (ep >= n) return;
  const LeanDev O = lean_of(out, n);
  const int motion = motion_of(b, e, ep);
  const Pattern pt = pattern_of(b, e, motion, ep);
  Target tg;
  target_state<true>(e, motion, pt, 0.0, tg);  // quadcopter_env.py:133-139
  double p[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    p[i] = tg.p[i] + off[i * n + ep];
    O.f[(QT_LR_X + i) * n + ep] = p[i];
  }
#pragma unroll
  for (int i = 3; i < 12; ++i) O.f[(QT_LR_X + i) * n + ep] = 0.0;
  const double err = sqrt(dot3_blas(p[0] - tg.p[0], p[1] - tg.p[1], p[2] - tg.p[2]));
  O.f[QT_LR_REWARD * n + ep] = -err;
#pragma unroll
  for (int r = 0; r < QT_FC_ROWS; ++r) O.c[r * n + ep] = 0;
#pragma unroll
  for (int r = 0; r < QT_FB_ROWS; ++r) O.b[r * n + ep] = 0;
}

// ----------------------------------------------------------- open-loop step

template <bool FREEZE>
__global__ __launch_bounds__(kBlock) void lean_step_kernel(qt_env_params e, BatchDev b,
                                                           const double* __restrict__ ttab, int64_t len,
                                                           const void* in, qt_view a, void* out, int inplace) {
  const int64_t ep = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t n = b.n;
  if (ep >= n) return;
  const LeanDev I = lean_of(in, n), O = lean_of(out, n);
  // every load before the first data-dependent branch
  const bool done = FREEZE && I.b[QT_FB_DONE * n + ep];
  double x[12], u[4];
#pragma unroll
  for (int i = 0; i < 12; ++i) x[i] = I.f[(QT_LR_X + i) * n + ep];
#pragma unroll
  for (int i = 0; i < 4; ++i) u[i] = view_at(a, i, ep);
  const Counts k = load_counts(I, n, ep);
  const EpisodeIn ei = episode_in(e, b, ep);
  const double t_next = time_at(ttab, len, k.step + 1);  // the table holds the same t + dt
  if (done) {
    if (!inplace) copy_column(I, O, n, ep);
    return;
  }
  env_step_into(e, ei, n, ep, x, t_next, k, u, O);
}

// ---------------------------------------------------- closed-loop step

// compute_action on lean frame I's observation, then env.step into lean frame
// O.  Reads 12 doubles, 3 int32 counters, the done flag and the pattern per
// episode, writes the lean frame (121 B) and the action.
template <int KC, bool FF, bool KS, bool FREEZE>
__global__ __launch_bounds__(kBlock) void lean_closed_step_kernel(qt_env_params e, qt_ctrl_params c, BatchDev b,
                                                                  const double* __restrict__ ttab, int64_t len,
                                                                  const void* in, double* integ, void* out,
                                                                  double* action, int inplace) {
  const int64_t ep = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t n = b.n;
  if (ep >= n) return;
  const LeanDev I = lean_of(in, n), O = lean_of(out, n);
  // every load before the first data-dependent branch (the done test, the
  // controller's finiteness test)
  const bool done = FREEZE && I.b[QT_FB_DONE * n + ep];
  constexpr int NI = integ_rows<KC>();
  double x[12], in4[4] = {0.0, 0.0, 0.0, NAN}, u[4];
#pragma unroll
  for (int i = 0; i < 12; ++i) x[i] = I.f[(QT_LR_X + i) * n + ep];
  const Counts k = load_counts(I, n, ep);
#pragma unroll
  for (int i = 0; i < NI; ++i) in4[i] = integ[i * n + ep];
  const double hover = b.hover ? b.hover[ep] : c.hover_thrust;
  CtlGains<KC, KS> G;
  load_gains<KC, KC == 3 || KS>(b, ep, G);
  const FFLane fl = ff_of(b, c, ep);
  const EpisodeIn ei = episode_in(e, b, ep);
  const double t = time_at(ttab, len, k.step);
  const double t_next = time_at(ttab, len, k.step + 1);  // the table holds the same t + dt
  if (done) {
    if (!inplace) copy_column(I, O, n, ep);
    if (action) {
#pragma unroll
      for (int i = 0; i < 4; ++i) action[i * n + ep] = 0.0;
    }
    return;
  }
  // the observation's target, by the call the full frame stored it with
  // (env_step_into at this time, frame_reset_kernel at 0); the acceleration
  // is read only by feed-forward
  Target tg;
  target_state<true>(e, ei.motion, ei.pt, t, tg);
  if (!FF) tg.a[0] = tg.a[1] = tg.a[2] = 0.0;
  // the observation time is the env time (quadcopter_env.py:495)
  control<KC, FF, KS>(c, b, ep, G, hover, x, x + 3, tg, t, fl, in4, u);
#pragma unroll
  for (int i = 0; i < NI; ++i) integ[i * n + ep] = in4[i];
  if (action) {
#pragma unroll
    for (int i = 0; i < 4; ++i) action[i * n + ep] = u[i];
  }
  env_step_into(e, ei, n, ep, x, t_next, k, u, O);
}

// ------------------------------------------------------------------ expand

// One full-frame column per lane from a lean one (quadtrack.h qt_lean_expand).
__global__ __launch_bounds__(kBlock) void lean_expand_kernel(qt_env_params e, BatchDev b,
                                                             const double* __restrict__ ttab, int64_t len,
                                                             const void* lean, void* frame) {
  const int64_t ep = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t n = b.n;
  if (ep >= n) return;
  const LeanDev I = lean_of(lean, n);
  double* f = static_cast<double*>(frame);
  int64_t* fc = reinterpret_cast<int64_t*>(f + QT_FR_ROWS * n);
  int8_t* fb = reinterpret_cast<int8_t*>(f + (QT_FR_ROWS + QT_FC_ROWS) * n);
  const Counts k = load_counts(I, n, ep);
  const EpisodeIn ei = episode_in(e, b, ep);
  const double t = time_at(ttab, len, k.step);
#pragma unroll
  for (int i = 0; i < 12; ++i) f[(QT_FR_X + i) * n + ep] = I.f[(QT_LR_X + i) * n + ep];
  Target tg;
  target_state<true>(e, ei.motion, ei.pt, t, tg);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    f[(QT_FR_TARGET + i) * n + ep] = tg.p[i];
    f[(QT_FR_TARGET + 3 + i) * n + ep] = tg.v[i];
    f[(QT_FR_TARGET + 6 + i) * n + ep] = tg.a[i];
  }
  const double reward = I.f[QT_LR_REWARD * n + ep];
  f[QT_FR_TIME * n + ep] = t;
  f[QT_FR_ERR * n + ep] = -reward;  // exact; a NaN's sign flips back
  f[QT_FR_REWARD * n + ep] = reward;
  f[QT_FR_RATIO * n + ep] = k.step == 0 ? 0.0 : (double)k.on / (double)k.step;  // frame_reset_kernel's 0.0
  fc[QT_FC_STEP * n + ep] = k.step;
  fc[QT_FC_VIOLATIONS * n + ep] = k.viol;
  fc[QT_FC_ON_TARGET * n + ep] = k.on;
#pragma unroll
  for (int r = 0; r < QT_FB_ROWS; ++r) fb[r * n + ep] = I.b[r * n + ep];
}

// ------------------------------------------------------------- dispatch

struct LeanClosedLaunch {
  hipStream_t s;
  const qt_env_params& e;
  const qt_ctrl_params& c;
  const BatchDev& b;
  const double* ttab;
  int64_t len;
  const void* in;
  double* integ;
  void* out;
  double* action;
  bool freeze;
  template <int KC, bool FF, bool KS>
  int run() {
    const int inplace = in == out;
    if (freeze)
      lean_closed_step_kernel<KC, FF, KS, true>
          <<<grid_of(b.n), kBlock, 0, s>>>(e, c, b, ttab, len, in, integ, out, action, inplace);
    else
      lean_closed_step_kernel<KC, FF, KS, false>
          <<<grid_of(b.n), kBlock, 0, s>>>(e, c, b, ttab, len, in, integ, out, action, inplace);
    return check_launch();
  }
};

// the table covers ttab[max_step + 1] (quadtrack.h "Time table")
bool table_covers(const double* ttab, int64_t len, int64_t max_step) {
  return ttab && max_step >= 0 && max_step + 1 < len;
}

}  // namespace

extern "C" {

int qt_lean_reset(const qt_env_params* env, const qt_batch* batch, const double* offset, void* lean,
                  void* stream) {
  if (!env || !batch || batch->n < 0 || batch->order) return QT_EINVAL;
  if (batch->n == 0) return QT_OK;
  if (!offset || !lean) return QT_EINVAL;
  lean_reset_kernel<<<grid_of(batch->n), kBlock, 0, (hipStream_t)stream>>>(*env, to_dev(batch), offset, lean);
  return check_launch();
}

int qt_lean_step(const qt_env_params* env, const qt_batch* batch, const double* ttab, int64_t len,
                 int64_t max_step, const void* in, qt_view action, void* out, int32_t freeze_done,
                 void* stream) {
  if (!env || !batch || batch->n < 0 || batch->order) return QT_EINVAL;
  if (batch->n == 0) return QT_OK;
  if (!in || !out || !valid_view(action) || !table_covers(ttab, len, max_step)) return QT_EINVAL;
  const BatchDev b = to_dev(batch);
  hipStream_t s = (hipStream_t)stream;
  const int inplace = in == out;
  if (freeze_done)
    lean_step_kernel<true><<<grid_of(b.n), kBlock, 0, s>>>(*env, b, ttab, len, in, action, out, inplace);
  else
    lean_step_kernel<false><<<grid_of(b.n), kBlock, 0, s>>>(*env, b, ttab, len, in, action, out, inplace);
  return check_launch();
}

int qt_lean_closed_step(const qt_env_params* env, const qt_ctrl_params* ctrl, const qt_batch* batch,
                        const double* ttab, int64_t len, int64_t max_step, const void* in, double* integ,
                        void* out, double* action, int32_t freeze_done, void* stream) {
  if (!env || !ctrl || !batch || !batch->K || batch->n < 0 || batch->order) return QT_EINVAL;
  if (batch->k_cols != 3 && batch->k_cols != 6 && batch->k_cols != 9) return QT_EINVAL;
  if (batch->n == 0) return QT_OK;
  if (!in || !out || (batch->k_cols != 6 && !integ) || !table_covers(ttab, len, max_step)) return QT_EINVAL;
  const BatchDev b = to_dev(batch);
  const bool ff = ctrl->feedforward_enabled != 0 || batch->ff != nullptr;
  LeanClosedLaunch l{(hipStream_t)stream, *env, *ctrl, b, ttab, len, in, integ, out, action, freeze_done != 0};
  return dispatch_ctl(batch->k_cols, ff, batch->k_structured != 0, l);
}

int qt_lean_expand(const qt_env_params* env, const qt_batch* batch, const double* ttab, int64_t len,
                   const void* lean, void* frame, void* stream) {
  if (!env || !batch || batch->n < 0 || batch->order) return QT_EINVAL;
  if (batch->n == 0) return QT_OK;
  if (!lean || !frame || !ttab || len < 1) return QT_EINVAL;
  lean_expand_kernel<<<grid_of(batch->n), kBlock, 0, (hipStream_t)stream>>>(*env, to_dev(batch), ttab, len, lean,
                                                                           frame);
  return check_launch();
}

}  // extern "C"
