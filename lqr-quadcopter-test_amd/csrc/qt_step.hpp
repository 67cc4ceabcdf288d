// qt_step.hpp — what the per-step kernels of both frame layouts share
// (qt_step.hip: the full frame, quadtrack.h qt_frame_row; qt_step_lean.hip:
// the lean frame, qt_lean_row): the episode's per-launch inputs, the
// controller dispatch and ONE env.step body.  The step body is written once
// and stores through the layout's store_early / store_late overloads, so that
// both layouts run the same source expressions (-ffp-contract=on contracts
// per expression: the lean path's results equal the full frame's bit for bit
// because the text is the same).  The device functions here are `static`:
// with internal linkage the optimizer sees every caller and carries the
// kernels' index ranges (0 <= ep < n) into the row addressing, as it does for
// a function of the including file.
#pragma once
#include "qt_kernels.hpp"

namespace qts {

using namespace qtk;

static __device__ __forceinline__ double view_at(const qt_view& v, int r, int64_t e) {
  return v.p[r * v.rs + e * v.es];
}

// Counters carried from frame to frame (info["step"], info["action_violations"],
// the env's on-target count).
struct Counts {
  int64_t step, viol, on;
};

// An episode's per-launch inputs outside the frame: motion type, target
// pattern, plant.  Loaded with everything else before any data-dependent
// branch, so that a step waits for memory once (DESIGN §3 "Per-step API").
struct EpisodeIn {
  int motion;
  Pattern pt;
  Plant pl;
};

static __device__ __forceinline__ EpisodeIn episode_in(const qt_env_params& e, const BatchDev& b, int64_t ep) {
  const int motion = motion_of(b, e, ep);
  return EpisodeIn{motion, pattern_of(b, e, motion, ep), make_plant(e, b.plant_mass ? b.plant_mass[ep] : e.mass)};
}

// QuadcopterEnv.step (quadcopter_env.py:152-232) of episode ep from state x
// with the raw action u, to the post-step time t (the caller's t + dt), into
// the frame O of either layout:
// _parse_and_validate_action (234-293), _integrate (295-327),
// _apply_state_constraints (428-465), observation (472-496), reward
// (504-511), termination (513-535), on-target count (204-207), info
// (209-226), success (537-553).  The results leave through two functions the
// layout (the type of O) provides, found at instantiation:
//   store_early(O, n, ep, tg, t, step)  what depends on time only (the target
//                         at t, t, the new step count), before the arithmetic
//   store_late(O, n, ep, x, err, ratio, k, term, on, viol, success)  the rest
// A layout stores what it keeps and drops the rest.
template <class Out>
static __device__ __forceinline__ void env_step_into(const qt_env_params& e, const EpisodeIn& in, int64_t n,
                                                     int64_t ep, double* x, double t, Counts k, const double* u,
                                                     const Out& O) {
  const int motion = in.motion;
  const Pattern& pt = in.pt;
  const Plant& pl = in.pl;
  double ua[4];
  // The rows that depend on time only (the target observation, time, step
  // count) first: their stores drain while the step computes, which shortens
  // a small batch's launch (one wave per SIMD: load, compute, store in
  // series; 65,536 episodes 9.0 -> 8.0-8.7 us, profiles/r06/step_kernel_ab_r06_early.jsonl).
  // Every load of the step precedes this (in == out steps in place).
  Target tg;
  target_state<true>(e, motion, pt, t, tg);
  store_early(O, n, ep, tg, t, k.step + 1);
  const bool viol = parse_action(e, u, ua);
  integrate(e, pl, x, ua);
  // np.clip's NaN propagation kept: a caller's action may drive the state anywhere
  const int term = constrain_terminate<true>(e, x, t);
  const double q0 = x[0] - tg.p[0], q1 = x[1] - tg.p[1], q2 = x[2] - tg.p[2];
  const double err = sqrt(dot3_blas(q0, q1, q2));  // float(np.linalg.norm(quad_pos - target_pos))
  const bool on = err <= e.target_radius;
  k.step += 1;
  k.viol += viol;
  k.on += on;
  const double ratio = (double)k.on / (double)k.step;
  const bool success = !(t < e.min_episode_duration) && ratio >= e.min_on_target_ratio;
  store_late(O, n, ep, x, err, ratio, k, term, on, viol, success);
}

// The controller of one episode: RiccatiLQRController / LQRController
// (compute_action) or PIDController (compute_action_pid, observation time
// `now`).  KS (the caller asserts the structured gain pattern): the six
// (nine) per-axis gains are read, which equals K s exactly for a finite s;
// a non-finite observation or integral takes the dense product, whose
// 0 * NaN terms the reference's K @ s has (riccati_lqr.py:864-900).
template <int KC, bool KS>
using CtlGains = Gains<KC, KC == 3 || KS>;

template <int KC, bool FF, bool KS>
static __device__ __forceinline__ bool control(const qt_ctrl_params& c, const BatchDev& b, int64_t ep,
                                               const CtlGains<KC, KS>& G, double hover, const double* qp,
                                               const double* qv, const Target& tg, double now, const FFLane& fl,
                                               double* in, double* u) {
  if constexpr (KC == 3) {
    compute_action_pid<FF>(c, G.k, hover, qp, qv, tg, now, fl, in, u);
    return false;
  } else if constexpr (KS) {
    double s = ((qp[0] + qp[1]) + (qp[2] + qv[0])) + ((qv[1] + qv[2]) + (tg.p[0] + tg.p[1])) +
               ((tg.p[2] + tg.v[0]) + (tg.v[1] + tg.v[2]));
    if (KC == 9) s += (in[0] + in[1]) + in[2];
    if (__builtin_expect(isfinite(s), 1)) return compute_action<KC, FF, true>(c, G, hover, qp, qv, tg, fl, in, u);
    Gains<KC, false> D;
    load_gains<KC, false>(b, ep, D);
    return compute_action<KC, FF, false>(c, D, hover, qp, qv, tg, fl, in, u);
  } else {
    return compute_action<KC, FF, false>(c, G, hover, qp, qv, tg, fl, in, u);
  }
}

// integral / controller-state rows: LQI 3, PID 4 (integral error + last time)
template <int KC>
constexpr int integ_rows() {
  return KC == 9 ? 3 : (KC == 3 ? 4 : 0);
}

// Calls L::template run<KC, FF, KS>() for a runtime (kc, ff, ks); PID (kc 3)
// is per-axis by construction.
template <class L>
int dispatch_ctl(int kc, bool ff, bool ks, L& l) {
  if (kc == 3) return ff ? l.template run<3, true, true>() : l.template run<3, false, true>();
  if (kc == 9) {
    if (ff) return ks ? l.template run<9, true, true>() : l.template run<9, true, false>();
    return ks ? l.template run<9, false, true>() : l.template run<9, false, false>();
  }
  if (ff) return ks ? l.template run<6, true, true>() : l.template run<6, true, false>();
  return ks ? l.template run<6, false, true>() : l.template run<6, false, false>();
}

inline bool valid_view(const qt_view& v) { return v.p != nullptr; }

}  // namespace qts
