// qt_policy.hip — the deep tracking policy's kernels and their C ABI
// (include/quadtrack.h, "the deep tracking policy"): compute_action for a
// batch of observations, and the fused closed loop with the policy as the
// controller.  The forward pass is qt_policy.hpp's policy_forward; the env
// step restates the call sequence of the exact flavour of run_steps
// (qt_kernels.hpp) on the same device functions, so a step from the same
// state and command gives the same numbers as qt_rollout's exact step.
// This unit is built with the default flags (exact f32: no relaxed math).
#include "qt_policy.hpp"
#include "qt_step.hpp"

using namespace qtp;

namespace {

// One wave = 64 consecutive episodes; a lane past the batch reads the last
// episode's inputs (so that every lane reaches the MFMAs) and stores nothing.

template <int NT>
__global__ __launch_bounds__(kBlock) void policy_action_kernel(PolicyDev P, int64_t n, qt_policy_obs o,
                                                               const int8_t* __restrict__ frozen,
                                                               double* __restrict__ action) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if ((p & ~(int64_t)63) >= n) return;  // a whole wave past the batch
  const bool live = p < n;
  const int64_t ep = live ? p : n - 1;
  double qp[3], qv[3], att[3], rate[3], tp[3], tv[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    qp[i] = qts::view_at(o.pos, i, ep), qv[i] = qts::view_at(o.vel, i, ep);
    att[i] = qts::view_at(o.att, i, ep), rate[i] = qts::view_at(o.rate, i, ep);
    tp[i] = qts::view_at(o.tpos, i, ep), tv[i] = qts::view_at(o.tvel, i, ep);
  }
  const bool zero = frozen && frozen[ep] != 0;
  float f[kPolicyIn];
  policy_features(qp, qv, att, rate, tp, tv, f);
  double u[4];
  policy_forward<NT>(P, f, u);
  if (live) {
#pragma unroll
    for (int i = 0; i < 4; ++i) action[i * n + ep] = zero ? 0.0 : u[i];
  }
}

// The closed loop of one lane's episode.  Per step: the policy's command on
// the current observation (every lane of the wave, MFMA), then, for the lanes
// still running, the Evaluator's pre-step record and env.step exactly as the
// exact flavour of run_steps does them: parse_action, integrate_closed,
// constrain_terminate, target_state, post-step error.
template <int NT>
__global__ __launch_bounds__(kBlock) void policy_rollout_kernel(qt_env_params e, qt_criteria cr, BatchDev b, PolicyDev P,
                                                                qt_state st, int nsteps, double* __restrict__ rec) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t n = b.n;
  if ((p & ~(int64_t)63) >= n) return;  // a whole wave past the batch
  const bool live = p < n;
  const int64_t ep = live ? p : n - 1;
  const int motion = motion_of(b, e, ep);
  const Pattern pt = pattern_of(b, e, motion, ep);
  const Plant pl = make_plant(e, b.plant_mass ? b.plant_mass[ep] : e.mass);
  double x[12], t;
  Target tg;
#pragma unroll
  for (int i = 0; i < 12; ++i) x[i] = st.x[i * n + ep];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    tg.p[i] = st.target[i * n + ep];
    tg.v[i] = st.target[(3 + i) * n + ep];
    tg.a[i] = st.target[(6 + i) * n + ep];
  }
  t = st.t[ep];
  Acc a = load_acc(st.acc, n, ep);
  const int term0 = a.term;
  if (!live) a.term = QT_TERM_TIME_LIMIT;  // takes no step, stores nothing
  // the pre-step tracking error, carried from the previous step's post-step
  // error (run_steps: positions are not constrained, so they are the same number)
  double err_pre = sqrt(sq3_ref(tg.p[0] - x[0], tg.p[1] - x[1], tg.p[2] - x[2]));
  const RateLin rl = make_rate_lin(e);
  const VelLin vl = make_vel_lin(e, pl);
  const SmallCoef sk;
  const double R = cr.target_radius;
  for (int s = 0; s < nsteps; ++s) {
    const bool running = a.term == QT_TERM_RUNNING;
    if (__builtin_amdgcn_ballot_w64(running) == 0) break;  // uniform: every episode of the wave is done
    float f[kPolicyIn];
    policy_features(x, x + 3, x + 6, x + 9, tg.p, tg.v, f);
    double u[4];
    policy_forward<NT>(P, f, u);
    if (running) {
      // ---- the Evaluator's pre-step record (eval.py:142-159) -> metrics accumulators
      const double err = err_pre;
      const double un = sqrt_noscale(u[0] * u[0] + u[1] * u[1] + u[2] * u[2] + u[3] * u[3]);
      a.sum_e += err;
      a.sum_e2 += err * err;
      a.max_e = (!(err <= a.max_e) && !(a.max_e != a.max_e)) ? err : a.max_e;  // np.max, NaN-propagating
      const bool on = err <= R;
      a.on_pre += on;
      a.sum_u += un;
      overshoot_step(a, on, err - R, cr.overshoot_window);  // no-op on the first step (prev_on < 0)
      a.prev_on = on;
      // ---- env.step (quadcopter_env.py:152-232)
      // The attitude's sin / cos are evaluated at every step (run_steps carries
      // them from step to step and evaluates them at a launch's start): a step
      // is then a function of the stored state alone, so a run in chunks gives
      // the bits of a run in one launch.
      double ua[4], d4[3];
      a.viol += parse_action(e, u, ua);
      Trig ta, t4;
      trig_of(x + 6, ta);
      integrate_closed<-1>(e, rl, vl, pl, ta, x, ua, d4, t4, sk);
      t += e.dt;
      const int term = constrain_terminate<false>(e, x, t);
      target_state<true>(e, motion, pt, t, tg);
      const double q0 = x[0] - tg.p[0], q1 = x[1] - tg.p[1], q2 = x[2] - tg.p[2];
      err_pre = sqrt_noscale(sq3_ref(q0, q1, q2));  // this step's post-step error, the next one's pre-step
      a.on_post += err_pre <= e.target_radius;
      a.term = term;
      a.steps += 1;
      if (rec) {
        double* r = rec + (int64_t)s * 16 * n + ep;
#pragma unroll
        for (int i = 0; i < 12; ++i) r[i * n] = x[i];
#pragma unroll
        for (int i = 0; i < 4; ++i) r[(12 + i) * n] = u[i];
      }
    }
  }
  if (live && term0 == QT_TERM_RUNNING) {  // an episode done before the launch keeps its stored state
#pragma unroll
    for (int i = 0; i < 12; ++i) st.x[i * n + ep] = x[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      st.target[i * n + ep] = tg.p[i];
      st.target[(3 + i) * n + ep] = tg.v[i];
      st.target[(6 + i) * n + ep] = tg.a[i];
    }
    st.t[ep] = t;
    store_acc(st.acc, n, ep, a);
  }
}

// tiles of 32 of the widest hidden layer, rounded up to 1, 2 or 4 (0: invalid policy)
int policy_tiles(const qt_policy* p) {
  if (!p || !p->params || p->n_hidden < 1 || p->n_hidden > QT_POLICY_MAX_HIDDEN) return 0;
  if (p->activation < QT_ACT_RELU || p->activation > QT_ACT_LEAKY_RELU) return 0;
  int wmax = 0;
  for (int i = 0; i < p->n_hidden; ++i) {
    if (p->width[i] < 1 || p->width[i] > QT_POLICY_MAX_WIDTH) return 0;
    wmax = p->width[i] > wmax ? p->width[i] : wmax;
  }
  const int t = (wmax + 31) / 32;
  return t == 3 ? 4 : t;
}

PolicyDev policy_dev(const qt_policy* p) {
  PolicyDev d{};
  d.w = p->params, d.nh = p->n_hidden, d.act = p->activation;
  for (int i = 0; i < 4; ++i) {
    d.scale[i] = (float)(p->hi[i] - p->lo[i]);
    d.lo[i] = (float)p->lo[i];
  }
  return d;
}

}  // namespace

extern "C" {

int qt_policy_version(void) { return 1; }

int qt_policy_action(const qt_policy* policy, int64_t n, const qt_policy_obs* obs, const int8_t* frozen,
                     double* action, void* stream) {
  const int nt = policy_tiles(policy);
  if (nt == 0 || n < 0) return QT_EINVAL;
  if (n == 0) return QT_OK;
  if (!obs || !action || !obs->pos.p || !obs->vel.p || !obs->att.p || !obs->rate.p || !obs->tpos.p || !obs->tvel.p)
    return QT_EINVAL;
  const PolicyDev P = policy_dev(policy);
  hipStream_t s = (hipStream_t)stream;
  if (nt == 1)
    policy_action_kernel<1><<<grid_of(n), kBlock, 0, s>>>(P, n, *obs, frozen, action);
  else if (nt == 2)
    policy_action_kernel<2><<<grid_of(n), kBlock, 0, s>>>(P, n, *obs, frozen, action);
  else
    policy_action_kernel<4><<<grid_of(n), kBlock, 0, s>>>(P, n, *obs, frozen, action);
  return check_launch();
}

int qt_policy_rollout(const qt_env_params* env, const qt_policy* policy, const qt_criteria* crit,
                      const qt_batch* batch, qt_state st, int32_t nsteps, double* rec, void* stream) {
  const int nt = policy_tiles(policy);
  if (nt == 0 || !env || !crit || !batch || batch->n < 0 || nsteps < 0 || batch->order) return QT_EINVAL;
  if (batch->n == 0 || nsteps == 0) return QT_OK;
  if (!valid_state(st, false)) return QT_EINVAL;
  const PolicyDev P = policy_dev(policy);
  const BatchDev b = to_dev(batch);
  hipStream_t s = (hipStream_t)stream;
  const int grid = grid_of(batch->n);
  if (nt == 1)
    policy_rollout_kernel<1><<<grid, kBlock, 0, s>>>(*env, *crit, b, P, st, nsteps, rec);
  else if (nt == 2)
    policy_rollout_kernel<2><<<grid, kBlock, 0, s>>>(*env, *crit, b, P, st, nsteps, rec);
  else
    policy_rollout_kernel<4><<<grid, kBlock, 0, s>>>(*env, *crit, b, P, st, nsteps, rec);
  return check_launch();
}

}  // extern "C"
