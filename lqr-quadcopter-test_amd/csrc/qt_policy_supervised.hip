// qt_policy_supervised.hip — the fused policy rollout with a classical teacher
// (include/quadtrack.h, "supervised policy rollout"; reference: the imitation
// mode of the trainer, train.py:654-862): the policy flies the episode and, at
// every step, a supervisor (Riccati-LQR / heuristic LQR, LQI or PID) is asked
// what it would have commanded on the same observation.  The launch keeps the
// per-episode sum of squared differences, a sampled (features, teacher
// command, policy command) data set and, on request, every teacher command.
//
// The episode body restates policy_rollout_kernel (qt_policy.hip) statement
// for statement on the same device functions, so the flight has the bits of
// qt_policy_rollout: the teacher never influences it.  The teacher is
// qts::control<KC, false, KS> (qt_step.hpp), the function of the per-step
// API's action_obs_kernel, so its commands and its integral state have the
// bits of qt_compute_action_obs on the same observations.
//
// One kernel per (NT, KC, KS): the teacher's variant is a template argument,
// not a switch inside the step (DESIGN §3 "Supervised rollout" has the
// register report of every variant beside its policy_rollout_kernel<NT>).  The
// teacher runs inside the step BEFORE the forward pass, with the gains loaded
// there: no gain register, teacher temporary or sample row is live across the
// MFMA section; the integral rows, the loss and four f32 labels are carried.
// qt_policy.hip, qt_policy.hpp and qt_policy_population.hip are not touched.
// Built with the default flags (exact f32: no relaxed math), as qt_policy.hip.
#include "qt_policy.hpp"
#include "qt_step.hpp"

using namespace qtp;

namespace {

// sum_i (u_i - fl32(s_i))^2 added to `loss` in index order, every product and
// every add rounded on its own (s: the teacher's commands already rounded to f32)
__device__ __forceinline__ double loss_step(double loss, const double* u, const float* s) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const double d = u[i] - (double)s[i];
    const double d2 = d * d;
    loss = loss + d2;
  }
  return loss;
}

template <int NT, int KC, bool KS>
__global__ __launch_bounds__(kBlock) void policy_supervised_kernel(qt_env_params e, qt_ctrl_params c, qt_criteria cr,
                                                                   BatchDev b, PolicyDev P, qt_state st, int nsteps,
                                                                   qt_policy_supervision sup,
                                                                   double* __restrict__ rec) {
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
  // the teacher's carried state: LQI integral | PID integral error + last observation time
  constexpr int NI = qts::integ_rows<KC>();
  double in[4] = {0.0, 0.0, 0.0, NAN};
#pragma unroll
  for (int i = 0; i < NI; ++i) in[i] = st.integ[i * n + ep];
  double loss = sup.loss[ep];
  // the lane's sample cursor: the first slot whose step is not behind the episode
  const int S = sup.samples;
  int slot = 0, next = -1;
  for (; slot < S; ++slot) {
    next = sup.sample_steps[(int64_t)slot * n + ep];
    if (next >= a.steps) break;
  }
  if (slot >= S) next = -1;
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
    // ---- the supervisor on the same observation (train.py:673-696), BEFORE the forward pass: its
    // temporaries, the gains and the slot's 22 feature and label rows are dead when the MFMA section
    // starts; only the four f32 labels cross it, for the loss.  The teacher reads the observation
    // alone, so its place in the step changes no result.  The observation time is the env time.
    const bool sampled = running && a.steps == next;  // next >= 0 only while slot < S
    float label[4] = {};
    if (running) {
      double su[4];
      const double hover = b.hover ? b.hover[ep] : c.hover_thrust;
      qts::CtlGains<KC, KS> G;
      load_gains<KC, KC == 3 || KS>(b, ep, G);
      qts::control<KC, false, KS>(c, b, ep, G, hover, x, x + 3, tg, t, FFLane{}, in, su);
#pragma unroll
      for (int i = 0; i < 4; ++i) label[i] = (float)su[i];  // torch.tensor(..., dtype=torch.float32)
      if (sampled) {
        float* q = sup.sample + (int64_t)slot * QT_SUP_ROWS * n + ep;
#pragma unroll
        for (int i = 0; i < kPolicyIn; ++i) q[i * n] = f[i];
#pragma unroll
        for (int i = 0; i < 4; ++i) q[(kPolicyIn + i) * n] = label[i];
      }
      if (sup.teacher_rec) {
        double* r = sup.teacher_rec + (int64_t)s * 4 * n + ep;
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i * n] = su[i];
      }
    }
    double u[4];
    policy_forward<NT>(P, f, u);
    if (running) {
      loss = loss_step(loss, u, label);
      if (sampled) {
        float* q = sup.sample + ((int64_t)slot * QT_SUP_ROWS + kPolicyIn + 4) * n + ep;
#pragma unroll
        for (int i = 0; i < 4; ++i) q[i * n] = (float)u[i];
        ++slot;
        next = slot < S ? sup.sample_steps[(int64_t)slot * n + ep] : -1;
      }
      // ---- the Evaluator's pre-step record -> metrics accumulators
      const double err = err_pre;
      const double un = sqrt_noscale(u[0] * u[0] + u[1] * u[1] + u[2] * u[2] + u[3] * u[3]);
      a.sum_e += err;
      a.sum_e2 += err * err;
      a.max_e = (!(err <= a.max_e) && !(a.max_e != a.max_e)) ? err : a.max_e;  // np.max, NaN-propagating
      const bool on = err <= R;
      a.on_pre += on;
      a.sum_u += un;
      overshoot_step(a, on, err - R, cr.overshoot_window);
      a.prev_on = on;
      // ---- env.step, a function of the stored state alone (chunks give the bits of one launch)
      double ua[4], d4[3];
      a.viol += parse_action(e, u, ua);
      Trig ta, t4;
      trig_of(x + 6, ta);
      integrate_closed<-1>(e, rl, vl, pl, ta, x, ua, d4, t4, sk);
      t += e.dt;
      const int term = constrain_terminate<false>(e, x, t);
      target_state<true>(e, motion, pt, t, tg);
      const double q0 = x[0] - tg.p[0], q1 = x[1] - tg.p[1], q2 = x[2] - tg.p[2];
      err_pre = sqrt_noscale(sq3_ref(q0, q1, q2));
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
#pragma unroll
    for (int i = 0; i < NI; ++i) st.integ[i * n + ep] = in[i];
    sup.loss[ep] = loss;
  }
}

// qt_policy.hip's rules: tiles of 32 of the widest hidden layer, rounded up to 1, 2 or 4 (0: invalid)
int shape_tiles(const qt_policy* p) {
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

struct SupLaunch {
  hipStream_t s;
  int grid;
  const qt_env_params& e;
  const qt_ctrl_params& c;
  const qt_criteria& cr;
  const BatchDev& b;
  const PolicyDev& P;
  const qt_state& st;
  int nsteps;
  const qt_policy_supervision& sup;
  double* rec;
  template <int NT, int KC, bool KS>
  void run() const {
    policy_supervised_kernel<NT, KC, KS><<<grid, kBlock, 0, s>>>(e, c, cr, b, P, st, nsteps, sup, rec);
  }
  // PID (kc 3) is per-axis by construction
  template <int NT>
  void teacher(int kc, bool ks) const {
    if (kc == 3)
      run<NT, 3, true>();
    else if (kc == 9)
      ks ? run<NT, 9, true>() : run<NT, 9, false>();
    else
      ks ? run<NT, 6, true>() : run<NT, 6, false>();
  }
};

}  // namespace

extern "C" {

int qt_policy_supervised_version(void) { return 1; }

int qt_policy_supervised_rollout(const qt_env_params* env, const qt_ctrl_params* ctrl, const qt_policy* policy,
                                 const qt_criteria* crit, const qt_batch* batch, qt_state st, int32_t nsteps,
                                 const qt_policy_supervision* sup, double* rec, void* stream) {
  const int nt = shape_tiles(policy);
  if (nt == 0 || !env || !crit || !batch || batch->n < 0 || nsteps < 0 || batch->order) return QT_EINVAL;
  if (!ctrl || !sup || !sup->loss || !batch->K) return QT_EINVAL;
  const int kc = batch->k_cols;
  if (kc != 3 && kc != 6 && kc != 9) return QT_EINVAL;
  if ((ctrl->use_lqi != 0) != (kc == 9)) return QT_EINVAL;
  if (ctrl->feedforward_enabled != 0 || batch->ff) return QT_EINVAL;  // feed-forward teachers: out of scope
  if (kc != 6 && !st.integ) return QT_EINVAL;
  if (sup->samples < 0 || (sup->samples > 0 && (!sup->sample_steps || !sup->sample))) return QT_EINVAL;
  if (batch->n == 0 || nsteps == 0) return QT_OK;
  if (!valid_state(st, kc != 6)) return QT_EINVAL;
  PolicyDev P{};
  P.w = policy->params, P.nh = policy->n_hidden, P.act = policy->activation;
  for (int i = 0; i < 4; ++i) {
    P.scale[i] = (float)(policy->hi[i] - policy->lo[i]);
    P.lo[i] = (float)policy->lo[i];
  }
  const BatchDev b = to_dev(batch);
  const SupLaunch l{(hipStream_t)stream, grid_of(batch->n), *env, *ctrl, *crit, b, P, st, nsteps, *sup, rec};
  const bool ks = batch->k_structured != 0;
  if (nt == 1)
    l.teacher<1>(kc, ks);
  else if (nt == 2)
    l.teacher<2>(kc, ks);
  else
    l.teacher<4>(kc, ks);
  return check_launch();
}

}  // extern "C"
