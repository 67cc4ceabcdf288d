// qt_policy_population.hip — the fused policy rollout for a population of
// networks of one shape (include/quadtrack.h, "policy populations"): every
// wave runs its own member's parameter block.  The episode body restates
// policy_rollout_kernel (qt_policy.hip) statement for statement on the same
// device functions (policy_features, policy_forward, the exact env step), so
// a member's episodes get the bits of a single-policy launch of that member;
// only the slot -> (member, episode) map and the weight base differ (the base
// is the member's block in global memory, or the wave's copy of it in LDS).
// qt_policy.hip and qt_policy.hpp are not touched by this unit.
// Built with the default flags (exact f32: no relaxed math), as qt_policy.hip.
#include <cstdlib>

#include "qt_policy.hpp"
#include "qt_step.hpp"

using namespace qtp;

namespace {

// Launch slots are padded per member to whole waves: EP = 64 wpm slots per
// member, wave w belongs to member w / wpm, a wave never holds two members.
// The member index is made wave-uniform (readfirstlane), so the weight base is
// a scalar: the output layer's weights stay scalar loads and an A operand's
// address stays base + lane.  A dead lane of a member's last wave reads its own
// member's last episode (every lane reaches the MFMAs), takes no env step and
// stores nothing.
//
// STAGE: the wave first copies its member's block into its own quarter of the
// block's LDS (stage floats per wave) and runs the network from there.  The
// four waves of a block hold up to four members, whose blocks together exceed
// the CU's first-level caches; the values and their order of use are the same,
// so the results are the bits of the unstaged kernel.  A wave reads only what
// it wrote itself (LDS operations of one wave execute in order): no block
// barrier, so a wave past the population may return before it.
template <int NT, bool STAGE>
__global__ __launch_bounds__(kBlock) void policy_population_kernel(qt_env_params e, qt_criteria cr, BatchDev b,
                                                                   PolicyDev P0, int members, int64_t stride,
                                                                   int64_t E, int64_t wpm, int stage, qt_state st,
                                                                   int nsteps, double* __restrict__ rec) {
  extern __shared__ __attribute__((aligned(16))) float staged[];
  const int wave_in_block = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t wave = (int64_t)blockIdx.x * (kBlock / 64) + wave_in_block;
  if (wave / wpm >= members) return;  // a whole wave past the population
  const int m = __builtin_amdgcn_readfirstlane((int)(wave / wpm));
  const int64_t local = (wave - (int64_t)m * wpm) * 64 + (threadIdx.x & 63);
  const int64_t n = b.n;
  const bool live = local < E;
  const int64_t ep = (int64_t)m * E + (live ? local : E - 1);
  PolicyDev P = P0;
  P.w = P0.w + (int64_t)m * stride;
  if (STAGE) {
    float* mine = staged + wave_in_block * stage;
    const int nb = (int)policy_block_floats(P0.nh, NT);  // <= stage (host)
    for (int i = threadIdx.x & 63; i < nb; i += 64) mine[i] = P.w[i];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    P.w = mine;
  }
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
  }
}

constexpr int64_t kLdsBytes = 160 * 1024;  // LDS of a gfx950 CU, all of which one workgroup may take

// QT_POPULATION_STAGE=0 runs every shape unstaged (timing comparisons, and the tests of that path)
bool stage_off() {
  const char* v = getenv("QT_POPULATION_STAGE");
  return v && v[0] == '0';
}

// qt_policy.hip's rules: tiles of 32 of the widest hidden layer, rounded up to 1, 2 or 4 (0: invalid)
int shape_tiles(const qt_policy* p) {
  if (!p->params || p->n_hidden < 1 || p->n_hidden > QT_POLICY_MAX_HIDDEN) return 0;
  if (p->activation < QT_ACT_RELU || p->activation > QT_ACT_LEAKY_RELU) return 0;
  int wmax = 0;
  for (int i = 0; i < p->n_hidden; ++i) {
    if (p->width[i] < 1 || p->width[i] > QT_POLICY_MAX_WIDTH) return 0;
    wmax = p->width[i] > wmax ? p->width[i] : wmax;
  }
  const int t = (wmax + 31) / 32;
  return t == 3 ? 4 : t;
}

}  // namespace

extern "C" {

int qt_policy_population_version(void) { return 1; }

int qt_policy_population_rollout(const qt_env_params* env, const qt_policy_population* pop, const qt_criteria* crit,
                                 const qt_batch* batch, qt_state st, int32_t nsteps, double* rec, void* stream) {
  if (!pop || !env || !crit || !batch || nsteps < 0 || batch->order) return QT_EINVAL;
  const int nt = shape_tiles(&pop->shape);
  if (nt == 0 || pop->members < 1 || pop->episodes_per_member < 1) return QT_EINVAL;
  if (pop->stride < policy_block_floats(pop->shape.n_hidden, nt)) return QT_EINVAL;
  const int64_t M = pop->members, E = pop->episodes_per_member;
  int64_t n, slots;
  if (__builtin_mul_overflow(M, E, &n) || n != batch->n) return QT_EINVAL;
  const int64_t wpm = (E + 63) / 64;  // n fits, so wpm and 64 wpm do
  if (__builtin_mul_overflow(M, wpm * 64, &slots) || (slots + kBlock - 1) / kBlock > INT32_MAX) return QT_EINVAL;
  if (nsteps == 0) return QT_OK;
  if (!valid_state(st, false)) return QT_EINVAL;
  PolicyDev P{};
  P.w = pop->shape.params, P.nh = pop->shape.n_hidden, P.act = pop->shape.activation;
  for (int i = 0; i < 4; ++i) {
    P.scale[i] = (float)(pop->shape.hi[i] - pop->shape.lo[i]);
    P.lo[i] = (float)pop->shape.lo[i];
  }
  const BatchDev b = to_dev(batch);
  hipStream_t s = (hipStream_t)stream;
  const int grid = grid_of(slots);
  const int mem = pop->members;
  // staged when the four waves' blocks fit the CU's LDS ([64, 64]: 4 x 22.8 KB; never [128, 128])
  const int64_t stage = (policy_block_floats(pop->shape.n_hidden, nt) + 63) / 64 * 64;
  const int64_t lds = (kBlock / 64) * stage * (int64_t)sizeof(float);
  const bool staged = lds <= kLdsBytes && !stage_off();
#define QT_POP_LAUNCH(NT)                                                                                         \
  do {                                                                                                            \
    if (staged) {                                                                                                 \
      if (hipFuncSetAttribute((const void*)policy_population_kernel<NT, true>,                                    \
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)                \
        return QT_ELAUNCH;                                                                                        \
      policy_population_kernel<NT, true><<<grid, kBlock, (size_t)lds, s>>>(*env, *crit, b, P, mem, pop->stride, E, \
                                                                           wpm, (int)stage, st, nsteps, rec);     \
    } else {                                                                                                      \
      policy_population_kernel<NT, false><<<grid, kBlock, 0, s>>>(*env, *crit, b, P, mem, pop->stride, E, wpm, 0, \
                                                                  st, nsteps, rec);                               \
    }                                                                                                             \
  } while (0)
  if (nt == 1)
    QT_POP_LAUNCH(1);
  else if (nt == 2)
    QT_POP_LAUNCH(2);
  else
    QT_POP_LAUNCH(4);
#undef QT_POP_LAUNCH
  return check_launch();
}

}  // extern "C"
