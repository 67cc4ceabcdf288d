// qt_policy_optim.hip — gradient clipping, the optimiser step and the packed
// block in one launch, and the host loop that enqueues one pass of minibatch
// steps (include/quadtrack.h, "clip + optimiser step and the fused imitation
// fit").  Phases, arithmetic and summation order: qt_policy_optim.hpp.  Built
// with the default flags (exact f32: correctly rounded division and square
// root, no relaxed math).
#include <cmath>

#include "qt_policy_optim.hpp"

using namespace qto;

namespace {

struct OptArgs {
  int kind, skip, clip, lerp_low, sgd_plain;
  int flat, block_floats;
  double beta1, beta2, lr;
  float max_norm, wd, shrink, w1, b1, b2, w2, eps, momentum, neg_lr;
  const float* grad;
  float* theta;
  float* m;
  float* v;
  int64_t* step;
  int64_t* skipped;
  float* block;
  float* grad_norm;
  GradLayout lay;
};

constexpr int kOptBatch = 8;  // elements a thread loads before it computes (phase 2)

// phase 2 for one optimiser.  A thread's elements t, t + 1024, ... go in batches of kOptBatch: all loads of a
// batch first (an element past the end reads element 0 and is not stored), then the arithmetic, then the
// stores, so that a batch costs one trip to memory.  The body is branch-free: where torch chooses between
// two forms of a formula, both are formed and one is selected.
template <int KIND>
__device__ __forceinline__ void update(const OptArgs& a, int tid, bool first, float coef, float neg_step,
                                       float bc2_sqrt) {
  // the arrays do not overlap (quadtrack.h)
  const float* __restrict__ grad = a.grad;
  float* __restrict__ theta = a.theta;
  float* __restrict__ mom = a.m;
  float* __restrict__ var = a.v;
  const bool decay = a.wd != 0.0f, lerp_low = a.lerp_low != 0;
  for (int base = tid; base < a.flat; base += kOptBatch * kOptThreads) {
    float g[kOptBatch], th[kOptBatch], m[kOptBatch], v[kOptBatch];
#pragma unroll
    for (int u = 0; u < kOptBatch; ++u) {
      const int i = base + u * kOptThreads, j = i < a.flat ? i : 0;
      g[u] = grad[j], th[u] = theta[j], m[u] = mom[j];
      v[u] = KIND == QT_OPT_SGD ? 0.0f : var[j];
    }
#pragma unroll
    for (int u = 0; u < kOptBatch; ++u) {
#pragma clang fp contract(off)
      g[u] = g[u] * coef;  // coef = 1 without clipping: exact
      if (KIND == QT_OPT_ADAMW) {
        th[u] = th[u] * a.shrink;
      } else {
        const float d = a.wd * th[u];
        const float gd = g[u] + d;
        g[u] = decay ? gd : g[u];
      }
      if (KIND == QT_OPT_SGD) {
        float buf = m[u] * a.momentum;
        buf = buf + g[u];
        m[u] = first ? g[u] : buf;
        const float d = a.neg_lr * m[u];
        th[u] = th[u] + d;
      } else {
        const float diff = g[u] - m[u];
        const float lo = a.w1 * diff, hi = diff * a.b1;
        const float mlo = m[u] + lo, mhi = g[u] - hi;
        m[u] = lerp_low ? mlo : mhi;
        v[u] = v[u] * a.b2;
        float gg = a.w2 * g[u];
        gg = gg * g[u];
        v[u] = v[u] + gg;
        float den = sqrtf(v[u]);
        den = den / bc2_sqrt;
        den = den + a.eps;
        float num = neg_step * m[u];
        num = num / den;
        th[u] = th[u] + num;
      }
    }
#pragma unroll
    for (int u = 0; u < kOptBatch; ++u) {
      const int i = base + u * kOptThreads;
      if (i < a.flat) {
        theta[i] = th[u], mom[i] = m[u];
        if (KIND != QT_OPT_SGD) var[i] = v[u];
      }
    }
  }
}

// phase 3 for one layer's part of the block
template <typename F>
__device__ __forceinline__ void pack_part(const float* __restrict__ theta, float* __restrict__ part, int count,
                                          int tid, F source) {
#pragma unroll 4
  for (int rem = tid; rem < count; rem += kOptThreads) {
    const int src = source(rem);
    const float x = theta[src < 0 ? 0 : src];
    part[rem] = src < 0 ? 0.0f : x;
  }
}

__global__ __launch_bounds__(kOptThreads) void optim_kernel(OptArgs a) {
  __shared__ double red[kOptThreads / 64];
  const int tid = threadIdx.x;
  const int64_t step = *a.step;

  // ---------------------------------------------------------------- phase 1: the norm
  double s = 0.0;
#pragma unroll 8
  for (int i = tid; i < a.flat; i += kOptThreads) {
    const double g = (double)a.grad[i];
    s = s + g * g;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s = s + __shfl_xor(s, o, 64);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  double total = red[0];
#pragma unroll
  for (int w = 1; w < kOptThreads / 64; ++w) total = total + red[w];
  const float norm = (float)sqrt(total);
  if (tid == 0 && a.grad_norm) a.grad_norm[0] = norm;
  if (a.skip && !(fabsf(norm) <= 3.4028234663852886e38f)) {  // NaN or infinite: uniform
    if (tid == 0) a.skipped[0] = a.skipped[0] + 1;
    return;
  }

  // ---------------------------------------------------------------- phase 2: the update
  float coef = 1.0f, neg_step = 0.0f, bc2_sqrt = 1.0f;
  {
#pragma clang fp contract(off)
    if (a.clip) {
      const float c = a.max_norm / (norm + 1e-6f);
      coef = c > 1.0f ? 1.0f : c;  // torch.clamp(max=1): NaN stays NaN
    }
    if (a.kind != QT_OPT_SGD) {
      const double t = (double)(step + 1);
      const double bc1 = 1.0 - pow(a.beta1, t), bc2 = 1.0 - pow(a.beta2, t);
      neg_step = (float)(-(a.lr / bc1));
      bc2_sqrt = (float)sqrt(bc2);
    }
  }
  const bool first = step == 0 || a.sgd_plain;
  switch (a.kind) {  // uniform
    case QT_OPT_ADAM: update<QT_OPT_ADAM>(a, tid, first, coef, neg_step, bc2_sqrt); break;
    case QT_OPT_ADAMW: update<QT_OPT_ADAMW>(a, tid, first, coef, neg_step, bc2_sqrt); break;
    default: update<QT_OPT_SGD>(a, tid, first, coef, neg_step, bc2_sqrt); break;
  }
  if (tid == 0) a.step[0] = step + 1;
  if (!a.block) return;

  // ---------------------------------------------------------------- phase 3: the pack
  __syncthreads();  // the workgroup's stores to theta are visible to its loads
  const GradLayout& g = a.lay;
  float* part = a.block;
  pack_part(a.theta, part, first_part(g), tid, [&](int rem) { return first_source(g, rem); });
  part += first_part(g);
  for (int L = 1; L < g.nh; ++L, part += hidden_part(g))  // uniform
    pack_part(a.theta, part, hidden_part(g), tid, [&](int rem) { return hidden_source(g, L, rem); });
  pack_part(a.theta, part, output_part(g), tid, [&](int rem) { return output_source(g, rem); });
}

// tiles of 32 of the widest hidden layer, rounded up to 1, 2 or 4 (0: invalid shape; qt_policy's rules but
// for params, which the step does not read)
int optim_tiles(const qt_policy* p) {
  if (!p || p->n_hidden < 1 || p->n_hidden > QT_POLICY_MAX_HIDDEN) return 0;
  if (p->activation < QT_ACT_RELU || p->activation > QT_ACT_LEAKY_RELU) return 0;
  int wmax = 0;
  for (int i = 0; i < p->n_hidden; ++i) {
    if (p->width[i] < 1 || p->width[i] > QT_POLICY_MAX_WIDTH) return 0;
    wmax = p->width[i] > wmax ? p->width[i] : wmax;
  }
  const int t = (wmax + 31) / 32;
  return t == 3 ? 4 : t;
}

bool rate(double x) { return std::isfinite(x) && x >= 0.0; }

bool valid_optim(const qt_policy_optim* o) {
  if (!o || !o->theta || !o->m || !o->step || !o->skipped) return false;
  if (o->kind != QT_OPT_ADAM && o->kind != QT_OPT_SGD && o->kind != QT_OPT_ADAMW) return false;
  if (o->kind != QT_OPT_SGD && !o->v) return false;
  if (!rate(o->lr) || !rate(o->weight_decay) || !rate(o->eps) || !rate(o->momentum)) return false;
  if (!(o->beta1 >= 0.0 && o->beta1 < 1.0) || !(o->beta2 >= 0.0 && o->beta2 < 1.0)) return false;
  return !std::isnan(o->max_norm);
}

int launch_step(const qt_policy* shape, int nt, const qt_policy_optim* o, const float* grad, float* grad_norm,
                hipStream_t s) {
  OptArgs a{};
  a.lay = grad_layout(shape, nt);
  a.kind = o->kind, a.skip = o->skip_nonfinite != 0, a.clip = o->max_norm > 0.0;
  a.lerp_low = 1.0 - o->beta1 < 0.5, a.sgd_plain = o->momentum == 0.0;
  a.flat = (int)a.lay.flat, a.block_floats = (int)policy_block_floats(a.lay.nh, nt);
  a.beta1 = o->beta1, a.beta2 = o->beta2, a.lr = o->lr;
  a.max_norm = (float)o->max_norm, a.wd = (float)o->weight_decay;
  a.shrink = (float)(1.0 - o->lr * o->weight_decay);
  a.w1 = (float)(1.0 - o->beta1), a.b1 = (float)o->beta1, a.b2 = (float)o->beta2, a.w2 = (float)(1.0 - o->beta2);
  a.eps = (float)o->eps, a.momentum = (float)o->momentum, a.neg_lr = (float)(-o->lr);
  a.grad = grad, a.theta = o->theta, a.m = o->m, a.v = o->v, a.step = o->step, a.skipped = o->skipped;
  a.block = o->block, a.grad_norm = grad_norm;
  optim_kernel<<<1, kOptThreads, 0, s>>>(a);
  return check_launch();
}

}  // namespace

extern "C" {

int qt_policy_optim_version(void) { return 1; }

int qt_policy_optim_step(const qt_policy* shape, const qt_policy_optim* opt, const float* grad, void* stream) {
  const int nt = optim_tiles(shape);
  if (nt == 0 || !grad || !valid_optim(opt)) return QT_EINVAL;
  return launch_step(shape, nt, opt, grad, opt->grad_norm, (hipStream_t)stream);
}

int qt_policy_imitation_fit(const qt_policy* policy, const qt_policy_optim* opt, const qt_policy_fit_io* io,
                            void* stream) {
  const int nt = optim_tiles(policy);
  if (nt == 0 || !io || !valid_optim(opt)) return QT_EINVAL;
  if (!policy->params || !opt->block || policy->params != opt->block) return QT_EINVAL;
  if (!io->features || !io->targets || !io->order || !io->grad || !io->losses || !io->workspace) return QT_EINVAL;
  if (io->rows < 1 || io->m_total < 1 || io->batch < 1 || !std::isfinite(io->weight)) return QT_EINVAL;
  const int64_t widest = io->batch < io->m_total ? io->batch : io->m_total;
  const int64_t need = qt_policy_grad_workspace(policy, widest);  // < 0: more samples than the gradient entry takes
  if (need < 0 || io->workspace_bytes < need) return QT_EINVAL;
  qt_policy_grad_io g{};
  g.features = io->features, g.targets = io->targets, g.rows = io->rows, g.weight = io->weight;
  g.grad = io->grad, g.workspace = io->workspace, g.workspace_bytes = io->workspace_bytes;
  int64_t k = 0;
  for (int64_t at = 0; at < io->m_total; at += io->batch, ++k) {
    g.index = io->order + at;
    g.m = io->m_total - at < io->batch ? io->m_total - at : io->batch;
    g.loss = io->losses + k;
    int rc = qt_policy_imitation_grad(policy, &g, stream);
    if (rc != QT_OK) return rc;
    rc = launch_step(policy, nt, opt, io->grad, io->norms ? io->norms + k : opt->grad_norm, (hipStream_t)stream);
    if (rc != QT_OK) return rc;
  }
  return QT_OK;
}

}  // extern "C"
