// qt_policy_grad.hip — the imitation loss of the deep tracking policy and its
// gradient with respect to every weight and bias (include/quadtrack.h,
// "imitation-loss gradient").  Layout, summation and reduction order:
// qt_policy_grad.hpp.  Built with the default flags, as qt_policy.hip (exact
// f32: no relaxed math), so the forward half gives qt_policy_action's bits.
#include <cmath>

#include "qt_policy_grad.hpp"

using namespace qtg;

namespace {

struct GradArgs {
  const float* features;  // [rows][18]
  const float* targets;   // [rows][4]
  const int64_t* index;   // NULL or [m]
  int64_t m, tiles;
  float c;          // (float)(weight * 2 / (4 m))
  const float* wt;  // transposed hidden-layer blocks (workspace)
  float* part;      // [G][flat] running partial gradients (workspace)
  double* lpart;    // [G] partial sums of squared errors (workspace)
  float* pred;      // NULL or [m][4]
  GradLayout lay;
};

// T_L[mt][k][l] = W_L[2 k + (l >> 5)][32 mt + (l & 31)] for the hidden layers L = 1..nh-1, read from the
// packed block's A[mt'][kt'][r][l'] = W[32 mt' + (l' & 31)][32 kt' + crow(r, l' >> 5)]
template <int NT>
__global__ __launch_bounds__(kBlock) void transpose_kernel(const float* __restrict__ w, int nh, float* __restrict__ wt) {
  constexpr int HP = 32 * NT, LAYER = NT * NT * 1024;
  const int e = blockIdx.x * kBlock + threadIdx.x;
  if (e >= (nh - 1) * LAYER) return;
  const int L = e / LAYER, rem = e % LAYER;  // L: hidden layer L + 1
  const int mt = rem / (NT * 1024), k = (rem >> 6) % (HP / 2), l = rem & 63;
  const int i = 2 * k + (l >> 5), j = 32 * mt + (l & 31);
  const int q = j & 31, r = 4 * (q >> 3) + (q & 3), hb = (q >> 2) & 1;
  const float* base = w + NT * 9 * 64 + HP + L * (LAYER + HP);
  wt[e] = base[(((i >> 5) * NT + (j >> 5)) * 16 + r) * 64 + 32 * hb + (i & 31)];
}

// one 32-unit tile of a layer (both sample tiles), activated, to LDS as [unit][sample]
__device__ __forceinline__ void store_tile(float* Hl, int act, int mt, const f32x16& c0, const f32x16& c1, int half,
                                           int col) {
  f32x16 h[2][1];
  h[0][0] = c0, h[1][0] = c1;
  activate_tiles<1>(act, h);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float* d = Hl + (32 * mt + 8 * (r >> 2) + 4 * half + (r & 3)) * kGradLds + col;
    d[0] = h[0][0][r], d[32] = h[1][0][r];
  }
}

// One wave per workgroup; 64 samples per tile, one per lane in the forward half.
template <int NT, int NH>
__global__ __launch_bounds__(64) void grad_kernel(PolicyDev P, GradArgs a) {
  constexpr int HP = 32 * NT, S = kGradLds, HS = HP * S;
  __shared__ float lds[(kPolicyIn + NH * HP) * S + 4 * 64];
  float* X = lds;                           // features [input][sample]
  float* H = lds + kPolicyIn * S;           // per layer [unit][sample]: h, later delta
  float* DO = lds + (kPolicyIn + NH * HP) * S;  // delta of the output layer [row][sample]
  const int lane = threadIdx.x, half = lane >> 5, col = lane & 31;
  const GradLayout& g = a.lay;
  float* part = a.part + (int64_t)blockIdx.x * g.flat;
  double lsum = 0.0;
  bool first = true;
  for (int64_t t = blockIdx.x; t < a.tiles; t += gridDim.x, first = false) {
    const int64_t p = 64 * t + lane;
    const bool live = p < a.m;
    const int64_t q = live ? p : a.m - 1;
    const int64_t row = a.index ? a.index[q] : q;
    float f[kPolicyIn];
#pragma unroll
    for (int j = 0; j < kPolicyIn; ++j) f[j] = a.features[row * kPolicyIn + j];
    __syncthreads();  // the previous tile's reads of LDS are done
#pragma unroll
    for (int j = 0; j < kPolicyIn; ++j) X[j * S + lane] = f[j];

    // ---------------------------------------------------------------- forward half (qt_policy.hpp's policy_forward)
    float b0[9], b1[9];
#pragma unroll
    for (int s = 0; s < 9; ++s) {
      b0[s] = f[2 * s], b1[s] = f[2 * s + 1];
      half_swap(b0[s], b1[s]);
    }
    // The hidden layers' B operands are read back from LDS (register r of tile kt is row crow(r, half) of
    // H[L-1]) instead of kept in registers: the same operands in the same order, and no variant has to hold
    // two layers' accumulators at once.
    const float* w = P.w;
    {
      const float* bias = w + NT * 9 * 64;
      for (int mt = 0; mt < NT; ++mt) {
        f32x16 c;
#pragma unroll
        for (int r = 0; r < 16; ++r) c[r] = bias[32 * mt + 8 * (r >> 2) + 4 * half + (r & 3)];
        f32x16 c0 = c, c1 = c;
#pragma unroll
        for (int s = 0; s < 9; ++s) {
          const float av = w[(mt * 9 + s) * 64 + lane];
          c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0[s], c0, 0, 0, 0);
          c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1[s], c1, 0, 0, 0);
        }
        store_tile(H, P.act, mt, c0, c1, half, col);
      }
      w = bias + HP;
    }
#pragma nounroll
    for (int L = 1; L < NH; ++L) {
      __syncthreads();
      const float* bias = w + NT * NT * 16 * 64;
      const float* Hp = H + (L - 1) * HS;
      for (int mt = 0; mt < NT; ++mt) {
        f32x16 c;
#pragma unroll
        for (int r = 0; r < 16; ++r) c[r] = bias[32 * mt + 8 * (r >> 2) + 4 * half + (r & 3)];
        f32x16 c0 = c, c1 = c;
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float av = w[((mt * NT + kt) * 16 + r) * 64 + lane];
            const float* hv = Hp + (32 * kt + 8 * (r >> 2) + 4 * half + (r & 3)) * S + col;
            c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, hv[0], c0, 0, 0, 0);
            c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, hv[32], c1, 0, 0, 0);
          }
        store_tile(H + L * HS, P.act, mt, c0, c1, half, col);
      }
      w = bias + HP;
    }
    __syncthreads();
    // output layer on the VALU: this lane's sample, inputs in index order
    const float* wo = w;
    const float* bo = w + 4 * HP;
    float* Hl = H + (NH - 1) * HS;
    float y[4] = {bo[0], bo[1], bo[2], bo[3]};
#pragma unroll 8
    for (int k = 0; k < HP; ++k) {
      const float v = Hl[k * S + lane];
#pragma unroll
      for (int i = 0; i < 4; ++i) y[i] = fmaf(wo[i * HP + k], v, y[i]);
    }
    float dout[4];
    double e = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma clang fp contract(off)
      const float s = 1.0f / (1.0f + expf(-y[i]));
      const float mm = s * P.scale[i];
      const float u = mm + P.lo[i];
      if (a.pred && live) a.pred[p * 4 + i] = u;
      const float d = u - a.targets[row * 4 + i];
      const float d2 = d * d;
      e = e + (double)d2;
      float gq = d * a.c;
      gq = gq * P.scale[i];
      gq = gq * (1.0f - s);
      gq = gq * s;
      dout[i] = live ? gq : 0.0f;
    }
    if (!live) e = 0.0;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) e = e + __shfl_xor(e, o, 64);
    lsum = lsum + e;
#pragma unroll
    for (int i = 0; i < 4; ++i) DO[i * 64 + lane] = dout[i];
    __syncthreads();

    // ---------------------------------------------------------------- backward half
    {  // output layer's weights and bias: lane = input unit
      const int wi = g.in[NH];
      for (int k = lane; k < wi; k += 64) {
        float acc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = first ? 0.0f : part[g.w[NH] + i * wi + k];
        for (int s = 0; s < 64; ++s) {
          const float hv = Hl[k * S + s];
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[i] = fmaf(DO[i * 64 + s], hv, acc[i]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) part[g.w[NH] + i * wi + k] = acc[i];
      }
      if (lane < 4) {
        float acc = first ? 0.0f : part[g.b[NH] + lane];
        for (int s = 0; s < 64; ++s) acc = acc + DO[lane * 64 + s];
        part[g.b[NH] + lane] = acc;
      }
    }
    __syncthreads();
    // the last hidden layer's delta over its activations
#pragma unroll 8
    for (int k = 0; k < HP; ++k) {
      const float v = Hl[k * S + lane];
      float dp = wo[k] * dout[0];
#pragma unroll
      for (int i = 1; i < 4; ++i) dp = fmaf(wo[i * HP + k], dout[i], dp);
      Hl[k * S + lane] = dp * activation_slope(P.act, v);
    }
    __syncthreads();
#pragma nounroll
    for (int L = NH - 1; L >= 0; --L) {
      float* D = H + L * HS;
      const int no = g.out[L], ni = g.in[L];
      for (int i = lane; i < no; i += 64) {  // bias: lane = unit
        float acc = first ? 0.0f : part[g.b[L] + i];
        for (int s = 0; s < 64; ++s) acc = acc + D[i * S + s];
        part[g.b[L] + i] = acc;
      }
      // dW_L = delta_L h_{L-1}^T
      const float* B = L > 0 ? H + (L - 1) * HS : X;
      for (int mt = 0; mt < NT; ++mt) {
        if (32 * mt >= no) break;  // uniform: a tile of padding rows
        float av[32];
#pragma unroll
        for (int k = 0; k < 32; ++k) av[k] = D[(32 * mt + col) * S + 2 * k + half];
        for (int nt = 0; nt < (L > 0 ? NT : 1); ++nt) {
          if (32 * nt >= ni) break;  // uniform
          const int j = 32 * nt + col;
          const bool jin = j < ni;
          float* dst = part + g.w[L] + j;
          f32x16 c;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int i = 32 * mt + 8 * (r >> 2) + 4 * half + (r & 3);
            c[r] = (!first && jin && i < no) ? dst[(int64_t)i * ni] : 0.0f;
          }
          const float* Bj = B + (jin ? j : 0) * S + half;
#pragma unroll
          for (int k = 0; k < 32; ++k) {
            const float bv = Bj[2 * k];
            c = __builtin_amdgcn_mfma_f32_32x32x2f32(av[k], jin ? bv : 0.0f, c, 0, 0, 0);
          }
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int i = 32 * mt + 8 * (r >> 2) + 4 * half + (r & 3);
            if (jin && i < no) dst[(int64_t)i * ni] = c[r];
          }
        }
      }
      if (L > 0) {  // delta_{L-1} = (W_L^T delta_L) * act'(h_{L-1}), over H[L-1]
        __syncthreads();
        float* Hp = H + (L - 1) * HS;
        const float* T = a.wt + (int64_t)(L - 1) * NT * NT * 1024;
        for (int mt = 0; mt < NT; ++mt) {
          f32x16 c0, c1;
#pragma unroll
          for (int r = 0; r < 16; ++r) c0[r] = 0.0f, c1[r] = 0.0f;
#pragma unroll 8
          for (int k = 0; k < HP / 2; ++k) {
            const float aw = T[(mt * (HP / 2) + k) * 64 + lane];
            const float d0 = D[(2 * k + half) * S + col], d1 = D[(2 * k + half) * S + 32 + col];
            c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(aw, d0, c0, 0, 0, 0);
            c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(aw, d1, c1, 0, 0, 0);
          }
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int idx = (32 * mt + 8 * (r >> 2) + 4 * half + (r & 3)) * S + col;
            const float v0 = Hp[idx], v1 = Hp[idx + 32];
            Hp[idx] = c0[r] * activation_slope(P.act, v0);
            Hp[idx + 32] = c1[r] * activation_slope(P.act, v1);
          }
        }
        __syncthreads();
      }
    }
  }
  if (lane == 0) a.lpart[blockIdx.x] = lsum;
}

// grad = the rows added in chunks of kGradFold: inside a chunk in ascending order, then the chunk sums in
// ascending order; loss = (sum of lpart in the same order) * weight / (4 m)
template <typename T>
__device__ __forceinline__ T fold_rows(const T* __restrict__ p, int G, int64_t stride) {
  T acc = 0;
  for (int c = 0; c < G; c += kGradFold) {
    T s = p[(int64_t)c * stride];
    const int end = c + kGradFold < G ? c + kGradFold : G;
    for (int gi = c + 1; gi < end; ++gi) s = s + p[(int64_t)gi * stride];
    acc = c == 0 ? s : acc + s;
  }
  return acc;
}

__global__ __launch_bounds__(kBlock) void fold_kernel(const float* __restrict__ part, const double* __restrict__ lpart,
                                                      int G, int64_t flat, double lscale, float* __restrict__ grad,
                                                      double* __restrict__ loss) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e < flat) grad[e] = fold_rows(part + e, G, flat);
  if (e == 0) loss[0] = fold_rows(lpart, G, 1) * lscale;
}

// tiles of 32 of the widest hidden layer, rounded up to 1, 2 or 4 (0: invalid policy; qt_policy's rules)
int grad_policy_tiles(const qt_policy* p) {
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

constexpr int64_t kGradMaxSamples = (int64_t)1 << 40;

int64_t workspace_bytes(const qt_policy* p, int nt, int64_t m) {
  const GradLayout g = grad_layout(p, nt);
  const int64_t G = grad_groups(m);
  return G * 8 + 4 * (grad_transposed_floats(g.nh, nt) + G * g.flat);
}

template <int NT>
int launch_grad(const PolicyDev& P, const GradArgs& a, int G, hipStream_t s) {
  switch (a.lay.nh) {
    case 1: grad_kernel<NT, 1><<<G, 64, 0, s>>>(P, a); break;
    case 2: grad_kernel<NT, 2><<<G, 64, 0, s>>>(P, a); break;
    case 3: grad_kernel<NT, 3><<<G, 64, 0, s>>>(P, a); break;
    default: grad_kernel<NT, 4><<<G, 64, 0, s>>>(P, a); break;
  }
  return check_launch();
}

}  // namespace

extern "C" {

int qt_policy_grad_version(void) { return 1; }

int64_t qt_policy_grad_workspace(const qt_policy* policy, int64_t m) {
  const int nt = grad_policy_tiles(policy);
  if (nt == 0 || m < 1 || m > kGradMaxSamples) return -1;
  return workspace_bytes(policy, nt, m);
}

int qt_policy_imitation_grad(const qt_policy* policy, const qt_policy_grad_io* io, void* stream) {
  const int nt = grad_policy_tiles(policy);
  if (nt == 0 || !io) return QT_EINVAL;
  if (!io->features || !io->targets || !io->grad || !io->loss || !io->workspace) return QT_EINVAL;
  if (io->m < 1 || io->m > kGradMaxSamples || io->rows < 1 || (!io->index && io->rows < io->m)) return QT_EINVAL;
  if (!std::isfinite(io->weight)) return QT_EINVAL;
  if (io->workspace_bytes < workspace_bytes(policy, nt, io->m)) return QT_EINVAL;
  PolicyDev P{};
  P.w = policy->params, P.nh = policy->n_hidden, P.act = policy->activation;
  for (int i = 0; i < 4; ++i) {
    P.scale[i] = (float)(policy->hi[i] - policy->lo[i]);
    P.lo[i] = (float)policy->lo[i];
  }
  GradArgs a{};
  a.lay = grad_layout(policy, nt);
  const int G = (int)grad_groups(io->m);
  a.features = io->features, a.targets = io->targets, a.index = io->index;
  a.m = io->m, a.tiles = grad_tiles(io->m);
  a.c = (float)(io->weight * 2.0 / (4.0 * (double)io->m));
  a.lpart = (double*)io->workspace;
  float* wt = (float*)(a.lpart + G);
  a.wt = wt;
  a.part = wt + grad_transposed_floats(a.lay.nh, nt);
  a.pred = io->pred;
  hipStream_t s = (hipStream_t)stream;
  const int nT = (int)grad_transposed_floats(a.lay.nh, nt);
  int rc = QT_OK;
  if (nT > 0) {
    if (nt == 1)
      transpose_kernel<1><<<grid_of(nT), kBlock, 0, s>>>(P.w, P.nh, wt);
    else if (nt == 2)
      transpose_kernel<2><<<grid_of(nT), kBlock, 0, s>>>(P.w, P.nh, wt);
    else
      transpose_kernel<4><<<grid_of(nT), kBlock, 0, s>>>(P.w, P.nh, wt);
    rc = check_launch();
    if (rc != QT_OK) return rc;
  }
  rc = nt == 1 ? launch_grad<1>(P, a, G, s) : nt == 2 ? launch_grad<2>(P, a, G, s) : launch_grad<4>(P, a, G, s);
  if (rc != QT_OK) return rc;
  fold_kernel<<<grid_of(a.lay.flat), kBlock, 0, s>>>(a.part, a.lpart, G, a.lay.flat,
                                                     io->weight / (4.0 * (double)io->m), io->grad, io->loss);
  return check_launch();
}

}  // extern "C"
