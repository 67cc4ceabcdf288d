// qt_policy.hpp — the deep tracking policy's forward pass on the f32-input
// MFMA (v_mfma_f32_32x32x2_f32), for the 64 episodes of a wavefront at once
// (reference: controllers/deep_tracking_policy.py, PolicyNetwork.forward and
// DeepTrackingPolicy._extract_features).
//
// Orientation.  Every layer is computed as W (out x in, the MFMA's A operand)
// times the activations (in x episodes, the B operand): the episodes are the
// N dimension, two tiles of 32 columns per wave (tile 0 = the wave's lanes
// 0-31, tile 1 = lanes 32-63), the output neurons the M dimension in tiles of
// 32 rows.  The accumulator of a 32x32 tile holds, in register r of lane l,
// row crow(r, l >> 5) = 8 (r >> 2) + 4 (l >> 5) + (r & 3) of column l & 31:
// exactly the shape of a B operand of two k values (k = l >> 5).  So register
// r of a layer's accumulator, after bias and activation, IS the B operand of
// the next layer's k-step r, when that step's A operand carries the weight
// columns crow(r, 0) (lanes 0-31) and crow(r, 1) (lanes 32-63).  The host
// packs the weights in that order (quadtrack/policy.py pack_params; layout
// below), so a step's A operand is one coalesced 256-byte load, and no value
// crosses between the lane halves from the first layer's accumulators to the
// last hidden layer's.  Only the 18 inputs (9 v_permlane32_swap) and the last
// hidden layer's activations (one swap per register pair, so that each lane
// holds its own episode's full vector for the 4-row output layer, which runs
// on the VALU with the weights in scalar registers) cross.
//
// Summation order of one output neuron, the same for every lane, batch size
// and entry point (the MFMA is a k-ordered fmaf chain per element, one
// rounding per product): accumulator = bias; first layer: inputs 0, 1, ..., 17;
// hidden layers: for every input tile of 32, registers r = 0..15, crow(r, 0)
// then crow(r, 1) (0, 4, 1, 5, 2, 6, 3, 7, 8, 12, ...); output layer: inputs
// 0, 1, 2, ... (fmaf chain).  Columns of an MFMA are independent, so an
// episode's result does not depend on the other lanes of its wave.
// tests/policy_model.py restates this order as a host program and
// tests/test_gpu_policy_model.py holds the kernels to it: a change of the
// order changes this paragraph and that model together.
//
// MFMA ignores EXEC: every lane of a wave must reach policy_forward (callers
// keep the lanes of a partial last wave and of finished episodes alive and
// mask only their loads and stores).
//
// Packed parameter block (floats; NT = tiles of 32 of the widest hidden layer,
// rounded up to 1, 2 or 4; HP = 32 NT; rows and columns beyond a layer's real
// size are zero, and every activation maps 0 to 0, so padding adds exact zeros):
//   layer 0:      A[NT][9][64]      A[mt][s][l] = W0[32 mt + (l & 31)][2 s + (l >> 5)]
//                 bias[HP]
//   layer 1..H-1: A[NT][NT][16][64] A[mt][kt][r][l] = W[32 mt + (l & 31)][32 kt + crow(r, l >> 5)]
//                 bias[HP]
//   output:       W[4][HP] row-major, bias[4]
#pragma once
#include "qt_kernels.hpp"

namespace qtp {

using namespace qtk;

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct PolicyDev {
  const float* w;  // packed block (above)
  int nh;          // hidden layers, 1..4
  int act;         // enum qt_activation
  float scale[4];  // (float)(hi - lo), as torch multiplies a float32 tensor by a Python float
  float lo[4];
};

constexpr int kPolicyIn = 18;

// floats of the packed block
__host__ __device__ constexpr int64_t policy_block_floats(int nh, int nt) {
  const int64_t hp = 32 * nt;
  return (int64_t)nt * 9 * 64 + hp + (int64_t)(nh - 1) * ((int64_t)nt * nt * 16 * 64 + hp) + 4 * hp + 4;
}

// DeepTrackingPolicy._extract_features (deep_tracking_policy.py:241-286): the
// differences in FP64 (numpy float64), then .astype(float32)
__device__ __forceinline__ void policy_features(const double* qp, const double* qv, const double* att,
                                                const double* rate, const double* tp, const double* tv, float* f) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    f[i] = (float)(tp[i] - qp[i]);
    f[3 + i] = (float)(tv[i] - qv[i]);
    f[6 + i] = (float)att[i];
    f[9 + i] = (float)rate[i];
    f[12 + i] = (float)tp[i];
    f[15 + i] = (float)tv[i];
  }
}

// nn.ReLU / nn.Tanh / nn.ELU / nn.LeakyReLU(0.1) on one accumulator register
template <int ACT>
__device__ __forceinline__ float activate(float x) {
  if (ACT == QT_ACT_RELU) return x < 0.0f ? 0.0f : x;  // NaN stays NaN
  if (ACT == QT_ACT_TANH) return tanhf(x);
  if (ACT == QT_ACT_ELU) return x > 0.0f ? x : expm1f(x);
  return x > 0.0f ? x : x * 0.1f;
}

template <int NT>
__device__ __forceinline__ void activate_tiles(int act, f32x16 (&h)[2][NT]) {
  auto all = [&](auto tag) {
    constexpr int A = decltype(tag)::value;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int mt = 0; mt < NT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) h[nt][mt][r] = activate<A>(h[nt][mt][r]);
  };
  switch (act) {  // uniform
    case QT_ACT_RELU: all(std::integral_constant<int, QT_ACT_RELU>{}); break;
    case QT_ACT_TANH: all(std::integral_constant<int, QT_ACT_TANH>{}); break;
    case QT_ACT_ELU: all(std::integral_constant<int, QT_ACT_ELU>{}); break;
    default: all(std::integral_constant<int, QT_ACT_LEAKY_RELU>{}); break;
  }
}

// lanes 32-63 of a exchange with lanes 0-31 of b (v_permlane32_swap)
__device__ __forceinline__ void half_swap(float& a, float& b) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  a = __uint_as_float(r[0]);
  b = __uint_as_float(r[1]);
}

// PolicyNetwork.forward of the wave's 64 episodes: f[18] this lane's features,
// u[4] its bounded command, sigmoid(raw) * (hi - lo) + lo in f32 (two
// roundings, as torch's mul and add), widened exactly to FP64.
template <int NT>
__device__ __forceinline__ void policy_forward(const PolicyDev& P, const float* f, double* u) {
  constexpr int HP = 32 * NT;
  const int lane = threadIdx.x & 63, half = lane >> 5;
  // first layer's B operands: step s holds inputs 2 s (lanes 0-31) and 2 s + 1
  // (lanes 32-63) of the tile's 32 episodes
  float b0[9], b1[9];
#pragma unroll
  for (int s = 0; s < 9; ++s) {
    b0[s] = f[2 * s], b1[s] = f[2 * s + 1];
    half_swap(b0[s], b1[s]);  // b0: episodes 0-31 (tile 0), b1: episodes 32-63 (tile 1)
  }
  const float* w = P.w;
  f32x16 h[2][NT];
  {
    const float* bias = w + NT * 9 * 64;
#pragma unroll
    for (int mt = 0; mt < NT; ++mt) {
      f32x16 c;
#pragma unroll
      for (int r = 0; r < 16; ++r) c[r] = bias[32 * mt + 8 * (r >> 2) + 4 * half + (r & 3)];
      f32x16 c0 = c, c1 = c;
#pragma unroll
      for (int s = 0; s < 9; ++s) {
        const float a = w[(mt * 9 + s) * 64 + lane];
        c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0[s], c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1[s], c1, 0, 0, 0);
      }
      h[0][mt] = c0, h[1][mt] = c1;
    }
    activate_tiles<NT>(P.act, h);
    w = bias + HP;
  }
  for (int L = 1; L < P.nh; ++L) {  // uniform
    const float* bias = w + NT * NT * 16 * 64;
    f32x16 g[2][NT];
#pragma unroll
    for (int mt = 0; mt < NT; ++mt) {
      f32x16 c;
#pragma unroll
      for (int r = 0; r < 16; ++r) c[r] = bias[32 * mt + 8 * (r >> 2) + 4 * half + (r & 3)];
      f32x16 c0 = c, c1 = c;
#pragma unroll
      for (int kt = 0; kt < NT; ++kt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float a = w[((mt * NT + kt) * 16 + r) * 64 + lane];
          c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, h[0][kt][r], c0, 0, 0, 0);
          c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, h[1][kt][r], c1, 0, 0, 0);
        }
      g[0][mt] = c0, g[1][mt] = c1;
    }
    activate_tiles<NT>(P.act, g);
#pragma unroll
    for (int mt = 0; mt < NT; ++mt) h[0][mt] = g[0][mt], h[1][mt] = g[1][mt];
    w = bias + HP;
  }
  // output layer on the VALU: each lane gathers its own episode's activations
  // (after the swap, h[0] holds row crow(r, 0) and h[1] row crow(r, 1) of the
  // lane's episode), weights and bias from uniform addresses
  const float* bo = w + 4 * HP;
  float y[4] = {bo[0], bo[1], bo[2], bo[3]};
#pragma unroll
  for (int kt = 0; kt < NT; ++kt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float lo = h[0][kt][r], hi = h[1][kt][r];
      half_swap(lo, hi);
      h[0][kt][r] = lo, h[1][kt][r] = hi;
    }
#pragma unroll
  for (int k = 0; k < HP; ++k) {  // inputs in index order
    const int q = k & 31, r = 4 * (q >> 3) + (q & 3);
    const float v = h[(q >> 2) & 1][k >> 5][r];
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = fmaf(w[i * HP + k], v, y[i]);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma clang fp contract(off)
    const float s = 1.0f / (1.0f + expf(-y[i]));
    const float m = s * P.scale[i];
    u[i] = (double)(m + P.lo[i]);
  }
}

}  // namespace qtp
