// qt_policy_optim.hpp — gradient clipping, the optimiser step and the packing
// of the new parameters, for the deep tracking policy's flat f32 parameter
// vector (include/quadtrack.h, "clip + optimiser step"): what
// clip_grad_norm_, torch.optim.{Adam, AdamW, SGD}.step() and
// quadtrack.policy.pack_params do, in one launch.
//
// One workgroup of kOptThreads = 1024 threads (16 waves on one CU).  The flat
// vector has 27 .. 52,484 elements, so the launch is latency-bound, and a
// second workgroup would have to read *step while the first one writes it.
//
// Phase 1, the norm.  Thread t adds (double)g_i * (double)g_i (exact: two
// 24-bit significands) for i = t, t + 1024, t + 2048, ... in ascending order
// into one FP64 accumulator that starts at +0; a wave adds its 64 lanes by a
// butterfly (xor 32, 16, 8, 4, 2, 1); the 16 wave sums go through LDS and
// every thread adds them in wave order 0..15.  norm = (float)sqrt(sum), the
// FP64 square root correctly rounded.  Every thread holds the same bits.
//
// Phase 2, the update (thread t: elements t, t + 1024, ..., loaded in batches
// of eight before the arithmetic so that a batch costs one trip to memory),
// each line one IEEE f32 operation, no contraction; sc(x) is the double x
// rounded to f32:
//   coef = min(1, sc(max_norm) / (norm + 1e-6f))      (max_norm > 0, else no clip; NaN stays NaN)
//   g = g_i * coef
//   Adam, SGD:  g = g + sc(weight_decay) * theta      (weight_decay != 0)
//   AdamW:      theta = theta * sc(1 - lr weight_decay)
//   Adam, AdamW (t = *step + 1, bc1 = 1 - pow(beta1, t), bc2 = 1 - pow(beta2, t) in double):
//     m = m + sc(1 - beta1) * (g - m)                 (1 - beta1 < 0.5, torch's lerp; else g - (g - m) * sc(beta1))
//     v = v * sc(beta2) + (sc(1 - beta2) * g) * g
//     theta = theta + (sc(-lr / bc1) * m) / (sqrt(v) / sc(sqrt(bc2)) + sc(eps))
//   SGD:  m = g at *step == 0 or momentum == 0, else m * sc(momentum) + g;  theta = theta + sc(-lr) * m
// With skip_nonfinite set and a NaN or infinite norm nothing of phases 2 and
// 3 runs; *skipped is incremented instead of *step.
//
// Phase 3, the pack, after a workgroup barrier: layer by layer, thread t
// writes elements t, t + 1024, ... of the layer's part of the block: element e
// is theta[block_source(e)], or +0 where block_source gives -1 (a row or
// column beyond a layer's size).  The map is the closed form of the layout
// quadtrack.h documents for qt_policy.params.
#pragma once
#include "qt_policy_grad.hpp"

namespace qto {

using namespace qtg;

constexpr int kOptThreads = 1024;

// The packed block is one part per layer, weights then bias; each function below gives, for element rem
// of its part, the index in the flat vector or -1 for padding, without a data-dependent branch (the kernel
// runs them in unrolled loops whose loads are in flight together).
__host__ __device__ inline int first_part(const GradLayout& g) { return g.nt * 576 + 32 * g.nt; }
__host__ __device__ inline int hidden_part(const GradLayout& g) { return g.nt * g.nt * 1024 + 32 * g.nt; }
__host__ __device__ inline int output_part(const GradLayout& g) { return 128 * g.nt + 4; }

// layer 0: A[NT][9][64], A[mt][s][l] = W0[32 mt + (l & 31)][2 s + (l >> 5)]; bias[HP]
__host__ __device__ inline int first_source(const GradLayout& g, int rem) {
  const int weights = g.nt * 576;
  const int mt = rem / 576, s = (rem >> 6) % 9, l = rem & 63;
  const int row = 32 * mt + (l & 31), col = 2 * s + (l >> 5);
  const int w = row < g.out[0] ? (int)g.w[0] + row * kPolicyIn + col : -1;
  const int i = rem - weights;
  const int b = i < g.out[0] ? (int)g.b[0] + i : -1;
  return rem < weights ? w : b;
}

// layer L = 1..nh-1: A[NT][NT][16][64], A[mt][kt][r][l] = W[32 mt + (l & 31)][32 kt + crow(r, l >> 5)]; bias[HP]
__host__ __device__ inline int hidden_source(const GradLayout& g, int L, int rem) {
  const int nt = g.nt, sh = nt >> 1, weights = nt * nt * 1024;  // nt = 1, 2, 4 = 1 << sh
  const int t = rem >> 10, mt = t >> sh, kt = t & (nt - 1), r = (rem >> 6) & 15, l = rem & 63;
  const int row = 32 * mt + (l & 31), col = 32 * kt + 8 * (r >> 2) + 4 * (l >> 5) + (r & 3);
  const int w = ((row < g.out[L]) & (col < g.in[L])) ? (int)g.w[L] + row * g.in[L] + col : -1;
  const int i = rem - weights;
  const int b = i < g.out[L] ? (int)g.b[L] + i : -1;
  return rem < weights ? w : b;
}

// output layer: W[4][HP] row-major; bias[4]
__host__ __device__ inline int output_source(const GradLayout& g, int rem) {
  const int nt = g.nt, sh = nt >> 1, hp = 32 * nt, weights = 4 * hp, nh = g.nh;
  const int i = rem >> (5 + sh), k = rem & (hp - 1);
  const int w = k < g.in[nh] ? (int)g.w[nh] + i * g.in[nh] + k : -1;
  return rem < weights ? w : (int)g.b[nh] + (rem - weights);
}

// element e of the whole block (the host's view of the three functions above; tests/test_policy_optim_cpu.py
// compares it with quadtrack.policy.pack_index)
__host__ __device__ inline int block_source(const GradLayout& g, int e) {
  if (e < first_part(g)) return first_source(g, e);
  e -= first_part(g);
  for (int L = 1; L < g.nh; ++L) {
    if (e < hidden_part(g)) return hidden_source(g, L, e);
    e -= hidden_part(g);
  }
  return output_source(g, e);
}

}  // namespace qto
