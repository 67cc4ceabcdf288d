// qt_policy_grad.hpp — the gradient of the imitation loss of the deep tracking
// policy (include/quadtrack.h, "imitation-loss gradient"), for 64 samples of a
// wavefront at once: qt_policy.hpp's forward pass restated with its
// activations kept, then the backward pass on the same f32-input MFMA
// (v_mfma_f32_32x32x2_f32).
//
//   loss = weight / (4 m) * sum_s sum_i (u_i(f_s) - t_{s,i})^2,
//   u = sigmoid(raw) * (float)(hi - lo) + lo   (PolicyNetwork.forward)
//
// Launches.  (1) transpose_kernel builds, in the workspace, every hidden
// layer's weights as the A operand of W^T (below) from the packed block.
// (2) grad_kernel: one wave per workgroup, G = min(tiles, kGradMaxGroups)
// workgroups, tiles = ceil(m / 64); workgroup g takes the sample tiles g,
// g + G, g + 2 G, ... in ascending order and keeps a running partial gradient
// in its own workspace row (plain loads and stores of elements only this lane
// touches).  (3) fold_kernel adds the G rows.  No floating-point atomic is
// used anywhere, so the bits are a function of the inputs and of m alone.
//
// Forward half.  qt_policy.hpp's arithmetic: the same MFMA sequence and
// summation order for the first and the hidden layers, the same fmaf chain in
// index order for the 4-row output layer (its inputs read back from LDS
// instead of exchanged between the lane halves: the same numbers), the same
// output stage.  So pred is bit for bit qt_policy_action's command.  Every
// layer's post-activation tile goes to LDS as H[L][unit][sample] (row stride
// kGradLds = 65 floats, so that a read down a column of 32 units meets 32
// different banks), the features as X[input][sample].  A hidden layer reads
// its B operands back from H[L-1] (register r of tile kt is row crow(r, half))
// instead of keeping them in registers: the same operands in the same order,
// and no variant holds two layers' accumulators at once (none spills).
//
// Backward half.  Derivatives come from the post-activation value h (relu:
// h > 0 ? 1 : 0; leaky_relu: h > 0 ? 1 : 0.1; tanh: 1 - h^2; elu: h > 0 ? 1 :
// h + 1: torch's values at a pre-activation of exactly 0).
//   output layer (VALU):  d_i = u_i - t_i;  delta_out_i = ((d_i c) scale_i (1 - s_i)) s_i
//     with s the sigmoid and c = (float)(weight * 2 / (4 m)), formed in double
//     on the host and applied here once.  A lane past m runs the whole pass on
//     sample m - 1 and its delta_out is forced to +0, so it adds exact zeros.
//   last hidden layer:    delta[k] = (sum_i Wout[i][k] delta_out_i, i = 0..3 in
//     order) * act'(h[k]), per lane, written over H[nh-1][k][sample].
//   dW_L = delta_L h_{L-1}^T:  samples are the K dimension.  A operand of
//     k-step k: delta_L[32 mt + (l & 31)][2 k + (l >> 5)], B operand:
//     h_{L-1}[32 nt + (l & 31)][2 k + (l >> 5)] (layer 0: the features, inputs
//     18-31 zero), both read from LDS.  The accumulator starts from the
//     workgroup's running partial (zero at its first tile), then the 64
//     samples of the tile are added in ascending order.
//   delta_{L-1} = (W_L^T delta_L) * act'(h_{L-1}):  A operand of k-step k:
//     T_L[mt][k][l] = W_L[2 k + (l >> 5)][32 mt + (l & 31)], one coalesced
//     256-byte load from the transposed block; B operand: delta_L[2 k +
//     (l >> 5)][sample] from LDS.  Sum from zero over the units of layer L in
//     index order 0, 1, 2, ...  The result is written over H[L-1].
//   biases and the output layer's weights (VALU, lane = unit): the running
//     partial, then the tile's samples 0..63 in ascending order.
// Padding rows and columns carry exact zeros through both halves and have no
// element in the partial rows or in the result.
//
// Reduction order of one gradient element, a function of m alone:
//   row g   = (((0 + tile g) + tile g + G) + tile g + 2 G) + ..., each tile's
//             samples in ascending order inside the MFMA / fmaf chain above;
//   grad    = the rows in chunks of kGradFold = 32: chunk c = ((row 32 c + row 32 c + 1) + ...) + row 32 c + 31,
//             grad = ((chunk 0 + chunk 1) + chunk 2) + ...
// The loss: per sample the f32 squares d_i * d_i widened to FP64 and added for
// i = 0..3; per tile a butterfly over the 64 lanes (xor 32, 16, 8, 4, 2, 1);
// per workgroup the tiles in ascending order; then the rows as for grad, times
// weight / (4 m) in FP64.
//
// Workspace (qt_policy_grad_workspace bytes): double lpart[G]; float
// T[nh - 1][NT][16 NT][64]; float part[G][flat size].
#pragma once
#include "qt_policy.hpp"

namespace qtg {

using namespace qtp;

constexpr int kGradMaxGroups = 1024;  // workgroups of grad_kernel (4 per CU of an MI355X)
constexpr int kGradFold = 32;         // rows per chunk of fold_kernel's sum
constexpr int kGradLds = 65;          // floats between two LDS rows of 64 samples

// offsets of every layer in parameters_to_vector order: weight [out][in] row-major, then bias
struct GradLayout {
  int nh, nt;
  int in[5], out[5];   // layers 0..nh (nh: the output layer)
  int64_t w[5], b[5];  // element offsets of weight and bias
  int64_t flat;        // flat_size(hidden_sizes)
};

inline GradLayout grad_layout(const qt_policy* p, int nt) {
  GradLayout g{};
  g.nh = p->n_hidden, g.nt = nt;
  int64_t off = 0;
  for (int L = 0; L <= g.nh; ++L) {
    g.in[L] = L == 0 ? kPolicyIn : p->width[L - 1];
    g.out[L] = L == g.nh ? 4 : p->width[L];
    g.w[L] = off;
    g.b[L] = off + (int64_t)g.out[L] * g.in[L];
    off = g.b[L] + g.out[L];
  }
  g.flat = off;
  return g;
}

inline int64_t grad_tiles(int64_t m) { return (m + 63) / 64; }
inline int64_t grad_groups(int64_t m) { return grad_tiles(m) < kGradMaxGroups ? grad_tiles(m) : kGradMaxGroups; }
// floats of the transposed blocks
inline int64_t grad_transposed_floats(int nh, int nt) { return (int64_t)(nh - 1) * nt * nt * 1024; }

// activation'(x) from the post-activation value h
__device__ __forceinline__ float activation_slope(int act, float h) {
  switch (act) {  // uniform
    case QT_ACT_RELU: return h > 0.0f ? 1.0f : 0.0f;
    case QT_ACT_TANH: return 1.0f - h * h;
    case QT_ACT_ELU: return h > 0.0f ? 1.0f : h + 1.0f;
    default: return h > 0.0f ? 1.0f : 0.1f;
  }
}

}  // namespace qtg
