// mlpfit_kernels.hpp -- the reference's MLP training step (autompc/sysid/mlp.py:177-217) for a TABLE of models
// (gfx950, f64 only): gathered mini-batch, forward act(A W' + b), SmoothL1Loss(beta = 1, mean), backward, Adam.
//
// One launch per layer forward and one per layer backward; grid y is the model, and a model that has no layer `l`
// (or a workgroup past the model's own tiles) returns at once.  Every ordering between layers and steps is a kernel
// boundary on one stream: no flags, no grid barrier, no atomics.
//
//   forward  (layer l, 256 threads = four waves per 16 x 16 output tile):
//     out = A_l W_l' + b_l over the nb rows of the step; hidden layer: A_{l+1} = act(out); output layer:
//     g_l = dSmoothL1(out - target) / (nb * out_dim).  A_0 is the feed gathered through the model's row order.
//   backward (layer l, 512 threads = eight waves per block J of 16 INPUT columns of W_l):
//     phase A (l > 0)   g_{l-1}[:, J] = (g_l W_l[:, J]) * act'(A_l[:, J])      reads W_l[:, J] only
//     -- workgroup barrier --
//     phase B           gW[:, J] = g_l' A_l[:, J], then Adam on W_l[:, J], m, v  writes W_l[:, J] only
//     The LAST workgroup of the grid's x owns no columns: it runs phase B against a column of ones -- the bias
//     gradient, the column sums of g_l -- and applies Adam to b_l ("bias = weight of a constant-1 input").
//   No workgroup reads a weight another one writes in the same launch.
//
// Sums.  A 16 x 16 tile accumulates with v_mfma_f64_16x16x4_f64 over the reduction index in blocks of 16: lane
// quad q takes indices 16 kb + 4 q + t, t = 0..3 of block kb (any fixed assignment is a valid sum order; this one
// gives every lane four consecutive values of a row-major operand).  Indices past the end contribute exact zeros.
// What bounds a tile is the latency of its operand loads (an activation written by the previous launch comes from
// beyond the reader's L2), not its MFMAs, so a wave requests a CHUNK of four blocks (32 values per lane) at once, and
// where the reduction is long (forward, phase A) four waves split it: wave s takes the chunks 4 s + 16 j, the four
// partial tiles meet in LDS and are added in the order ((p0 + p1) + p2) + p3.
// The order depends on the model's own dimensions and nb only, so a model's bits do not depend on its neighbours.
// act' is taken from the activation's RESULT (relu: a > 0; tanh: 1 - a^2; sigmoid: a (1 - a); selu: a > 0 ? scale :
// a + scale alpha), so only the activations are kept.
#pragma once
#include <hip/hip_runtime.h>

#include "mlp_tile.hpp"

namespace ampc {

constexpr int kFitMaxLayers = kMaxHidden + 1;   // linear layers of a model (hidden + output)
constexpr int kFitMaxWidth = 256;               // hidden width
constexpr int kFitMaxIn = 80;                   // nx + nu
constexpr int kFitMaxOut = 64;                  // nx
constexpr int kFitMaxBatch = 4096;              // rows of a mini-batch
constexpr int kFitFwdThreads = 256;
constexpr int kFitBwdThreads = 512;
constexpr int kFitChunk = 4;                    // 16-index blocks a wave requests at once

// One model of the table (device memory).  Offsets are in doubles: w / b into the flat parameter buffer (and alike
// into both moment buffers), a / g into the plan's activation and gradient buffers.
struct MlpFitModel {
  int n_layers;                  // linear layers, 2..5
  int act;                       // activation kind (0 relu, 1 tanh, 2 sigmoid, 3 selu)
  int dims[kFitMaxLayers + 1];   // nx + nu, hidden widths, nx
  int pad_;
  double lr;
  long long w[kFitMaxLayers], b[kFitMaxLayers];
  long long a[kFitMaxLayers];    // a[l], l >= 1: A_l [nb][dims[l]] (a[0] unused: A_0 is the gathered feed)
  long long g[kFitMaxLayers];    // g[l]: gradient of the loss w.r.t. layer l's pre-activation output [nb][dims[l + 1]]
};

struct MlpFitArgs {
  const MlpFitModel* models;
  const double* feed;      // [n_rows][dims[0]]
  const double* target;    // [n_rows][dims[n_layers]]
  const int* idx;          // [K][n_rows] row order of the epoch
  double* params;          // caller's flat parameter buffer
  double* m;               // Adam's first moment, laid out as params
  double* v;               // ... second moment
  double* abuf;            // activations
  double* gbuf;            // gradients
  int n_rows, row0, nb, layer;
  double bc1, bc2_sqrt;    // 1 - beta1^t, sqrt(1 - beta2^t)
};

__device__ __forceinline__ double fit_act_deriv(int kind, double a) {
  switch (kind) {
    case 0: return a > 0.0 ? 1.0 : 0.0;
    case 1: return 1.0 - a * a;
    case 2: return a * (1.0 - a);
    default: {
      const double alpha = 1.6732632423543772848170429916717, scale = 1.0507009873554804934193349852946;
      return a > 0.0 ? scale : a + scale * alpha;
    }
  }
}

// Entry r of a model's row order, kept inside the data whatever the caller uploaded.
__device__ __forceinline__ int fit_row(const int* order, int r, int n_rows) {
  const int v = order[r];
  return v < 0 ? 0 : (v >= n_rows ? n_rows - 1 : v);
}

// torch.optim.Adam's single-tensor step (torch/optim/adam.py _single_tensor_adam, defaults: beta 0.9 / 0.999, eps
// 1e-8, no weight decay, no amsgrad): m.lerp_(g, 1 - b1); v = v b2 + (1 - b2) g g;
// p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps).
__device__ __forceinline__ void fit_adam(double* p, double* m, double* v, double p0, double m0, double v0, double g,
                                         double step_size, double bc2_sqrt) {
  const double b1 = 0.9, b2 = 0.999, eps = 1e-8;
  const double m1 = m0 + (g - m0) * (1.0 - b1);
  const double v1 = v0 * b2 + (1.0 - b2) * g * g;
  *m = m1;
  *v = v1;
  const double denom = sqrt(v1) / bc2_sqrt + eps;
  *p = p0 - step_size * (m1 / denom);
}

// One chunk of a tile's reduction: blocks kb0 .. kb0 + 3, all operand loads first.  la(k) / lb(k): the lane's A / B
// operand at reduction index k (0 when the lane's row / column or k is outside).
template <typename LA, typename LB>
__device__ __forceinline__ d4 fit_chunk(d4 acc, int kb0, int q, LA&& la, LB&& lb) {
  double av[4 * kFitChunk], bv[4 * kFitChunk];
#pragma unroll
  for (int c = 0; c < kFitChunk; ++c)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int k = (kb0 + c) * 16 + 4 * q + t;
      av[4 * c + t] = la(k);
      bv[4 * c + t] = lb(k);
    }
#pragma unroll
  for (int e = 0; e < 4 * kFitChunk; ++e) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[e], bv[e], acc, 0, 0, 0);
  return acc;
}

// ---- forward -----------------------------------------------------------------------------------------------------
// grid (tiles, K), 256 threads.  Tile t of a model = (row tile t / ct, column tile t % ct), ct = ceil(out / 16).
__global__ __launch_bounds__(kFitFwdThreads) void mlpfit_forward_kernel(const MlpFitArgs a) {
  __shared__ double part[4][256];
  const MlpFitModel& md = a.models[blockIdx.y];
  const int l = a.layer;
  if (l >= md.n_layers) return;
  const int in = md.dims[l], out = md.dims[l + 1], nb = a.nb;
  const int ct = (out + 15) / 16, rt = (nb + 15) / 16;
  const int tile = blockIdx.x;
  if (tile >= ct * rt) return;                               // (the whole workgroup: before the barrier)
  const int r0 = (tile / ct) * 16, c0 = (tile % ct) * 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, q = lane >> 4;
  const int* order = a.idx + (size_t)blockIdx.y * a.n_rows + a.row0;

  // operands: A_l row r0 + i, W_l row c0 + i
  const int arow = r0 + i, wrow = c0 + i;
  const bool a_ok = arow < nb, w_ok = wrow < out;
  const double* ap = a.feed;
  if (a_ok) ap = l == 0 ? a.feed + (size_t)fit_row(order, arow, a.n_rows) * in : a.abuf + md.a[l] + (size_t)arow * in;
  const double* wp = a.params + md.w[l] + (size_t)(w_ok ? wrow : 0) * in;
  // what this thread's epilogue element needs (wave w finishes accumulator register r = w: row r0 + q + 4 w, column
  // c0 + i), requested before the products so that it arrives under them
  const int col = c0 + i, row = r0 + q + 4 * wave;
  const bool e_ok = col < out && row < nb, last = l == md.n_layers - 1;
  double bias = 0.0, want = 0.0;
  if (e_ok) {
    bias = a.params[md.b[l] + col];
    if (last) want = a.target[(size_t)fit_row(order, row, a.n_rows) * out + col];
  }
  d4 acc = {0.0, 0.0, 0.0, 0.0};
  const int nkb = (in + 15) / 16;
  for (int kb0 = kFitChunk * wave; kb0 < nkb; kb0 += 4 * kFitChunk)
    acc = fit_chunk(acc, kb0, q, [&](int k) { return (a_ok && k < in) ? ap[k] : 0.0; },
                    [&](int k) { return (w_ok && k < in) ? wp[k] : 0.0; });
#pragma unroll
  for (int r = 0; r < 4; ++r) part[wave][r * 64 + lane] = acc[r];
  __syncthreads();
  const int e = wave * 64 + lane;
  const double sum = ((part[0][e] + part[1][e]) + part[2][e]) + part[3][e];
  if (!e_ok) return;
  const double z = sum + bias;
  if (!last) {
    a.abuf[md.a[l + 1] + (size_t)row * out + col] = act_apply<double>(md.act, z);
  } else {
    const double d = z - want;
    const double s = fabs(d) < 1.0 ? d : (d > 0.0 ? 1.0 : -1.0);
    a.gbuf[md.g[l] + (size_t)row * out + col] = s * (1.0 / ((double)nb * (double)out));
  }
}

// ---- backward ----------------------------------------------------------------------------------------------------
// grid (ceil(max in / 16) + 1, K), 512 threads.  Workgroup jb owns input columns [16 jb, 16 jb + 16) of W_l; the
// last workgroup of x owns the bias.
__global__ __launch_bounds__(kFitBwdThreads) void mlpfit_backward_kernel(const MlpFitArgs a) {
  __shared__ double part[kFitBwdThreads / 64][256];
  const MlpFitModel& md = a.models[blockIdx.y];
  const int l = a.layer;
  if (l >= md.n_layers) return;
  const int in = md.dims[l], out = md.dims[l + 1], nb = a.nb;
  const bool bias_wg = blockIdx.x == gridDim.x - 1;
  const int j0 = blockIdx.x * 16;
  if (!bias_wg && j0 >= in) return;                          // (the whole workgroup: before any barrier)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, q = lane >> 4;
  const int* order = a.idx + (size_t)blockIdx.y * a.n_rows + a.row0;
  const double* g = a.gbuf + md.g[l];                        // [nb][out]
  double* W = a.params + md.w[l];                            // [out][in]
  const double step_size = md.lr / a.bc1;
  const int col = j0 + i;
  const bool col_ok = !bias_wg && col < in;

  // phase A: g_{l-1}[:, J] from the weights as they are before this step's update.  Two row tiles per pass, each
  // split over four waves.
  if (l > 0 && !bias_wg) {
    const double* A = a.abuf + md.a[l];                      // [nb][in], the activation's result
    double* gp = a.gbuf + md.g[l - 1];                       // [nb][in]
    const int rt = (nb + 15) / 16, nkb = (out + 15) / 16;
    for (int t0 = 0; t0 < rt; t0 += kFitBwdThreads / 256) {
      const int t = t0 + (wave >> 2), s = wave & 3;
      // the element this thread finishes after the barrier; its activation is requested now
      const int tt = tid >> 8, e = tid & 255, ln = e & 63;
      const int row = (t0 + tt) * 16 + (ln >> 4) + 4 * (e >> 6), c = j0 + (ln & 15);
      const bool e_ok = row < nb && c < in;
      const double act_out = e_ok ? A[(size_t)row * in + c] : 0.0;
      d4 acc = {0.0, 0.0, 0.0, 0.0};
      if (t < rt) {
        const int grow = t * 16 + i;                         // A operand: g_l[row][o]
        const bool g_ok = grow < nb;
        const double* gr = g + (size_t)(g_ok ? grow : 0) * out;
        for (int kb0 = kFitChunk * s; kb0 < nkb; kb0 += 4 * kFitChunk)
          acc = fit_chunk(acc, kb0, q, [&](int k) { return (g_ok && k < out) ? gr[k] : 0.0; },
                          [&](int k) { return (col_ok && k < out) ? W[(size_t)k * in + col] : 0.0; });   // W_l[o][J]
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) part[wave][r * 64 + lane] = acc[r];
      __syncthreads();
      if (e_ok) {
        const double sum = ((part[4 * tt][e] + part[4 * tt + 1][e]) + part[4 * tt + 2][e]) + part[4 * tt + 3][e];
        gp[(size_t)row * in + c] = sum * fit_act_deriv(md.act, act_out);
      }
      __syncthreads();
    }
  }
  __syncthreads();            // every read of W_l[:, J] above precedes every write below

  // phase B: gW[:, J] = g_l' A_l[:, J] (bias workgroup: g_l' 1) and Adam on it; one output tile per wave
  {
    const int ot = (out + 15) / 16, nkb = (nb + 15) / 16;
    for (int t = wave; t < ot; t += kFitBwdThreads / 64) {
      const int o = t * 16 + i;                              // A operand: g_l[r][o] (as [o][r])
      const bool o_ok = o < out;
      // the four parameters this lane updates (offsets into params / m / v), requested before the products
      size_t pe[4];
      bool p_ok[4];
      double p0[4], m0[4], v0[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int orow = t * 16 + q + 4 * r;
        p_ok[r] = orow < out && (bias_wg ? i == 0 : col_ok);
        pe[r] = bias_wg ? (size_t)md.b[l] + orow : (size_t)md.w[l] + (size_t)orow * in + col;
        p0[r] = m0[r] = v0[r] = 0.0;
        if (p_ok[r]) { p0[r] = a.params[pe[r]]; m0[r] = a.m[pe[r]]; v0[r] = a.v[pe[r]]; }
      }
      d4 acc = {0.0, 0.0, 0.0, 0.0};
      for (int kb0 = 0; kb0 < nkb; kb0 += kFitChunk)
        acc = fit_chunk(acc, kb0, q, [&](int r) { return (o_ok && r < nb) ? g[(size_t)r * out + o] : 0.0; },
                        [&](int r) {                         // B operand: A_l[r][J]
                          if (r >= nb) return 0.0;
                          if (bias_wg) return 1.0;
                          if (!col_ok) return 0.0;
                          return l == 0 ? a.feed[(size_t)fit_row(order, r, a.n_rows) * in + col]
                                        : a.abuf[md.a[l] + (size_t)r * in + col];
                        });
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (p_ok[r])
          fit_adam(a.params + pe[r], a.m + pe[r], a.v + pe[r], p0[r], m0[r], v0[r], acc[r], step_size, a.bc2_sqrt);
    }
  }
}

}  // namespace ampc
