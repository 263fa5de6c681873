// kstep_mlp_kernels.hpp -- k-step prediction error of a TABLE of MLP models of any mix of depth, widths and activation
// over recorded trajectories in one launch (gfx950, f64 only): the contract of kstep_error_kernel (kstep_kernels.hpp:
// one rollout of kmax steps per start point yields the error sums of every horizon 1..kmax; row_base / row_rem; control
// and observation indices of rows past their horizon clamped into the row's own trajectory; their error dropped by a
// SELECT, never multiplied by 0) on a model step that reads plain parameters.
//
// Models.  Grid (row tiles, models).  A workgroup reads its model through models[blockIdx.y], field by field through
// the pointer (wave-uniform loads; no by-value copy of the entry is made, so the run-time layer loop indexes memory,
// not a register array: mlp_tile.hpp, MlpDev::delta).  An entry holds n_layers, act, dims[] and, per layer, the
// addresses of the weight [out][in] (row-major, torch.nn.Linear's layout) and the bias [out], plus those of the four
// normalisers.  Nothing is packed per shape: the parameters are read where the fit left them.
//
// Step (the reference's MLP.pred_batch, autompc/sysid/mlp.py:229-236, unfolded):
//   in = ([x, u] - xu_mean) / xu_std;  a_{l+1} = act(a_l W_l' + b_l);  x' = x + (z dy_std + dy_mean), z the output layer.
// Geometry, the same for every model: 16 rows per tile, 256 threads = four waves.  LDS (doubles):
//   act[2][16][257]  the two activation buffers (odd row stride: conflict-free fragment reads); the normalised input is
//                    written into act[1], layer l reads act[(l + 1) & 1] and writes act[l & 1]
//   x[16][65]        the raw state
//   norm[288]        xu_mean[80] xu_std[80] dy_mean[64] dy_std[64]
//   rsum[2][16]      a step's row sums;  rows[2][16] (int) row_base / row_rem of the tile
// 76 800 bytes: two workgroups per CU.  The output layer leaves no activations, so its epilogue writes the step's
// squared errors [16][nx] (and delta errors) into columns 96.. / 160.. of the buffer it does NOT read, act[(n_layers - 1)
// & 1]: no other access of a step touches those columns between that epilogue and the row sums (the input occupies
// columns < 80 of act[1]; the next layer to write the buffer follows a barrier behind the row sums).
//
// A layer is v_mfma_f64_16x16x4_f64 over 16-column output tiles; wave w takes the tiles w, w + 4, w + 8, w + 12 and
// runs them side by side on one read of the A fragments.  A comes from LDS, W from global memory / L2: lane (i, q)
// takes k = 16 kb + 4 q + t, t = 0..3, of weight row 16 tile + i -- four consecutive doubles per request -- and the
// next block's weights are in flight under the MFMAs of the current one (two blocks per request spill: 249 VGPRs as it
// is).
//
// Padding.  Reduction indices k >= in are selected to exact zeros on BOTH operands in the one group of a layer that
// holds them; weight rows >= out are read from row out - 1 and land in columns that are never stored as results: a
// hidden layer stores 0 there, so a padded activation (sigmoid(0) = 0.5) never exists.  Rows past n_rows start from 0
// and behave as rows with rem = 0.
//
// Sums.  Output element (row, col) accumulates over k in blocks of 16 in order, inside a block as the MFMA does (t =
// 0..3 in order, each the sum over q = 0..3 of the products at k = 16 kb + 4 q + t): a function of the layer's own `in`
// only.  Errors as in kstep_error_kernel: squared in f64, a row's sum over d in order by one thread, the tile's rows in
// order by one thread, the tiles in order by kstep_reduce_kernel.  No atomics.  A model's sums are the same bits
// alone, in any batch, at any position of it, and from run to run; a diverging model yields non-finite sums of its
// own, no index depends on a state value.
#pragma once
#include "kstep_kernels.hpp"

namespace ampc {

constexpr int kKmRows = 16;
constexpr int kKmThreads = 256;
constexpr int kKmWaves = kKmThreads / 64;
constexpr int kKmMaxLayers = kMaxHidden + 1;   // linear layers (hidden + output)
constexpr int kKmMaxWidth = 256, kKmMaxIn = 80, kKmMaxOut = 64, kKmMaxCtrl = 16;
constexpr int kKmMaxTiles = kKmMaxWidth / 16 / kKmWaves;   // column tiles of a wave
constexpr int kKmActStride = kKmMaxWidth + 1, kKmXStride = kKmMaxOut + 1;
constexpr int kKmGroup = 1;                                // 16-index blocks of the reduction per weight request
constexpr int kKmErrCol = 96, kKmDerrCol = kKmErrCol + kKmMaxOut;
static_assert(kKmMaxOut <= 16 * kKmWaves, "the output layer is one tile per wave");
static_assert(kKmErrCol >= kKmMaxIn && kKmDerrCol + kKmMaxOut <= kKmActStride, "error columns lie behind the input");
// LDS map, in doubles
constexpr int kKmOffAct = 0;
constexpr int kKmOffX = 2 * kKmRows * kKmActStride;
constexpr int kKmOffNorm = kKmOffX + kKmRows * kKmXStride;
constexpr int kKmOffRsum = kKmOffNorm + 2 * kKmMaxIn + 2 * kKmMaxOut;
constexpr int kKmOffRows = kKmOffRsum + 2 * kKmRows;                    // 2 * 16 ints = 16 doubles
constexpr size_t kKmLdsBytes = (size_t)(kKmOffRows + kKmRows) * 8;

// One model of the table (device memory); every pointer is a device address.
struct KstepMlpModel {
  int n_layers;                         // linear layers, 2..5
  int act;                              // 0 relu, 1 tanh, 2 sigmoid, 3 selu
  int dims[kKmMaxLayers + 1];           // nx + nu, hidden widths, nx
  const double* w[kKmMaxLayers];        // [out][in] row-major
  const double* b[kKmMaxLayers];        // [out]
  const double* norm[4];                // xu_mean [nx + nu], xu_std [nx + nu], dy_mean [nx], dy_std [nx]
};

struct KstepMlpArgs {
  const double* obs;          // [total][nx]
  const double* ctrls;        // [total][nu]
  const double* inv_std;      // [nx] (only read when dpart != nullptr)
  const int* row_base;        // [n_rows]
  const int* row_rem;         // [n_rows]
  double* part;               // [n_models][tiles][kmax]
  double* dpart;              // same, delta errors; nullptr: not asked for
  int n_rows, tiles, kmax, nx, nu;
};

// The weights of one request group -- kKmGroup blocks from kb0 -- of a wave's NT tiles.  k0 = 16 kb0 + 4 q.
template <int NT, bool RAGGED>
__device__ __forceinline__ void km_fetch(double (&bv)[NT][4 * kKmGroup], const double* __restrict__ W, const int (&roff)[NT],
                                         int k0, int in) {
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int c = 0; c < kKmGroup; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = k0 + 16 * c + e;
        if constexpr (RAGGED) bv[t][4 * c + e] = k < in ? W[roff[t] + k] : 0.0;
        else bv[t][4 * c + e] = W[roff[t] + k];
      }
}
template <int NT>
__device__ __forceinline__ void km_fetch_group(double (&bv)[NT][4 * kKmGroup], const double* __restrict__ W,
                                               const int (&roff)[NT], int g, int q, int in) {
  if (16 * kKmGroup * (g + 1) <= in) km_fetch<NT, false>(bv, W, roff, 16 * kKmGroup * g + 4 * q, in);      // (wave-uniform)
  else km_fetch<NT, true>(bv, W, roff, 16 * kKmGroup * g + 4 * q, in);
}

// acc[t] += A[:, group] W_t[:, group]'.  ap: the lane's row of the input buffer.
template <int NT, bool RAGGED>
__device__ __forceinline__ void km_mma(d4 (&acc)[NT], const double (&bv)[NT][4 * kKmGroup], const double* ap, int k0, int in) {
  double av[4 * kKmGroup];
#pragma unroll
  for (int c = 0; c < kKmGroup; ++c)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int k = k0 + 16 * c + e;
      if constexpr (RAGGED) av[4 * c + e] = k < in ? ap[k] : 0.0;
      else av[4 * c + e] = ap[k];
    }
#pragma unroll
  for (int x = 0; x < 4 * kKmGroup; ++x)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[x], bv[t][x], acc[t], 0, 0, 0);
}
template <int NT>
__device__ __forceinline__ void km_mma_group(d4 (&acc)[NT], const double (&bv)[NT][4 * kKmGroup], const double* ap, int g, int q,
                                             int in) {
  if (16 * kKmGroup * (g + 1) <= in) km_mma<NT, false>(acc, bv, ap, 16 * kKmGroup * g + 4 * q, in);
  else km_mma<NT, true>(acc, bv, ap, 16 * kKmGroup * g + 4 * q, in);
}

// What the output layer's epilogue needs besides the layer itself.
struct KmStep {
  double* x;                  // LDS state [16][kKmXStride]
  const double* norm;         // LDS normalisers
  const int* rows;            // LDS row_base[16] | row_rem[16]
  double* err;                // LDS: this model's error buffer (column 0 of it)
  int j;                      // the step, 1..kmax
};

// One layer for the NT tiles w, w + 4, ... of wave w: bout = act(bin W' + b), or -- last -- the state update and the
// step's errors.
template <int NT>
__device__ __forceinline__ void km_layer(const double* __restrict__ W, const double* __restrict__ B, int in, int out,
                                         int act, bool last, const double* bin, double* bout, int w, int lane,
                                         const KstepMlpArgs& a, const KmStep& s) {
  const int i = lane & 15, q = lane >> 4;
  int roff[NT], col[NT];
  double bias[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    col[t] = 16 * (w + kKmWaves * t) + i;
    const int wr = col[t] < out ? col[t] : out - 1;
    roff[t] = wr * in;
    bias[t] = B[wr];
  }
  d4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
  const double* ap = bin + i * kKmActStride;
  const int ng = (in + 16 * kKmGroup - 1) / (16 * kKmGroup);      // request groups
  double b0[NT][4 * kKmGroup], b1[NT][4 * kKmGroup];
  km_fetch_group<NT>(b0, W, roff, 0, q, in);
#pragma unroll 1
  for (int g = 0; g < ng; g += 2) {
    if (g + 1 < ng) km_fetch_group<NT>(b1, W, roff, g + 1, q, in);
    km_mma_group<NT>(acc, b0, ap, g, q, in);
    if (g + 2 < ng) km_fetch_group<NT>(b0, W, roff, g + 2, q, in);
    if (g + 1 < ng) km_mma_group<NT>(acc, b1, ap, g + 1, q, in);
  }
  // accumulator register r of lane (i, q): row q + 4 r, column col[t]
  if (!last) {
    // z = sum + bias goes to the output buffer first and the thread then applies the activation to its own elements
    // in place, one column tile (four values) at a time: all 4 NT values side by side would hold 200 registers in
    // the exponential's temporaries
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) bout[(q + 4 * r) * kKmActStride + col[t]] = acc[t][r] + bias[t];
#pragma unroll 1
    for (int t = 0; t < NT; ++t) {
      const int c = 16 * (w + kKmWaves * t) + i;
      double* p = bout + q * kKmActStride + c;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double v = act_apply<double>(act, p[4 * r * kKmActStride]);
        p[4 * r * kKmActStride] = c < out ? v : 0.0;
      }
    }
    return;
  }
  // (the output layer has at most kKmMaxOut / 16 = 4 tiles: one per wave)
  if constexpr (NT == 1) {
    const int c = col[0];
    if (c >= out) return;
    const bool want_d = a.dpart != nullptr;
    const int nx = a.nx;
    const double dm = s.norm[2 * kKmMaxIn + c], ds = s.norm[2 * kKmMaxIn + kKmMaxOut + c];
    const double inv = want_d ? a.inv_std[c] : 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = q + 4 * r;
      const double x = s.x[row * kKmXStride + c];
      const double xn = x + ((acc[0][r] + bias[0]) * ds + dm);
      s.x[row * kKmXStride + c] = xn;
      const long long b = s.rows[row];
      const int rem = s.rows[kKmRows + row];
      const int k = s.j < rem ? s.j : rem;                            // clamped: never past the trajectory
      const double o = a.obs[(b + k) * nx + c];
      const double e = xn - o;
      s.err[row * kKmActStride + kKmErrCol + c] = e * e;
      if (want_d) {
        const double op = a.obs[(b + (k > 0 ? k - 1 : 0)) * nx + c];
        const double dd = ((xn - x) - (o - op)) * inv;
        s.err[row * kKmActStride + kKmDerrCol + c] = dd * dd;
      }
    }
  }
}

// (a unit that shares the layer routines above with a kernel of its own -- mppi_table_kernels.hpp -- leaves this
//  kernel out: it is defined once, in launch_kstep_mlp.cpp)
#ifndef AMPC_KM_LAYERS_ONLY
__global__ __launch_bounds__(kKmThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) void kstep_mlp_table_kernel(const KstepMlpModel* __restrict__ models,
                                                                      const KstepMlpArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  double* lds = reinterpret_cast<double*>(smem_raw);
  const KstepMlpModel* md = models + blockIdx.y;
  const int nl = md->n_layers, act = md->act;
  const int nx = a.nx, nu = a.nu, kin = nx + nu;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile = blockIdx.x, first = tile * kKmRows;
  const bool want_d = a.dpart != nullptr;
  double* buf0 = lds + kKmOffAct;
  double* buf1 = buf0 + kKmRows * kKmActStride;
  double* xs = lds + kKmOffX;
  double* norm = lds + kKmOffNorm;
  double* rsum = lds + kKmOffRsum;
  int* rows = reinterpret_cast<int*>(lds + kKmOffRows);
  double* err = ((nl - 1) & 1) ? buf1 : buf0;

  for (int i = tid; i < kin; i += kKmThreads) {
    norm[i] = md->norm[0][i];
    norm[kKmMaxIn + i] = md->norm[1][i];
  }
  for (int i = tid; i < nx; i += kKmThreads) {
    norm[2 * kKmMaxIn + i] = md->norm[2][i];
    norm[2 * kKmMaxIn + kKmMaxOut + i] = md->norm[3][i];
  }
  if (tid < kKmRows) {
    const int gr = first + tid;
    rows[tid] = gr < a.n_rows ? a.row_base[gr] : 0;
    rows[kKmRows + tid] = gr < a.n_rows ? a.row_rem[gr] : 0;
  }
  __syncthreads();
  // thread (row = tid / 16, c = tid % 16) walks the columns c, c + 16, ... of its row
  const int trow = tid >> 4, tcol = tid & 15;
  const long long tbase = rows[trow];
  const int trem = rows[kKmRows + trow];
  const bool tlive = first + trow < a.n_rows;
  for (int c = tcol; c < nx; c += 16) xs[trow * kKmXStride + c] = tlive ? a.obs[tbase * nx + c] : 0.0;
  __syncthreads();

  const size_t pbase = ((size_t)blockIdx.y * a.tiles + tile) * a.kmax;
  // the row sums of step `step` (threads 0..15, one row each, d in order), then the tile's sum (thread 0, rows in order)
  auto row_sums = [&](int step) {
    const bool counted = first + tid < a.n_rows && step <= rows[kKmRows + tid];
    const double* e = err + tid * kKmActStride;
    double s = 0.0, ds = 0.0;
    for (int d = 0; d < nx; ++d) s += e[kKmErrCol + d];
    if (want_d)
      for (int d = 0; d < nx; ++d) ds += e[kKmDerrCol + d];
    rsum[tid] = counted ? s : 0.0;
    rsum[kKmRows + tid] = counted ? ds : 0.0;
  };
  auto tile_sum = [&](int step) {
    double s = 0.0, ds = 0.0;
    for (int r = 0; r < kKmRows; ++r) { s += rsum[r]; ds += rsum[kKmRows + r]; }
    a.part[pbase + step - 1] = s;
    if (want_d) a.dpart[pbase + step - 1] = ds;
  };

  KmStep st;
  st.x = xs; st.norm = norm; st.rows = rows; st.err = err;
  for (int j = 1; j <= a.kmax; ++j) {
    // the normalised input [x | u] of this step; control row base + j - 1, clamped into the row's trajectory
    {
      const int cj = (j < trem ? j : trem) - 1;
      const long long urow = tbase + (cj > 0 ? cj : 0);
      for (int c = tcol; c < kin; c += 16) {
        const double v = c < nx ? xs[trow * kKmXStride + c] : a.ctrls[urow * nu + (c - nx)];
        buf1[trow * kKmActStride + c] = (v - norm[c]) / norm[kKmMaxIn + c];
      }
    }
    if (j > 1 && tid < kKmRows) row_sums(j - 1);
    __syncthreads();
    if (j > 1 && tid == 0) tile_sum(j - 1);
    st.j = j;
    for (int l = 0; l < nl; ++l) {
      const int in = md->dims[l], out = md->dims[l + 1];
      const double* W = md->w[l];
      const double* B = md->b[l];
      const double* bin = ((l + 1) & 1) ? buf1 : buf0;
      double* bout = (l & 1) ? buf1 : buf0;
      const bool last = l == nl - 1;
      const int ct = (out + 15) / 16;
      const int ntw = w < ct ? (ct - w + kKmWaves - 1) / kKmWaves : 0;     // this wave's tiles (wave-uniform)
      static_assert(kKmMaxTiles == 4, "one case per tile count");
      switch (ntw) {
        case 1: km_layer<1>(W, B, in, out, act, last, bin, bout, w, lane, a, st); break;
        case 2: km_layer<2>(W, B, in, out, act, last, bin, bout, w, lane, a, st); break;
        case 3: km_layer<3>(W, B, in, out, act, last, bin, bout, w, lane, a, st); break;
        case 4: km_layer<4>(W, B, in, out, act, last, bin, bout, w, lane, a, st); break;
        default: break;
      }
      __syncthreads();
    }
  }
  if (tid < kKmRows) row_sums(a.kmax);
  __syncthreads();
  if (tid == 0) tile_sum(a.kmax);
}
#endif  // AMPC_KM_LAYERS_ONLY

}  // namespace ampc
