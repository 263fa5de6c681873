// kstep_kernels.hpp -- k-step prediction error of many same-shape models over recorded trajectories (gfx950).
//
// Reference: autompc/evaluation/model_metrics.py:12-43 (get_model_rmse) and :45-111 (get_model_rmsmens).
// The reference runs, for every horizon h separately, h batched model steps from every start point
// (trajectory i, time t) with t + h <= L_i - 1 and compares the last prediction with obs[t + h].  The start
// points of horizon h are exactly those whose remaining length rem = L_i - 1 - t is at least h, so ONE
// rollout of kmax steps per start point gives the error sums of every horizon 1..kmax at once: step j of a
// row counts towards horizon j when j <= rem.
//
// Layout.  A row is one start point, rows of all trajectories concatenated (row_base[r] = index of its
// observation in the concatenated obs / ctrls arrays, row_rem[r] = rem; rows past the last one carry
// rem = 0).  A workgroup runs a tile of 16*MT rows of ONE model; the tile's states
// stay in the first-layer operand lds[L.xu] as in mlp_forward_kernel, and every step
//   loads control row base + j - 1 into the control columns, runs the net (mlp_tile.hpp),
//   sets x <- x + net output and, over the first obs_dim state entries,
//   sq    += (x_d - obs[base + j]_d)^2
//   dsq   += ((x_d - x_prev_d) - (obs[base + j]_d - obs[base + j - 1]_d)) * inv_std_d)^2     (optional: RMSMENS)
// Errors are formed in f64 from the model-precision state (an f32 state widens exactly, as it does on the
// host after pred_batch).
//
// Masking.  Rows with j > rem keep running (their states are garbage, possibly inf / NaN): their control
// and observation indices are clamped into the row's own trajectory and their error is dropped by a
// SELECT, never multiplied by 0 (0 * inf = NaN).
//
// Models.  One launch per model, each with that model's own descriptor (grid (tiles, 1), `model` names the
// model's slice of the partials and of init).  The byte-offset table of a plan with several models
// (model_delta_of / shift_model, mlp_tile.hpp) is not used here: in this run-time-shape kernel a shifted copy
// of the descriptor is demoted to scratch memory (456 B per lane, measured with
// -Rpass-analysis=kernel-resource-usage), while the descriptor read in place as the kernel argument keeps the
// kernel free of scratch.  Models of one shape share one tile geometry, so every launch has the same cost.
//
// Determinism.  No atomics: per step, every row's error is summed over d in order, the tile's rows in
// order by one thread, and the per-tile partials part[m][tile][j] are reduced over tiles in order by
// kstep_reduce_kernel.  Same inputs, same bits, whatever else runs on the device.
#pragma once
#include "mlp_tile.hpp"

namespace ampc {

struct KstepArgs {
  const double* obs;          // [total][obs_dim]
  const double* ctrls;        // [total][nu]
  const double* init;         // [n_models][total][nx] or nullptr (state = observation)
  const double* inv_std;      // [obs_dim] (only read when dpart != nullptr)
  const int* row_base;        // [n_rows]
  const int* row_rem;         // [n_rows]
  double* part;               // [n_models][tiles][kmax]
  double* dpart;              // same, delta errors; nullptr: not asked for
  long long total;            // concatenated trajectory rows
  int n_rows, tiles, kmax, obs_dim;
  int err_off;                // LDS offset (in doubles) of the error scratch [2][M][obs_dim] + [2][M]
};

template <typename T, int NT, int MT, int W, typename SH = DynShape, bool WIDE = false>
__global__ __launch_bounds__(64 * W) void kstep_error_kernel(const MlpDev<T> mlp_in, const TileLds L_in,
                                                             const KstepArgs a, int model) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* lds = reinterpret_cast<T*>(smem_raw);
  using Net = TileNet<T, NT, MT, W, false, 0, SH, WIDE>;
  constexpr int M = 16 * MT, NTHR = 64 * W;
  const int tile = blockIdx.x;
  const int first = tile * M;
  const MlpDev<T> mlp = SH::template fold<T>(mlp_in);
  const TileLds L = SH::template fold_lds<T, M, W>(L_in);
  const int tid = threadIdx.x, nx = mlp.nx, nu = mlp.nu, od = a.obs_dim;
  const bool want_d = a.dpart != nullptr;
  T* xu = lds + L.xu;
  double* err = reinterpret_cast<double*>(smem_raw) + a.err_off;     // [M][od]
  double* derr = err + M * od;                                         // [M][od]
  double* rsum = derr + M * od;                                        // [2][M]
  Net net;
  net.init(mlp);
  tile_load_constants<T, W>(mlp, L, lds, M);
  __syncthreads();
  // initial states: the observation (or the caller's model state) at the start point
  for (int i = tid; i < M * nx; i += NTHR) {
    const int row = i / nx, col = i - row * nx;
    const int gr = first + row;
    const long long b = gr < a.n_rows ? a.row_base[gr] : 0;
    double v = 0.0;
    if (gr < a.n_rows)
      v = a.init != nullptr ? a.init[((long long)model * a.total + b) * nx + col] : a.obs[b * od + col];
    xu[row * L.xu_stride + col] = (T)v;
  }
  const size_t pbase = ((size_t)model * a.tiles + tile) * a.kmax;
  for (int j = 1; j <= a.kmax; ++j) {
    for (int i = tid; i < M * nu; i += NTHR) {
      const int row = i / nu, col = i - row * nu;
      const int gr = first + row;
      const int rem = gr < a.n_rows ? a.row_rem[gr] : 0;
      const long long b = gr < a.n_rows ? a.row_base[gr] : 0;
      const int c = (j < rem ? j : rem) - 1;                         // clamped: never past the trajectory
      xu[row * L.xu_stride + nx + col] = (T)a.ctrls[(b + (c > 0 ? c : 0)) * nu + col];
    }
    __syncthreads();
    net.run(mlp, L, lds);
    for (int i = tid; i < M * nx; i += NTHR) {
      const int row = i / nx, col = i - row * nx;
      const T x = xu[row * L.xu_stride + col];
      const T xn = x + Net::output(mlp, L, lds, row, col);
      xu[row * L.xu_stride + col] = xn;
      if (col < od) {
        const int gr = first + row;
        const int rem = gr < a.n_rows ? a.row_rem[gr] : 0;
        const long long b = gr < a.n_rows ? a.row_base[gr] : 0;
        const int k = j < rem ? j : rem;
        const double o = a.obs[(b + k) * od + col];
        const double e = (double)xn - o;
        err[row * od + col] = e * e;
        if (want_d) {
          const double op = a.obs[(b + (k > 0 ? k - 1 : 0)) * od + col];
          const double dd = (((double)xn - (double)x) - (o - op)) * a.inv_std[col];
          derr[row * od + col] = dd * dd;
        }
      }
    }
    __syncthreads();
    if (tid < M) {
      const int gr = first + tid;
      const bool counted = gr < a.n_rows && j <= a.row_rem[gr];
      double s = 0.0, ds = 0.0;
      for (int d = 0; d < od; ++d) s += err[tid * od + d];
      if (want_d)
        for (int d = 0; d < od; ++d) ds += derr[tid * od + d];
      rsum[tid] = counted ? s : 0.0;
      rsum[M + tid] = counted ? ds : 0.0;
    }
    __syncthreads();
    if (tid == 0) {
      double s = 0.0, ds = 0.0;
      for (int r = 0; r < M; ++r) { s += rsum[r]; ds += rsum[M + r]; }
      a.part[pbase + j - 1] = s;
      if (want_d) a.dpart[pbase + j - 1] = ds;
    }
    // (the next writes to err / rsum follow the barriers inside the next net.run)
  }
}

// out[m][j] = sum over tiles, in tile order, of part[m][tile][j]  (T: the model precision of the unit that
// launches it -- one symbol per translation unit)
template <typename T>
__global__ void kstep_reduce_kernel(const double* __restrict__ part, double* __restrict__ out, int n_models,
                                    int tiles, int kmax) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_models * kmax) return;
  const int m = i / kmax, j = i - m * kmax;
  double s = 0.0;
  for (int t = 0; t < tiles; ++t) s += part[((size_t)m * tiles + t) * kmax + j];
  out[i] = s;
}

}  // namespace ampc
