// kstep_linear_kernels.hpp -- k-step prediction error of WIDE linear models (65 .. 256 states) over recorded
// trajectories (gfx950): the contract of kstep_error_kernel (kstep_kernels.hpp: one rollout of kmax steps per start
// point yields the error sums of every horizon 1..kmax) on the LinDev machinery of linear_kernels.hpp.
//
// Layout.  A row is one start point (row_base / row_rem as in kstep_kernels.hpp, row_start = first row of the
// row's trajectory).  Grid (row tiles, models): a workgroup of kLinW waves owns 16 rows of ONE model.  [x | u]
// ping-pongs between two LDS buffers as in linear_rollout_kernel; step j is one lin_tile product per output tile
// (v_mfma_f64_16x16x4_f64 / the f32 form) from buffer (j - 1) & 1 into buffer j & 1, the controls of step j + 1 are
// loaded beside it, and ONE workgroup barrier ends the step.  The lanes that hold the first obs_dim output columns
// form the squared errors straight from their accumulators,
//   sq  = (x_d - obs[base + j]_d)^2
//   dsq = (((x_d - x_prev_d) - (obs[base + j]_d - obs[base + j - 1]_d)) * inv_std_d)^2          (optional: RMSMENS)
// (x_prev is still in the other buffer), in f64 from the model-precision state, into an LDS error block that is
// double buffered by step parity: the last wave sums step j - 1's block while the others run step j's product, so
// the error sums need no barrier of their own.
//
// Models of different state dimensions share a launch: the kernel reads its model's KstepLinDesc from a table in
// global memory, field by field through the pointer (uniform loads; a by-value copy of a run-time-shape descriptor
// chosen by blockIdx is demoted to scratch, see kstep_kernels.hpp).  Every LDS offset depends on obs_dim and on the
// model's OWN kp only; the launch reserves the bytes of the widest model.
//
// Initial states are formed on the device by the model's state rule:
//   0  rows supplied by the caller [total][nx] (or the observation itself when rows == nullptr and nx == obs_dim)
//   1  ARX gather (arx.py:62-76 without the row's own control): column c is obs / ctrls[max(t - lag, row_start)][j] or
//      the constant 1 (KstepLinCol), a pure copy: bit-identical to ARX.traj_to_states
//   2  Koopman lift (koopman.py:105-122), basis-major: column f * obs_dim + d = fn_f(obs[t][d]); powers as a
//      double-double running product rounded once, sin / cos the device library's (as lqr_kernels.hpp)
//
// Masking.  Rows with j > rem keep running with control / observation indices clamped into their own trajectory;
// their error is dropped by a SELECT, never multiplied by 0.  Rows past n_rows behave as rows with rem = 0.
//
// Determinism.  No atomics.  The tile height is 16 whatever the call holds; an output entry is one MFMA
// accumulator's k-ordered chain; a row's error is summed over d in order, the tile's rows in order by one lane, the
// per-tile partials part[m][tile][j] over tiles in order by kstep_lin_reduce_kernel.  A model's sums are the same
// bits alone, in any batch, in any position of it, and from run to run.
#pragma once
#include "linear_kernels.hpp"

namespace ampc {

struct KstepLinCol {
  int src;      // 0: the constant 1, 1: obs[row][j], 2: ctrls[row][j]
  int lag;      // row = max(t - lag, first row of the trajectory)
  int j;
};

struct KstepLinDesc {
  int nx, nu, kp, ntile, ksn;
  int rule;                    // 0 rows, 1 ARX gather, 2 lift
  const void* wf;              // [ntile][ksn][64] fragments of [A | B] in the model's precision (LinDev::wf)
  const double* rows;          // rule 0: [total][nx] or nullptr (state = observation)
  const KstepLinCol* cols;     // rule 1: [nx]
  const double* prog;          // rule 2: [nx / obs_dim][2] (kind, parameter): 0 identity, 1 power, 2 sin, 3 cos
};

struct KstepLinArgs {
  const double* obs;          // [total][obs_dim]
  const double* ctrls;        // [total][nu]
  const double* inv_std;      // [obs_dim] (only read when dpart != nullptr)
  const int* row_base;        // [n_rows]
  const int* row_rem;         // [n_rows]
  const int* row_start;       // [n_rows]
  double* part;               // [n_models][tiles][kmax]
  double* dpart;              // same, delta errors; nullptr: not asked for
  int n_rows, tiles, kmax, obs_dim;
};

// LDS: error blocks [2][16][obs_dim] (+ the same for the delta errors) in f64, the tile's row_base / row_rem, then
// the two [16][xs] operand buffers in the model precision
__host__ __device__ constexpr size_t kstep_lin_err_doubles(int obs_dim, bool delta) {
  return (size_t)(delta ? 4 : 2) * 16 * obs_dim;
}
__host__ __device__ constexpr size_t kstep_lin_lds_bytes(int obs_dim, bool delta, int kp, int esz) {
  return kstep_lin_err_doubles(obs_dim, delta) * 8 + 32 * 4 + (size_t)2 * 16 * lin_xs(kp, esz) * esz;
}

__device__ __forceinline__ double kstep_lin_lift(double o, int kind, double par) {
  if (kind == 1) {                       // o ** p rounded once (as state_lift_kernel)
    const int pw = (int)par;
    double h = pw >= 1 ? o : 1.0, l = 0.0;
    for (int k = 1; k < pw; ++k) {
      const double ph = h * o;
      const double pe = fma(h, o, -ph) + l * o;
      h = ph + pe;
      l = pe - (h - ph);
    }
    return h;
  }
  if (kind == 2) return sin(par * o);
  if (kind == 3) return cos(par * o);
  return o;
}

template <typename T>
__global__ __launch_bounds__(64 * kLinW) void kstep_linear_kernel(const KstepLinDesc* __restrict__ descs,
                                                                   const KstepLinArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  constexpr int M = 16, NTHR = 64 * kLinW;
  const KstepLinDesc* d = descs + blockIdx.y;
  LinDev<T> m;
  m.nx = d->nx; m.nu = d->nu; m.kp = d->kp; m.ntile = d->ntile; m.ksn = d->ksn;
  m.wf = static_cast<const T*>(d->wf);
  const int rule = d->rule;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int nx = m.nx, nu = m.nu, od = a.obs_dim, xs = lin_xs(m.kp, (int)sizeof(T));
  const bool want_d = a.dpart != nullptr;
  const int tile = blockIdx.x, first = tile * M;
  double* err = reinterpret_cast<double*>(smem_raw);                   // [2][M][od]
  double* derr = err + 2 * M * od;                                     // [2][M][od] (want_d)
  int* sb = reinterpret_cast<int*>(err + kstep_lin_err_doubles(od, want_d));
  int* srem = sb + M;
  T* xb0 = reinterpret_cast<T*>(srem + M);
  T* xb[2] = {xb0, xb0 + M * xs};

  for (int i = tid; i < 2 * M * xs; i += NTHR) xb0[i] = T(0);
  if (tid < M) {
    const int gr = first + tid;
    sb[tid] = gr < a.n_rows ? a.row_base[gr] : 0;
    srem[tid] = gr < a.n_rows ? a.row_rem[gr] : 0;
  }
  __syncthreads();
  // ---- initial states by the model's rule, and the controls of step 1 --------------------------------------
  for (int i = tid; i < M * nx; i += NTHR) {
    const int row = i / nx, col = i - row * nx;
    const int gr = first + row;
    double v = 0.0;
    if (gr < a.n_rows) {
      const long long b = sb[row];
      if (rule == 1) {
        const KstepLinCol c = d->cols[col];
        if (c.src == 0) v = 1.0;
        else {
          long long r = b - c.lag;
          const long long s0 = a.row_start[gr];
          if (r < s0) r = s0;
          v = c.src == 1 ? a.obs[r * od + c.j] : a.ctrls[r * nu + c.j];
        }
      } else if (rule == 2) {
        const int f = col / od, j = col - f * od;
        const double* prog = d->prog;
        v = kstep_lin_lift(a.obs[b * od + j], (int)prog[2 * f], prog[2 * f + 1]);
      } else {
        const double* rows = d->rows;
        v = rows != nullptr ? rows[b * nx + col] : a.obs[b * od + col];
      }
    }
    xb[0][row * xs + col] = (T)v;
  }
  // controls of step j into buffer `dst`: row base + min(j, rem) - 1, clamped into the row's own trajectory
  auto controls = [&](int j, T* dst) {
    for (int i = tid; i < M * nu; i += NTHR) {
      const int row = i / nu, col = i - row * nu;
      const int rem = srem[row];
      const int c = (j < rem ? j : rem) - 1;
      dst[row * xs + nx + col] = (T)a.ctrls[((long long)sb[row] + (c > 0 ? c : 0)) * nu + col];
    }
  };
  controls(1, xb[0]);
  // the four accumulator rows of this lane
  long long rb[4];
  int rr[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = acc_row<T>(lane >> 4, r);
    rb[r] = sb[row];
    rr[r] = srem[row];
  }
  const size_t pbase = ((size_t)blockIdx.y * a.tiles + tile) * a.kmax;
  // sums of step j's error block, by the last wave: rows over d in order, then the rows in order by lane 0
  auto reduce = [&](int j) {
    const double* e = err + (size_t)(j & 1) * M * od;
    const double* de = derr + (size_t)(j & 1) * M * od;
    double s = 0.0, ds = 0.0;
    if (lane < M) {
      for (int q = 0; q < od; ++q) s += e[lane * od + q];
      if (want_d)
        for (int q = 0; q < od; ++q) ds += de[lane * od + q];
      const bool counted = j <= srem[lane];
      s = counted ? s : 0.0;
      ds = counted ? ds : 0.0;
    }
    double ts = 0.0, tds = 0.0;
#pragma unroll
    for (int r = 0; r < M; ++r) {
      ts += __shfl(s, r);
      tds += __shfl(ds, r);
    }
    if (lane == 0) {
      a.part[pbase + j - 1] = ts;
      if (want_d) a.dpart[pbase + j - 1] = tds;
    }
  };
  __syncthreads();
  for (int j = 1; j <= a.kmax; ++j) {
    const T* cur = xb[(j - 1) & 1];
    T* nxt = xb[j & 1];
    double* eb = err + (size_t)(j & 1) * M * od;
    double* deb = derr + (size_t)(j & 1) * M * od;
    for (int nt = w; nt < m.ntile; nt += kLinW) {
      const int col = 16 * nt + (lane & 15);
      const bool ecol = col < od;
      double o[4] = {0.0, 0.0, 0.0, 0.0}, op[4] = {0.0, 0.0, 0.0, 0.0};
      if (ecol) {                                  // (issued ahead of the product: the loads land behind the MFMAs)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int k = j < rr[r] ? j : rr[r];
          o[r] = a.obs[(rb[r] + k) * od + col];
          if (want_d) op[r] = a.obs[(rb[r] + (k > 0 ? k - 1 : 0)) * od + col];
        }
      }
      const typename Acc<T>::type acc = lin_tile<T>(m, cur, xs, nt, lane);
      if (col < nx) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = acc_row<T>(lane >> 4, r);
          const T xn = acc[r];
          nxt[row * xs + col] = xn;
          if (ecol) {
            const double e = (double)xn - o[r];
            eb[row * od + col] = e * e;
            if (want_d) {
              const double dd = (((double)xn - (double)cur[row * xs + col]) - (o[r] - op[r])) * a.inv_std[col];
              deb[row * od + col] = dd * dd;
            }
          }
        }
      }
    }
    if (j < a.kmax) controls(j + 1, nxt);
    if (w == kLinW - 1 && j > 1) reduce(j - 1);
    lds_barrier();
  }
  if (w == kLinW - 1) reduce(a.kmax);
}

// out[m][j] = sum over tiles, in tile order, of part[m][tile][j]
template <typename T>
__global__ void kstep_lin_reduce_kernel(const double* __restrict__ part, double* __restrict__ out, int n_models,
                                        int tiles, int kmax) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_models * kmax) return;
  const int m = i / kmax, j = i - m * kmax;
  double s = 0.0;
  for (int t = 0; t < tiles; ++t) s += part[((size_t)m * tiles + t) * kmax + j];
  out[i] = s;
}

}  // namespace ampc
