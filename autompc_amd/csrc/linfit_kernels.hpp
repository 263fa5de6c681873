// linfit_kernels.hpp -- least-squares fits of ARX and Koopman(lstsq) models in f64 (reference: autompc/sysid/arx.py:62-116,
// koopman.py:105-154), many configurations per call.
//
// linfit_gram_kernel + linfit_gram_reduce_kernel: G = F' [F | Y] of one design, by the shared Gram pass
// (gram_frame.hpp: row splits, MFMA tiles, ordered sum; its determinism contract holds here).  The feature columns
// (the ARX lag gather with index max(t - i, 0) inside the row's own trajectory, arx.py:62-76, or the Koopman basis
// functions applied element-wise, koopman.py:112-122) and the target columns (the next observation, lifted for
// Koopman) are formed from obs / ctrls by a per-column rule (LinfitCol); of the symmetric part F'F only the tiles on
// and above the diagonal are computed (the reduction mirrors them).
//
// linfit_solve_kernel: one workgroup per configuration.  It gathers the configuration's sub-matrix of G by a column
// index list, scales it to unit diagonal (D G D, D = diag(G)^-1/2), and factors it by fit_cholesky (gram_frame.hpp).
// The right-hand sides ride along as extra ROWS of the matrix ([S; Y' D]): the factorisation leaves L^-1 of them
// there, so only the back substitution remains.  The scaled Gram has unit diagonal, so a squared pivot is 1 - R^2 of
// that column against the ones before it.
// status = 1 ("not fitted here") when a diagonal entry or pivot is not positive and finite, a coefficient is not
// finite, or the smallest squared pivot is below n_features * 2^-26 (half the digits of the solution are gone).
#ifndef AMPC_LINFIT_KERNELS_HPP
#define AMPC_LINFIT_KERNELS_HPP
#include <hip/hip_runtime.h>

#include "gram_frame.hpp"

namespace ampc {

constexpr int kLinfitMaxTargets = 256;

// How one column of [F | Y] is formed from the data.
struct LinfitCol {
  int src;      // 0: the constant 1, 1: obs[row][j], 2: ctrls[row][j]
  int lag;      // row = max(t - lag, first row of the trajectory); -1: row = t + 1 (a target column)
  int j;
  int fn;       // index of the basis function (kind, parameter) applied to the value; -1: none
  __host__ __device__ static LinfitCol zero() { return LinfitCol{0, -2, 0, -1}; }     // a padding column
};

struct LinfitGramArgs {
  const double* obs;          // [R][no]
  const double* ctrls;        // [R][nu]
  const int* row_start;       // [R]: first row of the row's trajectory; -1: the row has no successor (no design row)
  const LinfitCol* cols;      // [wp] (padding columns: src 0 with lag -2 -> 0)
  const double* prog;         // [n_fn][2] (kind, parameter): 0 identity, 1 power, 2 sin, 3 cos
  const int* tiles;           // [n_tiles]: ti | tj << 16
  double* part;               // [splits][nfp][wp]
  int R, no, nu, wp, nfp, n_tiles, lds_stride;
};

// o ** p for an integer p >= 0, rounded once (double-double running product, as the device lifts of the closed
// loops: lqr_kernels.hpp, mppi_kernels.hpp)
__device__ inline double linfit_pow(double o, int pw) {
  double h = pw >= 1 ? o : 1.0, l = 0.0;
  for (int k = 1; k < pw; ++k) {
    const double ph = h * o;
    const double pe = fma(h, o, -ph) + l * o;
    h = ph + pe;
    l = pe - (h - ph);
  }
  return h;
}

__device__ inline double linfit_value(const LinfitGramArgs& a, const LinfitCol c, int g, int start) {
  if (c.src == 0) return c.lag == -2 ? 0.0 : 1.0;
  int row = c.lag < 0 ? g + 1 : g - c.lag;
  if (row < start) row = start;
  double v = c.src == 1 ? a.obs[(size_t)row * a.no + c.j] : a.ctrls[(size_t)row * a.nu + c.j];
  if (c.fn >= 0) {
    const int kind = (int)a.prog[2 * c.fn];
    const double par = a.prog[2 * c.fn + 1];
    if (kind == 1) v = linfit_pow(v, (int)par);
    else if (kind == 2) v = sin(par * v);
    else if (kind == 3) v = cos(par * v);
  }
  return v;
}

// grid (splits, tile groups); dynamic LDS: kFitChunk * lds_stride doubles.
__global__ __launch_bounds__(kFitThreads) void linfit_gram_kernel(const LinfitGramArgs a) {
  extern __shared__ __attribute__((aligned(16))) double linfit_lds[];
  // the (at most three) columns a thread forms
  constexpr int kCols = (kFitMaxFeat + kLinfitMaxTargets + 15 + kFitThreads - 1) / kFitThreads;
  gram_tiles<kCols>(linfit_lds, a.cols, a.tiles, a.n_tiles, a.wp, a.nfp, a.lds_stride, a.part, a.R, a.row_start,
                    [&a](const LinfitCol c, int g, int start) { return linfit_value(a, c, g, start); });
}

// G[a][b] = the ordered sum of the partial tile entries.  G is [nfp][wp]; entries with a >= nf or b >= nf + nt are
// not written.
__global__ void linfit_gram_reduce_kernel(const double* __restrict__ part, double* __restrict__ G, int splits, int nf,
                                          int w, int nfp, int wp) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nf * w) return;
  const int ra = i / w, cb = i - ra * w;
  G[(size_t)ra * wp + cb] = gram_split_sum(part, splits, nfp, wp, ra, cb, cb < nf);
}

// One configuration.  Read field by field through a global pointer (uniform loads), as LqrDesc.
struct LinfitSolveDesc {
  int n, nt, tcol, id;        // features, targets, first target column of G, output slot
  const double* g;            // the design's Gram [.][ldg]
  long long ldg;
  long long idx;              // offset (ints) of the column index list [n]
  long long ws;               // workspace offset (doubles): [n + nt][n]
  long long out;              // coefficient offset (doubles): [nt][n]
};

__global__ __launch_bounds__(kFitThreads) void linfit_solve_kernel(const LinfitSolveDesc* __restrict__ descs,
                                                                       const int* __restrict__ order,
                                                                       const int* __restrict__ idxbuf, double* ws,
                                                                       double* __restrict__ coef,
                                                                       int* __restrict__ status,
                                                                       double* __restrict__ min_pivot) {
  __shared__ double P[(kFitMaxFeat + kLinfitMaxTargets) * kFitPs];
  __shared__ double dsc[kFitMaxFeat];      // D
  __shared__ double linv[kFitMaxFeat];     // 1 / L[j][j]
  __shared__ double s_min;
  __shared__ int s_bad;
  constexpr int T = kFitThreads;
  const LinfitSolveDesc* d = descs + order[blockIdx.x];
  const int n = d->n, nt = d->nt, tcol = d->tcol, id = d->id;
  const double* __restrict__ G = d->g;
  const size_t ldg = (size_t)d->ldg;
  const int* __restrict__ idx = idxbuf + d->idx;
  double* M = ws + d->ws;
  double* out = coef + d->out;
  const int rows = n + nt, t = threadIdx.x;
  if (t == 0) { s_bad = 0; s_min = __builtin_inf(); }
  __syncthreads();
  for (int i = t; i < n; i += T) {
    const double g = G[idx[i] * ldg + idx[i]];
    if (!(g > 0.0) || !isfinite(g)) { s_bad = 1; s_min = g; }
    dsc[i] = 1.0 / sqrt(g);
  }
  __syncthreads();
  if (!s_bad) {
    for (int e = t; e < rows * n; e += T) {
      const int r = e / n, c = e - r * n;
      M[e] = r < n ? G[idx[r] * ldg + idx[c]] * dsc[r] * dsc[c] : G[idx[c] * ldg + tcol + (r - n)] * dsc[c];
    }
    __syncthreads();
    fit_cholesky(M, rows, n, P, linv, s_bad, s_min, s_min);
  }
  if (!s_bad) {
    // rows n.. hold y = L^-1 (D g_t); back substitution L' z = y by columns, z_j = y_j / L[j][j]
    for (int j = n - 1; j > 0; --j) {
      const double li = linv[j];
      for (int e = t; e < nt * j; e += T) {
        const int tt = e / j, i = e - tt * j;
        double* y = M + (size_t)(n + tt) * n;
        y[i] = fma(-M[(size_t)j * n + i], y[j] * li, y[i]);
      }
      __syncthreads();
    }
    for (int e = t; e < nt * n; e += T) {
      const int c = e % n;
      const double v = M[(size_t)n * n + e] * linv[c] * dsc[c];
      out[e] = v;
      if (!isfinite(v)) s_bad = 1;
    }
  }
  __syncthreads();
  if (s_bad)
    for (int e = t; e < nt * n; e += T) out[e] = __builtin_nan("");
  if (t == 0) {
    status[id] = (s_bad || s_min < (double)n * 0x1p-26) ? 1 : 0;
    min_pivot[id] = s_min;
  }
}

}  // namespace ampc
#endif
