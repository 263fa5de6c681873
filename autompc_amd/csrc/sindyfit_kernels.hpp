// sindyfit_kernels.hpp -- sequentially-thresholded least-squares (STLSQ) fits of SINDy models in f64 (what
// sysid/sindy.py SINDy.train does on the host), many configurations per call.
//
// sindyfit_gram_kernel + sindyfit_gram_reduce_kernel: G = Theta' [Theta | Y_discrete | Y_continuous] of EVERY design
// (feature library) of the call in one launch of the shared Gram pass (gram_frame.hpp: row splits, MFMA tiles, ordered
// sum; its determinism contract holds here): the design is a grid dimension.  A design's feature columns are the
// library's functions of [obs[t], ctrls[t]] (the seven kinds of sindy_kernels.hpp, evaluated by sindy_feature /
// sindy_ipow as the prediction kernels do), its target columns the next observation (discrete) and / or row t of an
// uploaded [R][nx] array (continuous: np.gradient of the observations or the caller's xdot); only the target sets a
// configuration of the design asks for are formed.  The per-column rule is SindyfitCol; of Theta'Theta only the tiles
// on and above the diagonal are computed (the reduction mirrors them).
//
// sindyfit_solve_kernel: one workgroup per (configuration, target).  A configuration is (design, time mode,
// threshold); alpha and max_iter belong to the call.  With keep = all features, every iteration gathers
// G[keep, keep] + alpha I and G[keep, target], scales to unit diagonal (D = diag(G + alpha I)^-1/2), factors by
// fit_cholesky (gram_frame.hpp; the right-hand side carried as an extra row), back-substitutes, and drops the kept
// features with |coef| < threshold; it stops when nothing is dropped, nothing is kept or max_iter solves were made.  The result is where(keep, coef, 0)
// of the last solve, as SINDy.train leaves it.
// Per pair: bad = 1 when, in any solve, a diagonal entry or pivot is not positive and finite, a coefficient is not
// finite, or the smallest squared pivot is below n_kept * 2^-26; the smallest squared pivot; the smallest threshold
// margin | |coef| - threshold | / threshold over all solves and kept features; the number of solves.  The host folds
// the pairs of a configuration in target order (status 1: bad, 2: margin below 2^-20).
#ifndef AMPC_SINDYFIT_KERNELS_HPP
#define AMPC_SINDYFIT_KERNELS_HPP
#include <hip/hip_runtime.h>

#include "sindyfit_frame.hpp"

namespace ampc {

// columns of a design: features + both target sets, padded to a tile; two per thread
constexpr int kSindyfitMaxCols = (kFitMaxFeat + 2 * kSindyfitMaxState + 15) / 16 * 16;
constexpr int kSindyfitColsPerThread = (kSindyfitMaxCols + kFitThreads - 1) / kFitThreads;



// One design.  Read field by field through a global pointer (uniform loads), as LinfitSolveDesc.
struct SindyfitDesign {
  const SindyfitCol* cols;    // [wp]
  const int* pool;            // [n_pair][2] (variable, exponent >= 1) of the monomial features
  const int* tiles;           // [n_tiles]: ti | tj << 16
  double* part;               // [splits][nfp][wp]
  double* G;                  // [nfp][wp]
  int nf, w, wp, nfp, n_tiles, lds_stride;
};




// grid (splits, tile groups, designs); dynamic LDS: kFitChunk * (largest lds_stride of the call) doubles.
__global__ __launch_bounds__(kFitThreads) void sindyfit_gram_kernel(const SindyfitGramArgs a) {
  extern __shared__ __attribute__((aligned(16))) double sindyfit_lds[];
  const SindyfitDesign* d = a.designs + blockIdx.z;
  const int n_tiles = d->n_tiles;
  if ((int)blockIdx.y * 4 * kFitAcc >= n_tiles) return;      // (uniform: a narrower design has fewer groups)
  const int wp = d->wp, nfp = d->nfp, stride = d->lds_stride;
  const SindyfitCol* __restrict__ cols = d->cols;
  const int* __restrict__ pool = d->pool;
  const int* __restrict__ tiles = d->tiles;
  gram_tiles<kSindyfitColsPerThread>(
      sindyfit_lds, cols, tiles, n_tiles, wp, nfp, stride, d->part, a.R, a.row_start,
      [&a, pool](const SindyfitCol c, int g, int) { return sindyfit_value(a, c, pool, g); });
}

// grid (blocks, designs): G[a][b] = the ordered sum of the partial tile entries.  Entries with a >= nf or b >= w are
// not written.
__global__ void sindyfit_gram_reduce_kernel(const SindyfitDesign* __restrict__ designs, int splits) {
  const SindyfitDesign* d = designs + blockIdx.y;
  const int nf = d->nf, w = d->w, wp = d->wp, nfp = d->nfp;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nf * w) return;
  const double* __restrict__ part = d->part;
  const int ra = i / w, cb = i - ra * w;
  d->G[(size_t)ra * wp + cb] = gram_split_sum(part, splits, nfp, wp, ra, cb, cb < nf);
}


__global__ __launch_bounds__(kFitThreads) void sindyfit_solve_kernel(
    const SindyfitSolveDesc* __restrict__ descs, const int* __restrict__ order, double* ws, double* __restrict__ coef,
    int* __restrict__ bad, double* __restrict__ min_pivot, double* __restrict__ min_margin, int* __restrict__ iters,
    const double alpha, const int max_iter) {
  __shared__ double P[(kFitMaxFeat + 1) * kFitPs];
  __shared__ double dsc[kFitMaxFeat];      // D
  __shared__ double linv[kFitMaxFeat];     // 1 / L[j][j]
  __shared__ double cf[kFitMaxFeat];       // coefficients of the last solve, by feature
  __shared__ int kl[kFitMaxFeat];          // kept features, in order
  __shared__ int keep[kFitMaxFeat];
  __shared__ double s_min, s_solve_min, s_margin;
  __shared__ int s_bad, s_nk, s_drop, s_iters;
  constexpr int T = kFitThreads;
  const SindyfitSolveDesc* d = descs + order[blockIdx.x];
  const int nf = d->n, tcol = d->tcol, id = d->id;
  const double* __restrict__ G = d->g;
  const size_t ldg = (size_t)d->ldg;
  double* M = ws + d->ws;
  double* out = coef + d->out;
  const double thr = d->threshold;
  const int t = threadIdx.x;
  for (int i = t; i < nf; i += T) { keep[i] = 1; cf[i] = 0.0; }
  if (t == 0) { s_bad = 0; s_min = __builtin_inf(); s_margin = __builtin_inf(); s_iters = 0; }
  __syncthreads();
  for (int it = 0; it < max_iter; ++it) {
    if (t == 0) {
      int nk = 0;
      for (int i = 0; i < nf; ++i)
        if (keep[i]) kl[nk++] = i;
      s_nk = nk; s_drop = 0; s_solve_min = __builtin_inf();
    }
    __syncthreads();
    const int n = s_nk, rows = n + 1;
    if (n == 0) break;
    for (int i = t; i < n; i += T) {
      const double g = G[kl[i] * ldg + kl[i]] + alpha;
      if (!(g > 0.0) || !isfinite(g)) { s_bad = 1; s_min = g; }
      dsc[i] = 1.0 / sqrt(g);
    }
    __syncthreads();
    if (s_bad) break;
    for (int e = t; e < rows * n; e += T) {
      const int r = e / n, c = e - r * n;
      M[e] = r < n ? (G[kl[r] * ldg + kl[c]] + (r == c ? alpha : 0.0)) * dsc[r] * dsc[c]
                   : G[kl[c] * ldg + tcol] * dsc[c];
    }
    __syncthreads();
    fit_cholesky(M, rows, n, P, linv, s_bad, s_min, s_solve_min);
    if (s_bad) break;
    // row n holds y = L^-1 (D g_t); back substitution L' z = y by columns, z_j = y_j / L[j][j]
    double* y = M + (size_t)n * n;
    for (int j = n - 1; j > 0; --j) {
      const double yj = y[j] * linv[j];
      for (int i = t; i < j; i += T) y[i] = fma(-M[(size_t)j * n + i], yj, y[i]);
      __syncthreads();
    }
    for (int i = t; i < nf; i += T) cf[i] = 0.0;
    __syncthreads();
    if (t == 0) {
      if (s_solve_min < s_min) s_min = s_solve_min;
      if (s_solve_min < (double)n * 0x1p-26) s_bad = 1;
      s_iters = it + 1;
    }
    // the kept features' coefficients, their threshold margins, and who is dropped (one thread per feature writes
    // its own entries; the minimum is folded by thread 0 in feature order)
    for (int c = t; c < n; c += T) {
      const double v = y[c] * linv[c] * dsc[c];
      cf[kl[c]] = v;
      if (!isfinite(v)) s_bad = 1;
      dsc[c] = thr > 0.0 ? fabs(fabs(v) - thr) / thr : __builtin_inf();     // (dsc is free again: the margins)
      if (fabs(v) < thr) { keep[kl[c]] = 0; s_drop = 1; }
    }
    __syncthreads();
    if (t == 0)
      for (int c = 0; c < n; ++c)
        if (dsc[c] < s_margin) s_margin = dsc[c];
    __syncthreads();
    const bool stop = s_bad || !s_drop;
    __syncthreads();                    // (thread 0 resets s_drop at the top of the next iteration)
    if (stop) break;
  }
  __syncthreads();
  for (int i = t; i < nf; i += T) out[i] = s_bad ? __builtin_nan("") : (keep[i] ? cf[i] : 0.0);
  if (t == 0) {
    bad[id] = s_bad;
    min_pivot[id] = s_min;
    min_margin[id] = s_margin;
    iters[id] = s_iters;
  }
}

}  // namespace ampc
#endif
