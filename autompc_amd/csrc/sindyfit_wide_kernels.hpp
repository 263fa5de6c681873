// sindyfit_wide_kernels.hpp -- the thresholded SINDy fit (sindyfit_kernels.hpp) for libraries of up to 2048 features.
// Same algorithm, statistics and status rules; a second pair of kernels because the narrow pair keeps all columns of
// sixteen design rows and five kFitMaxFeat arrays in LDS and updates the trailing matrix on the vector ALU.
//
// Gram pass.  sindyfit_wide_theta_kernel MATERIALISES [Theta | Y] of a run of 512-row splits of a design into device
// scratch, one thread per (column, 32 rows): every feature value is formed exactly once, by sindyfit_value (the
// narrow pass's rule; a row without a successor is dropped by a select, its values are never formed; rows past the
// data are zeros).  sindyfit_wide_gram_kernel is then a plain rank-k pass on v_mfma_f64_16x16x4_f64: one wave owns
// tile row ti and up to kWideAcc tile columns on or right of the diagonal, and per split, in split order, forms the
// split's partial tile in fresh accumulators (one k-ordered chain over the split's 512 rows) and adds it to the
// running sum.  The running sum is G itself: a later launch (the next run of splits of the same design) continues
// from what the earlier one stored, so the sum's bits are those of ((0 + p_0) + p_1) + ... whatever the cut -- there
// is no scratch of partial tiles and no atomics.  The tiles below the diagonal are written as mirrors.
//
// Solve.  sindyfit_wide_solve_kernel: one workgroup of kWideThreads per (configuration, target), no grid-wide
// synchronisation, no waiting on memory, every loop bounded by n or max_iter.  The kept list, keep flags, D, 1 / L_jj
// and the coefficients are dynamic LDS sized by the widest design of the launch.  wide_cholesky is right-looking with
// panels of kWideNb columns: the panel's diagonal block is factored in LDS, every row below it (the right-hand side
// row n included) is solved against that block by the thread that owns the row, staged in LDS, and the trailing matrix
// (global memory, the pair's [n + 1][n] workspace) is updated on v_mfma_f64_16x16x4_f64, the 16 x 16 tiles on and
// below the diagonal only.
#ifndef AMPC_SINDYFIT_WIDE_KERNELS_HPP
#define AMPC_SINDYFIT_WIDE_KERNELS_HPP
#include <hip/hip_runtime.h>

#include "sindyfit_frame.hpp"

namespace ampc {

constexpr int kWideMaxFeat = 2048;
constexpr int kWideThreads = 512, kWideWaves = kWideThreads / 64;
constexpr int kWideNb = 32, kWidePs = kWideNb + 1;     // Cholesky panel width, LDS row stride of its diagonal block
constexpr int kWideTrsmRows = 256;                     // panel rows solved against the diagonal block at a time
constexpr int kWideAcc = 8;                            // tiles (accumulators) per wave of the Gram pass
constexpr int kWideThetaRows = 32;                     // rows per thread of the Theta kernel
constexpr int kWideThetaCols = 256;                    // columns per workgroup of the Theta kernel

// One design of a wide call.  Read field by field through a global pointer (uniform loads).
struct SindyfitWideDesign {
  const SindyfitCol* cols;    // [wp]
  const int* pool;            // [n_pair][2] (variable, exponent >= 1) of the monomial features
  const int* groups;          // [n_groups]: ti | tj0 << 16, tile row and first tile column of a wave's tiles
  double* G;                  // [nfp][wp]
  int nf, w, wp, nfp, n_groups, pad;
};

// A run of row splits of one design: what one z-slice of a Gram launch forms.
struct SindyfitWideItem {
  int design, s0, s1, first;  // splits s0 .. s1 - 1; first: the running sum starts at zero
  long long theta;            // offset (doubles) of its [(s1 - s0) * 512][wp] block in the scratch
};

// grid (column blocks, row blocks of kWideThetaRows, items)
__global__ __launch_bounds__(kWideThetaCols) void sindyfit_wide_theta_kernel(
    const SindyfitGramArgs a, const SindyfitWideDesign* __restrict__ designs, const SindyfitWideItem* __restrict__ items,
    double* __restrict__ theta) {
  const SindyfitWideItem* it = items + blockIdx.z;
  const SindyfitWideDesign* d = designs + it->design;
  const int wp = d->wp, c = (int)blockIdx.x * kWideThetaCols + (int)threadIdx.x;
  const int nrows = (it->s1 - it->s0) * kFitSplitRows, r0 = (int)blockIdx.y * kWideThetaRows;
  if (r0 >= nrows || c >= wp) return;
  const SindyfitCol col = d->cols[c];
  const int* __restrict__ pool = d->pool;
  double* out = theta + it->theta + (size_t)r0 * wp + c;
  const int g0 = it->s0 * kFitSplitRows + r0;
  for (int r = 0; r < kWideThetaRows; ++r) {
    const int g = g0 + r;
    const int start = g < a.R ? a.row_start[g] : -1;
    // a row without a successor is dropped by a SELECT (its values are never formed)
    out[(size_t)r * wp] = start < 0 ? 0.0 : sindyfit_value(a, col, pool, g);
  }
}

// grid (groups / 4 rounded up, items); 256 threads: one wave per group of tiles
__global__ __launch_bounds__(256) void sindyfit_wide_gram_kernel(const SindyfitWideDesign* __restrict__ designs,
                                                                 const SindyfitWideItem* __restrict__ items,
                                                                 const double* __restrict__ theta) {
  const SindyfitWideItem* it = items + blockIdx.y;
  const SindyfitWideDesign* d = designs + it->design;
  const int lane = threadIdx.x & 63;
  const int gid = (int)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  if (gid >= d->n_groups) return;                   // (wave-uniform; the kernel has no barrier)
  const int wp = d->wp, nfp = d->nfp;
  const int word = d->groups[gid], ti = word & 0xffff, tj0 = word >> 16;
  const int nq = wp / 16 - tj0 < kWideAcc ? wp / 16 - tj0 : kWideAcc;
  double* G = d->G;
  const int lr = lane >> 4, lc = lane & 15;
  fit_d4 sum[kWideAcc];
#pragma unroll
  for (int q = 0; q < kWideAcc; ++q) {
    sum[q] = fit_d4{0.0, 0.0, 0.0, 0.0};
    if (!it->first && q < nq) {
#pragma unroll
      for (int r = 0; r < 4; ++r) sum[q][r] = G[(size_t)(16 * ti + lr + 4 * r) * wp + 16 * (tj0 + q) + lc];
    }
  }
  const double* th = theta + it->theta;
  for (int s = it->s0; s < it->s1; ++s, th += (size_t)kFitSplitRows * wp) {
    fit_d4 acc[kWideAcc];
#pragma unroll
    for (int q = 0; q < kWideAcc; ++q) acc[q] = fit_d4{0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < kFitSplitRows; k += 4) {
      const double* rowp = th + (size_t)(k + lr) * wp + lc;
      const double av = rowp[16 * ti];
#pragma unroll
      for (int q = 0; q < kWideAcc; ++q) {
        const double bv = q < nq ? rowp[16 * (tj0 + q)] : 0.0;
        acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[q], 0, 0, 0);
      }
    }
#pragma unroll
    for (int q = 0; q < kWideAcc; ++q)
#pragma unroll
      for (int r = 0; r < 4; ++r) sum[q][r] += acc[q][r];
  }
#pragma unroll
  for (int q = 0; q < kWideAcc; ++q) {
    if (q >= nq) continue;
    const int tj = tj0 + q;
#pragma unroll
    for (int r = 0; r < 4; ++r) {     // f64 16x16x4 result map: column lane & 15, row (lane >> 4) + 4 r
      G[(size_t)(16 * ti + lr + 4 * r) * wp + 16 * tj + lc] = sum[q][r];
      if (tj != ti && 16 * tj < nfp) G[(size_t)(16 * tj + lc) * wp + 16 * ti + lr + 4 * r] = sum[q][r];
    }
  }
}

// Factors the leading n x n block of M ([rows][n], rows = n + 1: the right-hand side rides along as row n) in place,
// all kWideThreads threads together.  Pd: LDS [kWideNb][kWidePs]; Rw: LDS [kWideTrsmRows][kWidePs]; linv takes 1 / L[j][j].  bad / bad_pivot /
// min_pivot as fit_cholesky's (gram_frame.hpp).
__device__ __forceinline__ void wide_cholesky(double* M, int rows, int n, double* Pd, double* Rw, double* linv, int& bad,
                                              double& bad_pivot, double& min_pivot) {
  constexpr int T = kWideThreads, NB = kWideNb, PS = kWidePs;
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int lr = lane >> 4, lc = lane & 15;
  for (int j0 = 0; j0 < n; j0 += NB) {
    const int nbw = n - j0 < NB ? n - j0 : NB;
    // the diagonal block, padded by the identity to NB columns
    for (int e = t; e < NB * NB; e += T) {
      const int r = e / NB, c = e - r * NB;
      Pd[r * PS + c] = (r < nbw && c < nbw) ? M[(size_t)(j0 + r) * n + j0 + c] : (r == c ? 1.0 : 0.0);
    }
    __syncthreads();
    for (int jj = 0; jj < nbw; ++jj) {
      if (t == 0) {
        const double piv = Pd[jj * PS + jj];
        if (!(piv > 0.0) || !isfinite(piv)) { bad = 1; bad_pivot = piv; }
        else {
          if (piv < min_pivot) min_pivot = piv;
          const double l = sqrt(piv);
          Pd[jj * PS + jj] = l;
          linv[j0 + jj] = 1.0 / l;
        }
      }
      __syncthreads();
      if (bad) break;
      const double l = Pd[jj * PS + jj];
      for (int r = jj + 1 + t; r < nbw; r += T) Pd[r * PS + jj] /= l;
      __syncthreads();
      const int cw = nbw - jj - 1;
      for (int e = t; e < cw * cw; e += T) {
        const int r = jj + 1 + e / cw, c = jj + 1 + e % cw;
        if (r >= c) Pd[r * PS + c] = fma(-Pd[r * PS + jj], Pd[c * PS + jj], Pd[r * PS + c]);
      }
      __syncthreads();
    }
    if (bad) break;
    for (int e = t; e < nbw * nbw; e += T) {
      const int r = e / nbw, c = e - r * nbw;
      if (r >= c) M[(size_t)(j0 + r) * n + j0 + c] = Pd[r * PS + c];
    }
    // the rows below the block: row r of the panel is L[r][j0 ..] = M[r][j0 ..] L_d^-T, kWideTrsmRows rows at a
    // time staged in LDS (row stride kWidePs: the threads' rows fall on distinct banks), one thread per row
    const int c1 = j0 + nbw;
    for (int base = c1; base < rows; base += kWideTrsmRows) {
      const int cnt = rows - base < kWideTrsmRows ? rows - base : kWideTrsmRows;
      for (int e = t; e < cnt * nbw; e += T) {
        const int r = e / nbw, c = e - r * nbw;
        Rw[r * PS + c] = M[(size_t)(base + r) * n + j0 + c];
      }
      __syncthreads();
      if (t < cnt) {
        double* row = Rw + t * PS;
        for (int j = 0; j < nbw; ++j) {
          const double* lj = Pd + j * PS;
          double s = row[j];
          for (int q = 0; q < j; ++q) s = fma(-row[q], lj[q], s);
          row[j] = s / lj[j];
        }
      }
      __syncthreads();
      for (int e = t; e < cnt * nbw; e += T) {
        const int r = e / nbw, c = e - r * nbw;
        M[(size_t)(base + r) * n + j0 + c] = Rw[r * PS + c];
      }
      __syncthreads();
    }
    __syncthreads();
    if (c1 >= n) break;
    // trailing update M[r][c] -= sum_q L[r][q] L[c][q] (r >= c >= c1; c1 is a multiple of 16 here), by 16 x 16
    // tiles: a wave takes every kWideWaves-th tile of a tile row and keeps the row's A fragments
    const int T0 = c1 >> 4, TI1 = (rows - 1) >> 4, TJ1 = (n - 1) >> 4;
    for (int I = T0; I <= TI1; ++I) {
      const int ra = 16 * I + lc;
      double af[NB / 4];
#pragma unroll
      for (int ks = 0; ks < NB / 4; ++ks)
        af[ks] = ra < rows ? -M[(size_t)ra * n + j0 + 4 * ks + lr] : 0.0;
      const int jend = I < TJ1 ? I : TJ1;
      for (int J = T0 + wave; J <= jend; J += kWideWaves) {
        const int rb = 16 * J + lc;           // B[k][j] = L[16 J + j][k]
        const int col = 16 * J + lc;
        fit_d4 acc;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * I + lr + 4 * r;
          acc[r] = (row < rows && col < n) ? M[(size_t)row * n + col] : 0.0;
        }
#pragma unroll
        for (int ks = 0; ks < NB / 4; ++ks) {
          const double bv = rb < n ? M[(size_t)rb * n + j0 + 4 * ks + lr] : 0.0;
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(af[ks], bv, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * I + lr + 4 * r;
          if (row < rows && col < n) M[(size_t)row * n + col] = acc[r];
        }
      }
    }
    __syncthreads();
  }
}

// Dynamic LDS of the solve kernel for designs of at most maxn features (bytes).
__host__ __device__ constexpr size_t wide_solve_lds(int maxn) {
  return (size_t)(kWideNb + kWideTrsmRows) * kWidePs * 8 + (size_t)maxn * (3 * 8 + 2 * 4);
}

// One workgroup per pair of the launch (descs[order[first + blockIdx.x]]); ws: the wave's workspace.
__global__ __launch_bounds__(kWideThreads) void sindyfit_wide_solve_kernel(
    const SindyfitSolveDesc* __restrict__ descs, const int* __restrict__ order, int first, int maxn, double* ws,
    double* __restrict__ coef, int* __restrict__ bad, double* __restrict__ min_pivot, double* __restrict__ min_margin,
    int* __restrict__ iters, const double alpha, const int max_iter) {
  extern __shared__ __attribute__((aligned(16))) double wide_lds[];
  double* Pd = wide_lds;                              // [kWideNb][kWidePs]
  double* Rw = Pd + kWideNb * kWidePs;                // [kWideTrsmRows][kWidePs]
  double* dsc = Rw + kWideTrsmRows * kWidePs;         // D; later the margins
  double* linv = dsc + maxn;                          // 1 / L[j][j]
  double* cf = linv + maxn;                           // coefficients of the last solve, by feature
  int* kl = (int*)(cf + maxn);                        // kept features, in order
  int* keep = kl + maxn;
  __shared__ double s_min, s_solve_min, s_margin;
  __shared__ int s_bad, s_nk, s_drop, s_iters;
  constexpr int T = kWideThreads;
  const SindyfitSolveDesc* d = descs + order[first + blockIdx.x];
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
    // gather: a wave per row, lanes along the columns
    for (int r = t >> 6; r < rows; r += T / 64) {
      double* mr = M + (size_t)r * n;
      if (r < n) {
        const double* gr = G + kl[r] * ldg;
        const double dr = dsc[r];
        for (int c = t & 63; c < n; c += 64) mr[c] = (gr[kl[c]] + (r == c ? alpha : 0.0)) * dr * dsc[c];
      } else {
        for (int c = t & 63; c < n; c += 64) mr[c] = G[kl[c] * ldg + tcol] * dsc[c];
      }
    }
    __syncthreads();
    wide_cholesky(M, rows, n, Pd, Rw, linv, s_bad, s_min, s_solve_min);
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
