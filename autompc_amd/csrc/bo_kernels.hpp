// bo_kernels.hpp -- the Bayesian-optimisation proposal (tuning/proposer.py: the algorithm's steps 3-5) on the device:
// a Matern-5/2 GP fitted for every row of a hyperparameter table, the posterior of the chosen row over a pool of
// candidate points, and greedy expected-improvement picks with the "believer" update.  f64 only.
//
// Kernel matrix.  bo_kmat_kernel, grid (elements / 256, G): row g's [n + 1][n] block gets k(X, X) + noise_g I (the
// whole square: the factorisation's trailing update reads the upper halves of its diagonal tiles) and z as row n.
//
// Factor.  bo_factor_kernel, one workgroup of kWideThreads per hyperparameter row: wide_cholesky
// (sindyfit_wide_kernels.hpp: 32-column panels, trailing update on v_mfma_f64_16x16x4_f64) with z riding along as row
// n, so t = L^-1 z is row n afterwards.  lml = -(sum_i t_i^2 / 2 + log L_ii): every thread sums its stride of i in
// order, thread 0 adds the kWideThreads partial sums in order.  A pivot that is not positive and finite: status 1,
// lml = -inf.
//
// Posterior.  bo_posterior_kernel, one workgroup of four waves per 64 pool points, a wave owns 16 of them from start
// to end (no wave ever reads what another wrote): V = L^-1 k(X, P) left-looking by panels of 32 rows.  A panel's
// [32][16] block starts as the kernel values (formed in the MFMA accumulator layout), takes -L[panel][0 .. i0) V[0 ..
// i0) on v_mfma_f64_16x16x4_f64 (B fragments are the wave's own earlier V rows), and is solved against the panel's
// 32 x 32 diagonal block of L (LDS) by sixteen lanes, one pool point each, row by row in order; the same lanes carry
// mu += v t and sum v^2.  V is [n + q][Mp] (Mp = m rounded up to 64; the padding columns repeat the last pool point
// and are never reported): the q rows behind n are the picks' believer rows.
//
// Picks.  Per pick bo_argmax_kernel (one workgroup: every thread scans its stride in ascending order keeping its two
// largest EI, a fixed tree joins them, lowest index on ties) and bo_append_kernel (a thread per pool point: c = k(p,
// p_j) - sum_i V[i][m] V[i][j] over the n + t rows in order, the new row, sigma^2 and EI).  No atomics anywhere: the
// same inputs give the same bits.
#ifndef AMPC_BO_KERNELS_HPP
#define AMPC_BO_KERNELS_HPP
#include <hip/hip_runtime.h>

// wide_cholesky's header also defines the wide SINDy fit's three kernels, which launch_sindyfit_wide.cpp already gives
// the library: this translation unit compiles its own copies under other names (never launched), so that it links.
#define sindyfit_wide_theta_kernel bo_unused_sindyfit_wide_theta_kernel
#define sindyfit_wide_gram_kernel bo_unused_sindyfit_wide_gram_kernel
#define sindyfit_wide_solve_kernel bo_unused_sindyfit_wide_solve_kernel
#include "sindyfit_wide_kernels.hpp"
#undef sindyfit_wide_theta_kernel
#undef sindyfit_wide_gram_kernel
#undef sindyfit_wide_solve_kernel

namespace ampc {

constexpr int kBoMaxN = 2048, kBoMaxD = 64, kBoMaxG = 64, kBoMaxM = 65536, kBoMaxQ = 256;
constexpr double kBoVarFloor = 1e-12;               // VAR_FLOOR of tuning/proposer.py
constexpr int kBoPoolBlock = 64, kBoPostThreads = 256, kBoPostWaves = 4;
constexpr int kBoSs = 17;                           // LDS row stride of a wave's [32][16] panel block
constexpr int kBoArgThreads = 1024;

static_assert(kBoMaxN <= kWideMaxFeat, "the factorisation is wide_cholesky's");

// k(a, b) = (1 + s + s^2 / 3) exp(-s), s = sqrt(5) |(a - b) o w|, the squares summed over the dimensions in order
__device__ __forceinline__ double bo_matern(const double* a, const double* b, const double* w, int d) {
  double s2 = 0.0;
  for (int k = 0; k < d; ++k) {
    const double t = (a[k] - b[k]) * w[k];
    s2 = fma(t, t, s2);
  }
  const double s = sqrt(5.0) * sqrt(s2);
  return (1.0 + s + s * s / 3.0) * exp(-s);
}

// EI for minimisation against zmin: sd (u Phi(u) + phi(u)), u = (zmin - mu) / sd, Phi(u) = erfc(-u / sqrt 2) / 2
__device__ __forceinline__ double bo_ei(double mu, double var, double zmin) {
  const double sd = sqrt(var), u = (zmin - mu) / sd;
  const double Phi = 0.5 * erfc(-u * 0.70710678118654752440);
  const double phi = 0.39894228040143267794 * exp(-0.5 * u * u);
  return sd * (u * Phi + phi);
}

// grid ((n + 1) n / 256 rounded up, G)
__global__ __launch_bounds__(256) void bo_kmat_kernel(const double* __restrict__ X, const double* __restrict__ z,
                                                      const double* __restrict__ hw, const double* __restrict__ hnoise,
                                                      int n, int d, double* __restrict__ Kall) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)(n + 1) * n) return;
  const int g = blockIdx.y, r = (int)(e / n), c = (int)(e - (long long)r * n);
  double* M = Kall + (size_t)g * (n + 1) * n;
  double v;
  if (r == n) v = z[c];
  else v = bo_matern(X + (size_t)r * d, X + (size_t)c * d, hw + (size_t)g * d, d) + (r == c ? hnoise[g] : 0.0);
  M[e] = v;
}

// Dynamic LDS of the factor kernel (bytes): wide_cholesky's two blocks, 1 / L_jj, the partial sums.
__host__ __device__ constexpr size_t bo_factor_lds(int n) {
  return (size_t)(kWideNb + kWideTrsmRows) * kWidePs * 8 + (size_t)n * 8 + (size_t)kWideThreads * 8;
}

// grid (G)
__global__ __launch_bounds__(kWideThreads) void bo_factor_kernel(double* Kall, int n, double* __restrict__ lml,
                                                                 int* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) double bo_lds[];
  double* Pd = bo_lds;                                // [kWideNb][kWidePs]
  double* Rw = Pd + kWideNb * kWidePs;                // [kWideTrsmRows][kWidePs]
  double* linv = Rw + kWideTrsmRows * kWidePs;        // [n]
  double* part = linv + n;                            // [kWideThreads]
  __shared__ double s_bad_pivot, s_min;
  __shared__ int s_bad;
  const int t = threadIdx.x, g = blockIdx.x;
  double* M = Kall + (size_t)g * (n + 1) * n;
  if (t == 0) { s_bad = 0; s_bad_pivot = 0.0; s_min = __builtin_inf(); }
  __syncthreads();
  wide_cholesky(M, n + 1, n, Pd, Rw, linv, s_bad, s_bad_pivot, s_min);
  __syncthreads();
  if (s_bad) {
    if (t == 0) { status[g] = 1; lml[g] = -__builtin_inf(); }
    return;
  }
  const double* tv = M + (size_t)n * n;
  double p = 0.0;
  for (int i = t; i < n; i += kWideThreads) p += 0.5 * tv[i] * tv[i] + log(M[(size_t)i * n + i]);
  part[t] = p;
  __syncthreads();
  if (t == 0) {
    double s = 0.0;
    for (int i = 0; i < kWideThreads; ++i) s += part[i];
    lml[g] = -s;
    status[g] = 0;
  }
}

// Dynamic LDS of the posterior kernel (bytes).
__host__ __device__ constexpr size_t bo_posterior_lds(int d) {
  return ((size_t)kBoPoolBlock * d + (size_t)kWideNb * d + (size_t)d + (size_t)kWideNb * kWidePs +
          (size_t)kBoPostWaves * kWideNb * kBoSs + (size_t)kWideNb) * 8;
}

// grid (Mp / 64).  L: the chosen row's factored [n + 1][n] block (row n = t).  V: [n + q][Mp], rows 0 .. n - 1 written.
__global__ __launch_bounds__(kBoPostThreads) void bo_posterior_kernel(
    const double* __restrict__ L, const double* __restrict__ X, const double* __restrict__ w,
    const double* __restrict__ pool, int n, int d, int m, int Mp, double zmin, double* V, double* __restrict__ mu,
    double* __restrict__ var0, double* __restrict__ var, double* __restrict__ ei) {
  constexpr int NB = kWideNb, PS = kWidePs, SS = kBoSs;
  extern __shared__ __attribute__((aligned(16))) double bo_lds[];
  double* Pl = bo_lds;                                // [64][d] the block's pool points
  double* Xl = Pl + kBoPoolBlock * d;                 // [NB][d] the panel's rows of X
  double* wl = Xl + NB * d;                           // [d]
  double* Ld = wl + d;                                // [NB][PS] the panel's diagonal block, padded by the identity
  double* Sall = Ld + NB * PS;                        // [waves][NB][SS]
  double* tl = Sall + kBoPostWaves * NB * SS;         // [NB] the panel's entries of t
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int lr = lane >> 4, lc = lane & 15;
  const int m0 = (int)blockIdx.x * kBoPoolBlock;
  const int col = m0 + 16 * wave + lc;                // this lane's pool point (column of V); < Mp
  double* S = Sall + wave * NB * SS;
  for (int e = t; e < kBoPoolBlock * d; e += kBoPostThreads) {
    const int p = e / d, k = e - p * d;
    const int src = m0 + p < m ? m0 + p : m - 1;
    Pl[e] = pool[(size_t)src * d + k];
  }
  for (int k = t; k < d; k += kBoPostThreads) wl[k] = w[k];
  double mu_acc = 0.0, ss = 0.0;
  for (int i0 = 0; i0 < n; i0 += NB) {
    const int nbw = n - i0 < NB ? n - i0 : NB;
    __syncthreads();                                  // the previous panel's LDS is free (and Pl, wl are staged)
    for (int e = t; e < NB * d; e += kBoPostThreads) {
      const int r = e / d, k = e - r * d;
      Xl[e] = r < nbw ? X[(size_t)(i0 + r) * d + k] : 0.0;
    }
    for (int e = t; e < NB * NB; e += kBoPostThreads) {
      const int r = e / NB, c = e - r * NB;
      Ld[r * PS + c] = (r < nbw && c <= r) ? L[(size_t)(i0 + r) * n + i0 + c] : (r == c ? 1.0 : 0.0);
    }
    if (t < NB) tl[t] = t < nbw ? L[(size_t)n * n + i0 + t] : 0.0;
    __syncthreads();
    fit_d4 acc[2];
#pragma unroll
    for (int I = 0; I < 2; ++I)
#pragma unroll
      for (int r = 0; r < 4; ++r) {                   // f64 16x16x4 result map: column lane & 15, row (lane >> 4) + 4 r
        const int row = 16 * I + lr + 4 * r;
        acc[I][r] = row < nbw ? bo_matern(Xl + row * d, Pl + (16 * wave + lc) * d, wl, d) : 0.0;
      }
    const int ra0 = i0 + lc, ra1 = i0 + 16 + lc;
    const double* la0 = L + (size_t)(ra0 < n ? ra0 : 0) * n + lr;
    const double* la1 = L + (size_t)(ra1 < n ? ra1 : 0) * n + lr;
    const double* vb = V + (size_t)lr * Mp + col;
    for (int q = 0; q < i0; q += 4) {
      const double bv = vb[(size_t)q * Mp];
      const double a0 = ra0 < n ? -la0[q] : 0.0, a1 = ra1 < n ? -la1[q] : 0.0;
      acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, bv, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, bv, acc[1], 0, 0, 0);
    }
#pragma unroll
    for (int I = 0; I < 2; ++I)
#pragma unroll
      for (int r = 0; r < 4; ++r) S[(16 * I + lr + 4 * r) * SS + lc] = acc[I][r];
    __syncthreads();
    if (lane < 16) {                                  // one pool point per lane, the panel's rows in order
      for (int j = 0; j < nbw; ++j) {
        const double* lj = Ld + j * PS;
        double s = S[j * SS + lc];
        for (int p = 0; p < j; ++p) s = fma(-lj[p], S[p * SS + lc], s);
        const double v = s / lj[j];
        S[j * SS + lc] = v;
        mu_acc = fma(v, tl[j], mu_acc);
        ss = fma(v, v, ss);
      }
    }
    __syncthreads();
#pragma unroll
    for (int I = 0; I < 2; ++I)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * I + lr + 4 * r;
        if (row < nbw) V[(size_t)(i0 + row) * Mp + col] = S[row * SS + lc];
      }
    __threadfence_block();                            // the wave reads these rows back as B fragments
  }
  if (lane < 16 && col < m) {
    const double v = fmax(1.0 - ss, kBoVarFloor);
    mu[col] = mu_acc;
    var0[col] = v;
    var[col] = v;
    ei[col] = bo_ei(mu_acc, v, zmin);
  }
}

// The better of two (EI, index) candidates: larger EI, lower index on ties; index -1 is "none".
__device__ __forceinline__ bool bo_better(double ea, int ia, double eb, int ib) {
  if (ib < 0) return true;
  if (ia < 0) return false;
  return ea > eb || (ea == eb && ia < ib);
}

// grid (1).  Pick `step`: the unpicked pool point of largest EI (NaN counts as -inf), its EI and its margin over the
// second largest; marks it picked.
__global__ __launch_bounds__(kBoArgThreads) void bo_argmax_kernel(const double* __restrict__ ei, int* __restrict__ picked,
                                                                  int m, int step, int* __restrict__ picks,
                                                                  double* __restrict__ pick_ei,
                                                                  double* __restrict__ pick_margin) {
  __shared__ double s_e1[kBoArgThreads], s_e2[kBoArgThreads];
  __shared__ int s_i1[kBoArgThreads], s_i2[kBoArgThreads];
  const int t = threadIdx.x;
  double e1 = -__builtin_inf(), e2 = -__builtin_inf();
  int i1 = -1, i2 = -1;
  for (int j = t; j < m; j += kBoArgThreads) {
    if (picked[j]) continue;
    double e = ei[j];
    if (!(e == e)) e = -__builtin_inf();
    if (bo_better(e, j, e1, i1)) { e2 = e1; i2 = i1; e1 = e; i1 = j; }
    else if (bo_better(e, j, e2, i2)) { e2 = e; i2 = j; }
  }
  s_e1[t] = e1; s_i1[t] = i1; s_e2[t] = e2; s_i2[t] = i2;
  __syncthreads();
  for (int h = kBoArgThreads / 2; h >= 1; h >>= 1) {
    if (t < h) {
      const double a1 = s_e1[t], a2 = s_e2[t], b1 = s_e1[t + h], b2 = s_e2[t + h];
      const int ia1 = s_i1[t], ia2 = s_i2[t], ib1 = s_i1[t + h], ib2 = s_i2[t + h];
      if (bo_better(a1, ia1, b1, ib1)) {              // a1 first; second: the better of a2, b1
        if (bo_better(b1, ib1, a2, ia2)) { s_e2[t] = b1; s_i2[t] = ib1; }
      } else {                                        // b1 first; second: the better of a1, b2
        s_e1[t] = b1; s_i1[t] = ib1;
        if (bo_better(a1, ia1, b2, ib2)) { s_e2[t] = a1; s_i2[t] = ia1; }
        else { s_e2[t] = b2; s_i2[t] = ib2; }
      }
    }
    __syncthreads();
  }
  if (t == 0) {
    const int j = s_i1[0] < 0 ? 0 : s_i1[0];          // (m >= q: an unpicked point always exists)
    const double best = s_e1[0], second = s_i2[0] < 0 ? 0.0 : s_e2[0];
    picks[step] = j;
    pick_ei[step] = best;
    pick_margin[step] = best > 0.0 ? (best - second) / best : 0.0;
    picked[j] = 1;
  }
}

// grid (m / 256 rounded up).  The believer row of pick `step` (V row nrows = n + step), sigma^2 and EI of every point.
__global__ __launch_bounds__(256) void bo_append_kernel(double* V, int Mp, int nrows, const int* __restrict__ picks,
                                                        int step, const double* __restrict__ pool,
                                                        const double* __restrict__ w, int d, double noise, double zmin,
                                                        int m, const double* __restrict__ mu, double* __restrict__ var,
                                                        double* __restrict__ ei) {
  const int c = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (c >= m) return;
  const int j = picks[step];
  double am = 0.0, aj = 0.0;
  const double* vm = V + c;
  const double* vj = V + j;
  for (int i = 0; i < nrows; ++i) {
    const double b = vj[(size_t)i * Mp];
    am = fma(vm[(size_t)i * Mp], b, am);
    aj = fma(b, b, aj);
  }
  const double cm = bo_matern(pool + (size_t)c * d, pool + (size_t)j * d, w, d) - am;
  const double cj = 1.0 - aj;                         // k(p_j, p_j) = 1
  const double r = cm / sqrt(fmax(cj + noise, kBoVarFloor));
  V[(size_t)nrows * Mp + c] = r;
  const double v = fmax(var[c] - r * r, kBoVarFloor);
  var[c] = v;
  ei[c] = bo_ei(mu[c], v, zmin);
}

}  // namespace ampc
#endif
