// linfit_kernels.hpp -- least-squares fits of ARX and Koopman(lstsq) models in f64 (reference: autompc/sysid/arx.py:62-116,
// koopman.py:105-154), many configurations per call.
//
// linfit_gram_kernel + linfit_gram_reduce_kernel: G = F' [F | Y] of one design.  A design row is one data row t of a
// trajectory that has a successor; its feature columns (the ARX lag gather with index max(t - i, 0) inside the row's
// own trajectory, arx.py:62-76, or the Koopman basis functions applied element-wise, koopman.py:112-122) and its
// target columns (the next observation, lifted for Koopman) are formed ON THE FLY from obs / ctrls by a per-column
// rule (LinfitCol), sixteen rows at a time into LDS: the wide design matrix never exists in HBM.  The Gram is
// accumulated on v_mfma_f64_16x16x4_f64, one accumulator per 16 x 16 tile; of the symmetric part F'F only the tiles
// on and above the diagonal are computed (the reduction mirrors them).
//
// Determinism.  Rows are split over workgroups by ROW INDEX only (kLinfitSplitRows consecutive data rows each,
// whatever the design's width); rows that are no design rows contribute exact zeros.  An entry's partial sum is one
// MFMA accumulator's k-ordered chain over the split's rows, the partials are summed over splits in order by
// linfit_gram_reduce_kernel.  No atomics: G[a][b] of two given columns has the same bits whatever other columns
// the design holds, and from run to run.
//
// linfit_solve_kernel: one workgroup per configuration.  It gathers the configuration's sub-matrix of G by a column
// index list, scales it to unit diagonal (D G D, D = diag(G)^-1/2), and factors it by a right-looking blocked
// Cholesky: a panel of kLinfitNb columns is factored in LDS, the trailing matrix (global memory, L2-resident: at
// most 528 x 272 doubles) is updated from the panel.  The right-hand sides ride along as extra ROWS of the matrix
// ([S; Y' D]): the factorisation leaves L^-1 of them there, so only the back substitution remains.  The scaled Gram
// has unit diagonal, so a squared pivot is 1 - R^2 of that column against the ones before it.
// status = 1 ("not fitted here") when a diagonal entry or pivot is not positive and finite, a coefficient is not
// finite, or the smallest squared pivot is below n_features * 2^-26 (half the digits of the solution are gone).
#ifndef AMPC_LINFIT_KERNELS_HPP
#define AMPC_LINFIT_KERNELS_HPP
#include <hip/hip_runtime.h>

namespace ampc {

constexpr int kLinfitThreads = 256;
constexpr int kLinfitSplitRows = 512;     // data rows per workgroup of the Gram pass (a constant: see Determinism)
constexpr int kLinfitChunk = 16;          // design rows formed in LDS at a time
constexpr int kLinfitAcc = 8;             // tiles (accumulators) per wave
constexpr int kLinfitMaxFeat = 272;       // 256 states + 16 controls
constexpr int kLinfitMaxTargets = 256;
constexpr int kLinfitNb = 8, kLinfitPs = kLinfitNb + 1;   // Cholesky panel width, LDS row stride of the panel

typedef double linfit_d4 __attribute__((ext_vector_type(4)));

// How one column of [F | Y] is formed from the data.
struct LinfitCol {
  int src;      // 0: the constant 1, 1: obs[row][j], 2: ctrls[row][j]
  int lag;      // row = max(t - lag, first row of the trajectory); -1: row = t + 1 (a target column)
  int j;
  int fn;       // index of the basis function (kind, parameter) applied to the value; -1: none
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

// grid (splits, tile groups): workgroup (s, q) accumulates tiles 32 q .. 32 q + 31 over data rows
// kLinfitSplitRows s ..; dynamic LDS: kLinfitChunk * lds_stride doubles.
__global__ __launch_bounds__(kLinfitThreads) void linfit_gram_kernel(const LinfitGramArgs a) {
  extern __shared__ __attribute__((aligned(16))) double linfit_lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int stride = a.lds_stride;
  int ti[kLinfitAcc], tj[kLinfitAcc];
  linfit_d4 acc[kLinfitAcc];
#pragma unroll
  for (int q = 0; q < kLinfitAcc; ++q) {
    const int id = ((int)blockIdx.y * 4 + wave) * kLinfitAcc + q;
    const int w = id < a.n_tiles ? a.tiles[id] : -1;
    ti[q] = w < 0 ? -1 : (w & 0xffff);
    tj[q] = w < 0 ? -1 : (w >> 16);
    acc[q] = linfit_d4{0.0, 0.0, 0.0, 0.0};
  }
  // the (at most three) columns this thread forms
  constexpr int kCols = (kLinfitMaxFeat + kLinfitMaxTargets + 15 + kLinfitThreads - 1) / kLinfitThreads;
  LinfitCol col[kCols];
#pragma unroll
  for (int m = 0; m < kCols; ++m) {
    const int c = tid + m * kLinfitThreads;
    col[m] = c < a.wp ? a.cols[c] : LinfitCol{0, -2, 0, -1};
  }
  const int row0 = (int)blockIdx.x * kLinfitSplitRows;
  const int rend = row0 + kLinfitSplitRows < a.R ? row0 + kLinfitSplitRows : a.R;
  for (int c0 = row0; c0 < rend; c0 += kLinfitChunk) {
#pragma unroll
    for (int m = 0; m < kCols; ++m) {
      const int c = tid + m * kLinfitThreads;
      if (c >= a.wp) continue;
      for (int r = 0; r < kLinfitChunk; ++r) {
        const int g = c0 + r;
        const int start = g < rend ? a.row_start[g] : -1;
        // a row without a successor is dropped by a SELECT (its values are never formed)
        linfit_lds[r * stride + c] = start < 0 ? 0.0 : linfit_value(a, col[m], g, start);
      }
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < kLinfitChunk / 4; ++ks) {
      const double* rowp = linfit_lds + (4 * ks + (lane >> 4)) * stride + (lane & 15);
#pragma unroll
      for (int q = 0; q < kLinfitAcc; ++q)
        if (ti[q] >= 0)
          acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(rowp[16 * ti[q]], rowp[16 * tj[q]], acc[q], 0, 0, 0);
    }
    __syncthreads();
  }
  double* part = a.part + (size_t)blockIdx.x * a.nfp * a.wp;
#pragma unroll
  for (int q = 0; q < kLinfitAcc; ++q) {
    if (ti[q] < 0) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r)       // f64 16x16x4 result map: column lane & 15, row (lane >> 4) + 4 r
      part[(size_t)(16 * ti[q] + (lane >> 4) + 4 * r) * a.wp + 16 * tj[q] + (lane & 15)] = acc[q][r];
  }
}

// G[a][b] = sum over splits, in split order, of the partial tile entries; an entry below the tile diagonal of the
// symmetric part is read from its mirror.  G is [nfp][wp]; entries with a >= nf or b >= nf + nt are not written.
__global__ void linfit_gram_reduce_kernel(const double* __restrict__ part, double* __restrict__ G, int splits, int nf,
                                          int w, int nfp, int wp) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nf * w) return;
  const int ra = i / w, cb = i - ra * w;
  int sr = ra, sc = cb;
  if (cb < nf && (cb >> 4) < (ra >> 4)) { sr = cb; sc = ra; }
  double s = 0.0;
  for (int k = 0; k < splits; ++k) s += part[((size_t)k * nfp + sr) * wp + sc];
  G[(size_t)ra * wp + cb] = s;
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

__global__ __launch_bounds__(kLinfitThreads) void linfit_solve_kernel(const LinfitSolveDesc* __restrict__ descs,
                                                                       const int* __restrict__ order,
                                                                       const int* __restrict__ idxbuf, double* ws,
                                                                       double* __restrict__ coef,
                                                                       int* __restrict__ status,
                                                                       double* __restrict__ min_pivot) {
  __shared__ double P[(kLinfitMaxFeat + kLinfitMaxTargets) * kLinfitPs];
  __shared__ double dsc[kLinfitMaxFeat];      // D
  __shared__ double linv[kLinfitMaxFeat];     // 1 / L[j][j]
  __shared__ double s_min;
  __shared__ int s_bad;
  constexpr int T = kLinfitThreads, PS = kLinfitPs;
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
    for (int j0 = 0; j0 < n; j0 += kLinfitNb) {
      const int nbw = n - j0 < kLinfitNb ? n - j0 : kLinfitNb, pr = rows - j0;
      for (int e = t; e < pr * nbw; e += T) {
        const int r = e / nbw, c = e - r * nbw;
        P[r * PS + c] = M[(size_t)(j0 + r) * n + j0 + c];
      }
      __syncthreads();
      for (int jj = 0; jj < nbw; ++jj) {
        if (t == 0) {
          const double piv = P[jj * PS + jj];
          if (!(piv > 0.0) || !isfinite(piv)) { s_bad = 1; s_min = piv; }
          else {
            if (piv < s_min) s_min = piv;
            const double l = sqrt(piv);
            P[jj * PS + jj] = l;
            linv[j0 + jj] = 1.0 / l;
          }
        }
        __syncthreads();
        if (s_bad) break;
        const double l = P[jj * PS + jj];
        for (int r = jj + 1 + t; r < pr; r += T) P[r * PS + jj] /= l;
        __syncthreads();
        const int cw = nbw - jj - 1;
        for (int e = t; e < (pr - jj - 1) * cw; e += T) {
          const int r = jj + 1 + e / cw, c = jj + 1 + e % cw;
          if (r >= c) P[r * PS + c] = fma(-P[r * PS + jj], P[c * PS + jj], P[r * PS + c]);
        }
        __syncthreads();
      }
      if (s_bad) break;
      for (int e = t; e < pr * nbw; e += T) {
        const int r = e / nbw, c = e - r * nbw;
        M[(size_t)(j0 + r) * n + j0 + c] = P[r * PS + c];
      }
      const int c1 = j0 + nbw, w = n - c1, h = rows - c1;
      for (int e = t; e < h * w; e += T) {
        const int r = c1 + e / w, c = c1 + e % w;
        if (r < c) continue;
        double v = M[(size_t)r * n + c];
        for (int q = 0; q < nbw; ++q) v = fma(-P[(r - j0) * PS + q], P[(c - j0) * PS + q], v);
        M[(size_t)r * n + c] = v;
      }
      __syncthreads();
    }
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
