// gram_frame.hpp -- the frame the GPU fits share (linfit_kernels.hpp, sindyfit_kernels.hpp, lasso_kernels.hpp): device
// functions only, the kernels that call them stay in the families' headers.
//
// gram_tiles: partial tiles of G = F' [F | Y] of one design.  A design row is one data row t of a trajectory that has
// a successor; the columns of [F | Y] are formed ON THE FLY from the data by the family's per-column rule, sixteen
// rows at a time into LDS: the wide design matrix never exists in HBM.  Accumulation on v_mfma_f64_16x16x4_f64, one
// accumulator per 16 x 16 tile of the design's tile list.
//
// Determinism.  Rows are split over workgroups by ROW INDEX only (kFitSplitRows consecutive data rows each, whatever
// the design's width); rows that are no design rows contribute exact zeros.  An entry's partial sum is one MFMA
// accumulator's k-ordered chain over the split's rows, the partials are summed over splits in order by
// gram_split_sum.  No atomics: G[a][b] of two given columns has the same bits whatever other columns or designs the
// call holds, and from run to run.
//
// fit_cholesky: the right-looking blocked Cholesky of the solve kernels: a panel of kFitNb columns is factored in
// LDS, the trailing matrix (global memory, L2-resident: at most 528 x 272 doubles) is updated from the panel.  Rows
// below the square part (right-hand sides) ride along: the factorisation leaves L^-1 of them there.
#ifndef AMPC_GRAM_FRAME_HPP
#define AMPC_GRAM_FRAME_HPP
#include <hip/hip_runtime.h>

namespace ampc {

constexpr int kFitThreads = 256;
constexpr int kFitSplitRows = 512;        // data rows per workgroup of the Gram pass (a constant: see Determinism)
constexpr int kFitChunk = 16;             // design rows formed in LDS at a time
constexpr int kFitAcc = 8;                // tiles (accumulators) per wave
constexpr int kFitMaxFeat = 272;          // features per design: 256 states + 16 controls
constexpr int kFitNb = 8, kFitPs = kFitNb + 1;   // Cholesky panel width, LDS row stride of the panel

typedef double fit_d4 __attribute__((ext_vector_type(4)));

// LDS row stride (doubles) of the design chunk: an odd multiple of 16, so the four rows of an MFMA fragment read
// fall on two disjoint halves of the banks
constexpr int gram_lds_stride(int wp) { return (wp / 16) % 2 ? wp : wp + 16; }

// Workgroup (blockIdx.x, blockIdx.y) = (s, q) accumulates tiles 32 q .. 32 q + 31 of the list (ti | tj << 16) over
// data rows kFitSplitRows s .. and writes them to part[s] ([nfp][wp]).  value(col, g, start) is column col's entry of
// data row g, whose trajectory starts at row start; Col::zero() is the rule of a padding column; lds holds
// kFitChunk * stride doubles; every thread forms at most kCols columns (wp <= kCols * kFitThreads).
template <int kCols, class Col, class Value>
__device__ __forceinline__ void gram_tiles(double* lds, const Col* cols, const int* tiles, int n_tiles, int wp, int nfp,
                                           int stride, double* part, int R, const int* row_start, Value value) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int ti[kFitAcc], tj[kFitAcc];
  fit_d4 acc[kFitAcc];
#pragma unroll
  for (int q = 0; q < kFitAcc; ++q) {
    const int id = ((int)blockIdx.y * 4 + wave) * kFitAcc + q;
    const int w = id < n_tiles ? tiles[id] : -1;
    ti[q] = w < 0 ? -1 : (w & 0xffff);
    tj[q] = w < 0 ? -1 : (w >> 16);
    acc[q] = fit_d4{0.0, 0.0, 0.0, 0.0};
  }
  Col col[kCols];
#pragma unroll
  for (int m = 0; m < kCols; ++m) {
    const int c = tid + m * kFitThreads;
    col[m] = c < wp ? cols[c] : Col::zero();
  }
  const int row0 = (int)blockIdx.x * kFitSplitRows;
  const int rend = row0 + kFitSplitRows < R ? row0 + kFitSplitRows : R;
  for (int c0 = row0; c0 < rend; c0 += kFitChunk) {
#pragma unroll
    for (int m = 0; m < kCols; ++m) {
      const int c = tid + m * kFitThreads;
      if (c >= wp) continue;
      for (int r = 0; r < kFitChunk; ++r) {
        const int g = c0 + r;
        const int start = g < rend ? row_start[g] : -1;
        // a row without a successor is dropped by a SELECT (its values are never formed)
        lds[r * stride + c] = start < 0 ? 0.0 : value(col[m], g, start);
      }
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < kFitChunk / 4; ++ks) {
      const double* rowp = lds + (4 * ks + (lane >> 4)) * stride + (lane & 15);
#pragma unroll
      for (int q = 0; q < kFitAcc; ++q)
        if (ti[q] >= 0)
          acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(rowp[16 * ti[q]], rowp[16 * tj[q]], acc[q], 0, 0, 0);
    }
    __syncthreads();
  }
  part += (size_t)blockIdx.x * nfp * wp;
#pragma unroll
  for (int q = 0; q < kFitAcc; ++q) {
    if (ti[q] < 0) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r)       // f64 16x16x4 result map: column lane & 15, row (lane >> 4) + 4 r
      part[(size_t)(16 * ti[q] + (lane >> 4) + 4 * r) * wp + 16 * tj[q] + (lane & 15)] = acc[q][r];
  }
}

// Sum over the row splits, in split order, of entry (a, b) of the partial tiles ([splits][prows][wp]).  Of the
// symmetric part only the tiles on and above the diagonal exist: with sym (column b belongs to it, too) an entry below
// the tile diagonal is read from its mirror.
__device__ __forceinline__ double gram_split_sum(const double* part, int splits, int prows, int wp, int a, int b,
                                                 bool sym) {
  if (sym && (b >> 4) < (a >> 4)) { const int t = a; a = b; b = t; }
  double s = 0.0;
  for (int k = 0; k < splits; ++k) s += part[((size_t)k * prows + a) * wp + b];
  return s;
}

// Factors the leading n x n block of M ([rows][n], rows >= n) in place, all threads of a kFitThreads workgroup
// together; P is the LDS panel ([rows][kFitPs]), linv takes 1 / L[j][j].  A pivot that is not positive and finite
// sets bad, is left in bad_pivot and ends the factorisation (M is then unfinished); min_pivot is lowered to the
// smallest squared pivot.  bad, bad_pivot and min_pivot are shared variables of the caller; bad must be 0 on entry.
__device__ __forceinline__ void fit_cholesky(double* M, int rows, int n, double* P, double* linv, int& bad,
                                             double& bad_pivot, double& min_pivot) {
  constexpr int T = kFitThreads, PS = kFitPs;
  const int t = threadIdx.x;
  for (int j0 = 0; j0 < n; j0 += kFitNb) {
    const int nbw = n - j0 < kFitNb ? n - j0 : kFitNb, pr = rows - j0;
    for (int e = t; e < pr * nbw; e += T) {
      const int r = e / nbw, c = e - r * nbw;
      P[r * PS + c] = M[(size_t)(j0 + r) * n + j0 + c];
    }
    __syncthreads();
    for (int jj = 0; jj < nbw; ++jj) {
      if (t == 0) {
        const double piv = P[jj * PS + jj];
        if (!(piv > 0.0) || !isfinite(piv)) { bad = 1; bad_pivot = piv; }
        else {
          if (piv < min_pivot) min_pivot = piv;
          const double l = sqrt(piv);
          P[jj * PS + jj] = l;
          linv[j0 + jj] = 1.0 / l;
        }
      }
      __syncthreads();
      if (bad) break;
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
    if (bad) break;
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

}  // namespace ampc
#endif
