// launch_linfit.cpp -- launchers of the least-squares fit kernels (linfit_kernels.hpp).  f64 only: compiled once.
#include "host_common.hpp"
#include "linfit_kernels.hpp"

size_t linfit_col_bytes() { return sizeof(LinfitCol); }
size_t linfit_desc_bytes() { return sizeof(LinfitSolveDesc); }

void linfit_pack_col(void* dst, int src, int lag, int j, int fn) {
  LinfitCol c{src, lag, j, fn};
  std::memcpy(dst, &c, sizeof c);
}

void linfit_pack_desc(void* dst, int n, int nt, int tcol, int id, const double* g, long long ldg, long long idx,
                      long long ws, long long out) {
  LinfitSolveDesc d{};
  d.n = n; d.nt = nt; d.tcol = tcol; d.id = id;
  d.g = g; d.ldg = ldg; d.idx = idx; d.ws = ws; d.out = out;
  std::memcpy(dst, &d, sizeof d);
}

// Partial tiles of one design's Gram: part holds splits * nfp * wp doubles (tile rows up to nfp / 16).
int linfit_launch_gram_part(hipStream_t st, int R, int no, int nu, const void* obs, const void* ctrls,
                            const void* row_start, const void* cols, const void* prog, const void* tiles, int n_tiles,
                            int wp, int nfp, void* part) {
  const int splits = (R + kFitSplitRows - 1) / kFitSplitRows;
  LinfitGramArgs a{};
  a.obs = (const double*)obs; a.ctrls = (const double*)ctrls; a.row_start = (const int*)row_start;
  a.cols = (const LinfitCol*)cols; a.prog = (const double*)prog; a.tiles = (const int*)tiles;
  a.part = (double*)part;
  a.R = R; a.no = no; a.nu = nu; a.wp = wp; a.nfp = nfp; a.n_tiles = n_tiles; a.lds_stride = gram_lds_stride(wp);
  const size_t lds = (size_t)kFitChunk * a.lds_stride * sizeof(double);
  REQUIRE(lds <= kLdsLimit, "internal: linfit design chunk does not fit LDS");
  HIP_OK(allow_lds(linfit_gram_kernel, lds));
  const int groups = (n_tiles + 4 * kFitAcc - 1) / (4 * kFitAcc);
  hipLaunchKernelGGL(linfit_gram_kernel, dim3(splits, groups), dim3(kFitThreads), lds, st, a);
  HIP_OK(hipGetLastError());
  return 0;
}

// Gram of one design: partial tiles, then the ordered sum.  part holds splits * nfp * wp doubles, G nfp * wp.
int linfit_launch_gram(hipStream_t st, int R, int no, int nu, const void* obs, const void* ctrls,
                       const void* row_start, const void* cols, const void* prog, const void* tiles, int n_tiles,
                       int nf, int nt, void* part, void* G) {
  const int wp = (nf + nt + 15) / 16 * 16, nfp = (nf + 15) / 16 * 16;
  const int splits = (R + kFitSplitRows - 1) / kFitSplitRows;
  if (int rc = linfit_launch_gram_part(st, R, no, nu, obs, ctrls, row_start, cols, prog, tiles, n_tiles, wp, nfp, part))
    return rc;
  const int w = nf + nt;
  hipLaunchKernelGGL(linfit_gram_reduce_kernel, dim3((nf * w + 255) / 256), dim3(256), 0, st, (const double*)part,
                     (double*)G, splits, nf, w, nfp, wp);
  HIP_OK(hipGetLastError());
  return 0;
}

int linfit_launch_solve(hipStream_t st, int n, const void* descs, const void* order, const void* idx, void* ws,
                        void* coef, void* status, void* min_pivot) {
  hipLaunchKernelGGL(linfit_solve_kernel, dim3(n), dim3(kFitThreads), 0, st, (const LinfitSolveDesc*)descs,
                     (const int*)order, (const int*)idx, (double*)ws, (double*)coef, (int*)status,
                     (double*)min_pivot);
  HIP_OK(hipGetLastError());
  return 0;
}
