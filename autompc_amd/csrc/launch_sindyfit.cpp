// launch_sindyfit.cpp -- launchers of the thresholded SINDy fit kernels (sindyfit_kernels.hpp).  f64 only: compiled once.
#include "host_common.hpp"
#include "sindyfit_kernels.hpp"

size_t sindyfit_col_bytes() { return sizeof(SindyfitCol); }
size_t sindyfit_design_bytes() { return sizeof(SindyfitDesign); }
size_t sindyfit_desc_bytes() { return sizeof(SindyfitSolveDesc); }
int sindyfit_max_state() { return kSindyfitMaxState; }
int sindyfit_max_ctrl() { return kSindyfitMaxCtrl; }
int sindyfit_zero_kind() { return SFC_ZERO; }
int sindyfit_next_obs_kind() { return SFC_NEXT_OBS; }
int sindyfit_ycont_kind() { return SFC_YCONT; }

void sindyfit_pack_col(void* dst, int kind, int a0, int a1, double par) {
  SindyfitCol c{kind, a0, a1, 0, par};
  std::memcpy(dst, &c, sizeof c);
}

void sindyfit_pack_design(void* dst, const void* cols, const void* pool, const void* tiles, double* part, double* G,
                          int nf, int w, int n_tiles) {
  SindyfitDesign d{};
  d.cols = (const SindyfitCol*)cols; d.pool = (const int*)pool; d.tiles = (const int*)tiles;
  d.part = part; d.G = G;
  d.nf = nf; d.w = w; d.wp = (w + 15) / 16 * 16; d.nfp = (nf + 15) / 16 * 16; d.n_tiles = n_tiles;
  d.lds_stride = gram_lds_stride(d.wp);
  std::memcpy(dst, &d, sizeof d);
}

void sindyfit_pack_desc(void* dst, int n, int tcol, int id, const double* g, long long ldg, long long ws,
                        long long out, double threshold) {
  SindyfitSolveDesc d{};
  d.n = n; d.tcol = tcol; d.id = id;
  d.g = g; d.ldg = ldg; d.ws = ws; d.out = out; d.threshold = threshold;
  std::memcpy(dst, &d, sizeof d);
}

// Grams of all designs: partial tiles in one launch, then the ordered sums in one launch.
int sindyfit_launch_gram(hipStream_t st, int R, int nx, int nu, const void* obs, const void* ctrls,
                         const void* ycont, const void* row_start, const void* designs, int n_designs,
                         int max_tiles, int max_wp, int max_entries) {
  SindyfitGramArgs a{};
  a.obs = (const double*)obs; a.ctrls = (const double*)ctrls; a.ycont = (const double*)ycont;
  a.row_start = (const int*)row_start; a.designs = (const SindyfitDesign*)designs;
  a.R = R; a.nx = nx; a.nu = nu;
  a.splits = (R + kFitSplitRows - 1) / kFitSplitRows;
  REQUIRE(max_wp <= kSindyfitMaxCols, "internal: sindyfit design wider than the kernel's column frame");
  const size_t lds = (size_t)kFitChunk * gram_lds_stride(max_wp) * sizeof(double);
  REQUIRE(lds <= kLdsLimit, "internal: sindyfit design chunk does not fit LDS");
  HIP_OK(allow_lds(sindyfit_gram_kernel, lds));
  const int groups = (max_tiles + 4 * kFitAcc - 1) / (4 * kFitAcc);
  hipLaunchKernelGGL(sindyfit_gram_kernel, dim3(a.splits, groups, n_designs), dim3(kFitThreads), lds, st, a);
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(sindyfit_gram_reduce_kernel, dim3((max_entries + 255) / 256, n_designs), dim3(256), 0, st,
                     (const SindyfitDesign*)designs, a.splits);
  HIP_OK(hipGetLastError());
  return 0;
}

int sindyfit_launch_solve(hipStream_t st, int n, const void* descs, const void* order, void* ws, void* coef,
                          void* bad, void* min_pivot, void* min_margin, void* iters, double alpha, int max_iter) {
  hipLaunchKernelGGL(sindyfit_solve_kernel, dim3(n), dim3(kFitThreads), 0, st, (const SindyfitSolveDesc*)descs,
                     (const int*)order, (double*)ws, (double*)coef, (int*)bad, (double*)min_pivot,
                     (double*)min_margin, (int*)iters, alpha, max_iter);
  HIP_OK(hipGetLastError());
  return 0;
}
