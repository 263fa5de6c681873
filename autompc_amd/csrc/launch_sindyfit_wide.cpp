// launch_sindyfit_wide.cpp -- launchers of the wide thresholded SINDy fit kernels (sindyfit_wide_kernels.hpp).  f64
// only: compiled once.
#include "host_common.hpp"
#include "sindyfit_wide_kernels.hpp"

size_t sindyfit_wide_design_bytes() { return sizeof(SindyfitWideDesign); }
size_t sindyfit_wide_item_bytes() { return sizeof(SindyfitWideItem); }
int sindyfit_wide_max_feat() { return kWideMaxFeat; }
int sindyfit_wide_acc() { return kWideAcc; }

void sindyfit_wide_pack_design(void* dst, const void* cols, const void* pool, const void* groups, double* G, int nf,
                               int w, int n_groups) {
  SindyfitWideDesign d{};
  d.cols = (const SindyfitCol*)cols; d.pool = (const int*)pool; d.groups = (const int*)groups; d.G = G;
  d.nf = nf; d.w = w; d.wp = (w + 15) / 16 * 16; d.nfp = (nf + 15) / 16 * 16; d.n_groups = n_groups;
  std::memcpy(dst, &d, sizeof d);
}

void sindyfit_wide_pack_item(void* dst, int design, int s0, int s1, int first, long long theta) {
  SindyfitWideItem it{design, s0, s1, first, theta};
  std::memcpy(dst, &it, sizeof it);
}

// One wave of the Gram pass: [Theta | Y] of the items' splits into the scratch, then the rank-k pass onto the Grams.
int sindyfit_wide_launch_gram(hipStream_t st, int R, int nx, int nu, const void* obs, const void* ctrls,
                              const void* ycont, const void* row_start, const void* designs, const void* items,
                              int n_items, int max_splits, int max_wp, int max_groups, void* theta) {
  SindyfitGramArgs a{};
  a.obs = (const double*)obs; a.ctrls = (const double*)ctrls; a.ycont = (const double*)ycont;
  a.row_start = (const int*)row_start; a.designs = nullptr;
  a.R = R; a.nx = nx; a.nu = nu;
  a.splits = (R + kFitSplitRows - 1) / kFitSplitRows;
  const int row_blocks = max_splits * (kFitSplitRows / kWideThetaRows);
  REQUIRE(row_blocks <= 65535 && n_items <= 65535, "internal: sindyfit wide Gram wave exceeds the grid limits");
  hipLaunchKernelGGL(sindyfit_wide_theta_kernel,
                     dim3((max_wp + kWideThetaCols - 1) / kWideThetaCols, row_blocks, n_items), dim3(kWideThetaCols),
                     0, st, a, (const SindyfitWideDesign*)designs, (const SindyfitWideItem*)items, (double*)theta);
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(sindyfit_wide_gram_kernel, dim3((max_groups + 3) / 4, n_items), dim3(256), 0, st,
                     (const SindyfitWideDesign*)designs, (const SindyfitWideItem*)items, (const double*)theta);
  HIP_OK(hipGetLastError());
  return 0;
}

// One wave of the solve: pairs order[first .. first + count), the widest of them of maxn features.
int sindyfit_wide_launch_solve(hipStream_t st, int first, int count, int maxn, const void* descs, const void* order,
                               void* ws, void* coef, void* bad, void* min_pivot, void* min_margin, void* iters,
                               double alpha, int max_iter) {
  REQUIRE(maxn >= 1 && maxn <= kWideMaxFeat, "internal: sindyfit wide solve wider than the kernel's limit");
  const size_t lds = wide_solve_lds(maxn);
  REQUIRE(lds <= kLdsLimit, "internal: sindyfit wide solve arrays do not fit LDS");
  HIP_OK(allow_lds(sindyfit_wide_solve_kernel, lds));
  hipLaunchKernelGGL(sindyfit_wide_solve_kernel, dim3(count), dim3(kWideThreads), lds, st,
                     (const SindyfitSolveDesc*)descs, (const int*)order, first, maxn, (double*)ws, (double*)coef,
                     (int*)bad, (double*)min_pivot, (double*)min_margin, (int*)iters, alpha, max_iter);
  HIP_OK(hipGetLastError());
  return 0;
}
