// launch_lasso.cpp -- launchers of the lasso fit kernels (lasso_kernels.hpp).  f64 only: compiled once.  The Gram pass
// itself is linfit_gram_kernel, launched through launch_linfit.cpp.
#include "host_common.hpp"
#include "lasso_kernels.hpp"

size_t lasso_design_bytes() { return sizeof(LassoDesign); }
size_t lasso_pair_bytes() { return sizeof(LassoPair); }
int lasso_max_feat() { return kLassoMaxFeat; }

void lasso_pack_design(void* dst, const double* part, double* G, double* Qt, double* yy, int* bad, int nf, int nt,
                       int wp, int ldp, int splits, double m) {
  LassoDesign d{};
  d.part = part; d.G = G; d.Qt = Qt; d.yy = yy; d.bad = bad;
  d.nf = nf; d.nt = nt; d.wp = wp; d.ldp = ldp; d.splits = splits; d.m = m;
  std::memcpy(dst, &d, sizeof d);
}

void lasso_pack_pair(void* dst, const double* G, const double* q, const double* yy, const int* bad, double* out,
                     double alpha, int nf, int ldp, int id) {
  LassoPair p{};
  p.G = G; p.q = q; p.yy = yy; p.bad = bad; p.out = out; p.alpha = alpha; p.nf = nf; p.ldp = ldp; p.id = id;
  std::memcpy(dst, &p, sizeof p);
}

int lasso_launch_centre(hipStream_t st, const void* designs, int n_designs, int max_entries) {
  hipLaunchKernelGGL(lasso_centre_kernel, dim3((max_entries + 255) / 256, n_designs), dim3(256), 0, st,
                     (const LassoDesign*)designs);
  HIP_OK(hipGetLastError());
  return 0;
}

int lasso_launch_cd(hipStream_t st, int n_pairs, const void* pairs, void* status, void* margins, void* sweeps) {
  hipLaunchKernelGGL(lasso_cd_kernel, dim3(n_pairs), dim3(64), 0, st, (const LassoPair*)pairs, (int*)status,
                     (double*)margins, (int*)sweeps);
  HIP_OK(hipGetLastError());
  return 0;
}
