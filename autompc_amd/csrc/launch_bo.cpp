// launch_bo.cpp -- launchers of the Bayesian-optimisation proposal kernels (bo_kernels.hpp).  f64 only: compiled once.
#include "host_common.hpp"
#include "bo_kernels.hpp"

int bo_max_n() { return kBoMaxN; }
int bo_max_d() { return kBoMaxD; }
int bo_max_g() { return kBoMaxG; }
int bo_max_m() { return kBoMaxM; }
int bo_max_q() { return kBoMaxQ; }
int bo_pool_block() { return kBoPoolBlock; }

// Kernel matrices of all G rows, then their factorisations: Kall [G][n + 1][n], lml / status [G].
int bo_launch_fit(hipStream_t st, int n, int d, int G, const void* X, const void* z, const void* hw, const void* hnoise,
                  void* Kall, void* lml, void* status) {
  const long long elems = (long long)(n + 1) * n;
  hipLaunchKernelGGL(bo_kmat_kernel, dim3((unsigned)((elems + 255) / 256), G), dim3(256), 0, st, (const double*)X,
                     (const double*)z, (const double*)hw, (const double*)hnoise, n, d, (double*)Kall);
  HIP_OK(hipGetLastError());
  const size_t lds = bo_factor_lds(n);
  REQUIRE(lds <= kLdsLimit, "internal: the proposal's factorisation arrays do not fit LDS");
  HIP_OK(allow_lds(bo_factor_kernel, lds));
  hipLaunchKernelGGL(bo_factor_kernel, dim3(G), dim3(kWideThreads), lds, st, (double*)Kall, n, (double*)lml,
                     (int*)status);
  HIP_OK(hipGetLastError());
  return 0;
}

// Posterior of the factored row L over the pool: V rows 0 .. n - 1, mu, var0 (= var), ei.
int bo_launch_posterior(hipStream_t st, const void* L, const void* X, const void* w, const void* pool, int n, int d,
                        int m, int Mp, double zmin, void* V, void* mu, void* var0, void* var, void* ei) {
  const size_t lds = bo_posterior_lds(d);
  REQUIRE(lds <= kLdsLimit, "internal: the proposal's posterior arrays do not fit LDS");
  HIP_OK(allow_lds(bo_posterior_kernel, lds));
  hipLaunchKernelGGL(bo_posterior_kernel, dim3(Mp / kBoPoolBlock), dim3(kBoPostThreads), lds, st, (const double*)L,
                     (const double*)X, (const double*)w, (const double*)pool, n, d, m, Mp, zmin, (double*)V,
                     (double*)mu, (double*)var0, (double*)var, (double*)ei);
  HIP_OK(hipGetLastError());
  return 0;
}

// q greedy picks: an argmax launch per pick and, between picks, the believer row of the pick just made.
int bo_launch_picks(hipStream_t st, int n, int d, int m, int Mp, int q, const void* pool, const void* w, double noise,
                    double zmin, void* V, const void* mu, void* var, void* ei, void* picked, void* picks,
                    void* pick_ei, void* pick_margin) {
  for (int s = 0; s < q; ++s) {
    hipLaunchKernelGGL(bo_argmax_kernel, dim3(1), dim3(kBoArgThreads), 0, st, (const double*)ei, (int*)picked, m, s,
                       (int*)picks, (double*)pick_ei, (double*)pick_margin);
    HIP_OK(hipGetLastError());
    if (s + 1 == q) break;
    hipLaunchKernelGGL(bo_append_kernel, dim3((m + 255) / 256), dim3(256), 0, st, (double*)V, Mp, n + s,
                       (const int*)picks, s, (const double*)pool, (const double*)w, d, noise, zmin, m,
                       (const double*)mu, (double*)var, (double*)ei);
    HIP_OK(hipGetLastError());
  }
  return 0;
}
