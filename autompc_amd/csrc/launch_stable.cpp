// launch_stable.cpp -- launchers of the stable fit kernels (stable_kernels.hpp).  f64 only: compiled once.  The Gram
// pass itself is linfit_gram_kernel and the least-squares start linfit_solve_kernel, launched through
// launch_linfit.cpp.
#include "host_common.hpp"
#include "stable_kernels.hpp"

size_t stable_desc_bytes() { return sizeof(StableDesc); }
int stable_max_n() { return kStableMaxN; }
long long stable_scratch_doubles(int n, int nu) { return stable_ws_doubles(n, nu); }

void stable_pack_desc(void* dst, const double* G, const double* W0, const double* yy, const int* w0_status, double* ws,
                      double* out, double tie, int n, int nu, int ldg, int id) {
  StableDesc d{};
  d.G = G; d.W0 = W0; d.yy = yy; d.w0_status = w0_status; d.ws = ws; d.out = out;
  d.tie = tie; d.n = n; d.nu = nu; d.ldg = ldg; d.id = id;
  std::memcpy(dst, &d, sizeof d);
}

// G [nf][wp] and yy [nt] from the partial tiles [splits][wp][wp]
int stable_launch_gram(hipStream_t st, const void* part, void* G, void* yy, int splits, int nf, int nt, int wp) {
  const int entries = nf * (nf + nt) + nt;
  hipLaunchKernelGGL(stable_gram_kernel, dim3((entries + 255) / 256), dim3(256), 0, st, (const double*)part,
                     (double*)G, (double*)yy, splits, nf, nt, wp);
  HIP_OK(hipGetLastError());
  return 0;
}

int stable_launch_fgm(hipStream_t st, int n_configs, const void* descs, void* status, void* error, void* iterations,
                      void* trials, void* margin) {
  REQUIRE(kStableLdsBytes <= kLdsLimit, "internal: the stable fit's matrices do not fit LDS");
  HIP_OK(allow_lds(stable_fgm_kernel, kStableLdsBytes));
  hipLaunchKernelGGL(stable_fgm_kernel, dim3(n_configs), dim3(kStableThreads), kStableLdsBytes, st,
                     (const StableDesc*)descs, (int*)status, (double*)error, (int*)iterations, (int*)trials,
                     (double*)margin);
  HIP_OK(hipGetLastError());
  return 0;
}
