// launch_kstep_mlp.cpp -- launcher of kstep_mlp_table_kernel (kstep_mlp_kernels.hpp): stages the trajectories and the
// start points, runs every model of the table in ONE launch and reduces the per-tile partials.  f64 only: compiled once.
// The C entry, its argument checks and the packing of host-resident parameters are in api_kstep_mlp.cpp.
#include "host_common.hpp"
#include "kstep_mlp_kernels.hpp"

size_t kstep_mlp_model_bytes() { return sizeof(KstepMlpModel); }

// max hidden layers, hidden width, nx + nu, nx, nu
void kstep_mlp_limits(int out[5]) {
  out[0] = kMaxHidden; out[1] = kKmMaxWidth; out[2] = kKmMaxIn; out[3] = kKmMaxOut; out[4] = kKmMaxCtrl;
}

void kstep_mlp_pack_model(void* dst, int n_layers, int act, const int* dims, const double* const* w,
                          const double* const* b, const double* const* norm) {
  KstepMlpModel m{};
  m.n_layers = n_layers; m.act = act;
  for (int l = 0; l <= n_layers; ++l) m.dims[l] = dims[l];
  for (int l = 0; l < n_layers; ++l) { m.w[l] = w[l]; m.b[l] = b[l]; }
  for (int i = 0; i < 4; ++i) m.norm[i] = norm[i];
  std::memcpy(dst, &m, sizeof m);
}

// d_models: the table [n_models] in device memory, complete on `st`.  Synchronises `st` before it returns.
int kstep_mlp_launch(hipStream_t st, int n_models, const void* d_models, int nx, int nu, int n_traj,
                     const int* traj_len, const double* obs, const double* ctrls, int kmax, const double* inv_std,
                     double* sq_err, double* sq_delta_err) {
  // start points: (trajectory i, t), t = 0 .. L_i - 2
  long long total = 0;
  std::vector<int> base, rem;
  for (int i = 0; i < n_traj; ++i) {
    for (int t = 0; t + 1 < traj_len[i]; ++t) {
      base.push_back((int)(total + t));
      rem.push_back(traj_len[i] - 1 - t);
    }
    total += traj_len[i];
  }
  const int n_rows = (int)base.size();
  const bool want_d = sq_delta_err != nullptr;
  if (n_rows == 0) {
    std::fill(sq_err, sq_err + (size_t)n_models * kmax, 0.0);
    if (want_d) std::fill(sq_delta_err, sq_delta_err + (size_t)n_models * kmax, 0.0);
    return 0;
  }
  REQUIRE(total < (1LL << 31), "ampc_kstep_errors_mlp: more than 2^31 trajectory rows");
  // (the tile height is 16 whatever the call holds: a model's sums are the same bits alone or in a batch)
  const int tiles = (n_rows + kKmRows - 1) / kKmRows;
  REQUIRE((long long)tiles * n_models * kmax < (1LL << 31), "ampc_kstep_errors_mlp: too many partial sums");
  static_assert(kKmLdsBytes <= kLdsLimit / 2, "two workgroups per CU");

  ScopedBuf d_obs, d_ctrl, d_inv, d_base, d_rem, d_part, d_dpart, d_out;
  HIP_OK(d_obs.reserve((size_t)total * nx * 8));
  HIP_OK(d_ctrl.reserve((size_t)total * nu * 8));
  HIP_OK(d_base.reserve((size_t)n_rows * 4));
  HIP_OK(d_rem.reserve((size_t)n_rows * 4));
  HIP_OK(d_part.reserve((size_t)n_models * tiles * kmax * 8));
  HIP_OK(d_out.reserve((size_t)2 * n_models * kmax * 8));
  HIP_OK(hipMemcpyAsync(d_obs.p, obs, (size_t)total * nx * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_ctrl.p, ctrls, (size_t)total * nu * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_base.p, base.data(), (size_t)n_rows * 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_rem.p, rem.data(), (size_t)n_rows * 4, hipMemcpyHostToDevice, st));
  if (want_d) {
    HIP_OK(d_dpart.reserve((size_t)n_models * tiles * kmax * 8));
    HIP_OK(d_inv.reserve((size_t)nx * 8));
    HIP_OK(hipMemcpyAsync(d_inv.p, inv_std, (size_t)nx * 8, hipMemcpyHostToDevice, st));
  }
  KstepMlpArgs a;
  a.obs = (const double*)d_obs.p; a.ctrls = (const double*)d_ctrl.p;
  a.inv_std = want_d ? (const double*)d_inv.p : nullptr;
  a.row_base = (const int*)d_base.p; a.row_rem = (const int*)d_rem.p;
  a.part = (double*)d_part.p; a.dpart = want_d ? (double*)d_dpart.p : nullptr;
  a.n_rows = n_rows; a.tiles = tiles; a.kmax = kmax; a.nx = nx; a.nu = nu;
  HIP_OK(allow_lds(kstep_mlp_table_kernel, kKmLdsBytes));
  // grid.y is limited to 65535 workgroups: more models than that go in slices of the same launch geometry
  for (int m0 = 0; m0 < n_models; m0 += 32768) {
    const int nm = std::min(32768, n_models - m0);
    KstepMlpArgs as = a;
    as.part = a.part + (size_t)m0 * tiles * kmax;
    if (want_d) as.dpart = a.dpart + (size_t)m0 * tiles * kmax;
    hipLaunchKernelGGL(kstep_mlp_table_kernel, dim3(tiles, nm), dim3(kKmThreads), kKmLdsBytes, st,
                       (const KstepMlpModel*)d_models + m0, as);
  }
  HIP_OK(hipGetLastError());
  double* out = (double*)d_out.p;
  const int nr = n_models * kmax;
  hipLaunchKernelGGL(kstep_reduce_kernel<double>, dim3((nr + 255) / 256), dim3(256), 0, st, (const double*)d_part.p,
                     out, n_models, tiles, kmax);
  if (want_d)
    hipLaunchKernelGGL(kstep_reduce_kernel<double>, dim3((nr + 255) / 256), dim3(256), 0, st,
                       (const double*)d_dpart.p, out + nr, n_models, tiles, kmax);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(sq_err, out, (size_t)nr * 8, hipMemcpyDeviceToHost, st));
  if (want_d) HIP_OK(hipMemcpyAsync(sq_delta_err, out + nr, (size_t)nr * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  return 0;
}
