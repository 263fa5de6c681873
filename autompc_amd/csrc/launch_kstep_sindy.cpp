// launch_kstep_sindy.cpp -- ampc_kstep_errors_sindy: k-step prediction error sums of SINDy models (any mix of feature
// libraries, coefficients and time modes) over recorded trajectories in ONE launch (kstep_sindy_kernels.hpp).
// Compiled once per precision (-DAMPC_T=double|float, csrc/build.py); the f64 unit also carries the C entry, which
// checks the arguments and dispatches on the models' precision.
#include "host_common.hpp"
#include "kstep_sindy_kernels.hpp"

#ifndef AMPC_T
#error "compile with -DAMPC_T=double or -DAMPC_T=float"
#endif

template <typename T>
int kstep_sindy_impl(ampc_handle* const* models, int n_models, int n_traj, const int* traj_len, const double* obs,
                     const double* ctrls, int kmax, const double* inv_std, double* sq_err, double* sq_delta_err) {
  ampc_handle* h = models[0];
  for (int i = 1; i < n_models; ++i) HIP_OK(hipStreamSynchronize(models[i]->stream));   // (staging done)
  const int nx = h->nx, nu = h->nu;
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
  REQUIRE(total < (1LL << 31), "ampc_kstep_errors_sindy: more than 2^31 trajectory rows");
  // (the tile height is 64 whatever the call holds, and every LDS offset is the model's own: a model's sums are the
  //  same bits alone or in a batch; only the reserved bytes follow the largest model)
  const int tiles = (n_rows + kKsRows - 1) / kKsRows;
  size_t lds_bytes = 0;
  for (int i = 0; i < n_models; ++i) {
    const size_t b = kstep_sindy_lds_bytes(nx, nu, models[i]->s_ntab, want_d, sindy_stage_bytes<T>(models[i]),
                                           (int)sizeof(T));
    REQUIRE(b <= kLdsLimit,
            "ampc_kstep_errors_sindy: a model's per-thread columns (2 nx + nu + table entries, 64 rows) do not fit "
            "LDS with the error block");
    lds_bytes = std::max(lds_bytes, b);
  }
  REQUIRE((long long)tiles * n_models * kmax < (1LL << 31), "ampc_kstep_errors_sindy: too many partial sums");

  ScopedBuf d_obs, d_ctrl, d_inv, d_base, d_rem, d_part, d_dpart, d_out, d_desc;
  HIP_OK(d_obs.reserve((size_t)total * nx * 8));
  HIP_OK(d_ctrl.reserve((size_t)total * nu * 8));
  HIP_OK(d_base.reserve((size_t)n_rows * 4));
  HIP_OK(d_rem.reserve((size_t)n_rows * 4));
  HIP_OK(d_part.reserve((size_t)n_models * tiles * kmax * 8));
  HIP_OK(d_out.reserve((size_t)2 * n_models * kmax * 8));
  HIP_OK(hipMemcpyAsync(d_obs.p, obs, (size_t)total * nx * 8, hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipMemcpyAsync(d_ctrl.p, ctrls, (size_t)total * nu * 8, hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipMemcpyAsync(d_base.p, base.data(), (size_t)n_rows * 4, hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipMemcpyAsync(d_rem.p, rem.data(), (size_t)n_rows * 4, hipMemcpyHostToDevice, h->stream));
  if (want_d) {
    HIP_OK(d_dpart.reserve((size_t)n_models * tiles * kmax * 8));
    HIP_OK(d_inv.reserve((size_t)nx * 8));
    HIP_OK(hipMemcpyAsync(d_inv.p, inv_std, (size_t)nx * 8, hipMemcpyHostToDevice, h->stream));
  }
  // the descriptor table: every model's SindyDev (pointers into its handle's buffers)
  std::vector<SindyDev<T>> descs(n_models);
  for (int i = 0; i < n_models; ++i) descs[i] = sindy_of<T>(models[i]);
  HIP_OK(d_desc.reserve(descs.size() * sizeof(SindyDev<T>)));
  HIP_OK(hipMemcpyAsync(d_desc.p, descs.data(), descs.size() * sizeof(SindyDev<T>), hipMemcpyHostToDevice, h->stream));

  KstepSindyArgs a;
  a.obs = (const double*)d_obs.p; a.ctrls = (const double*)d_ctrl.p;
  a.inv_std = want_d ? (const double*)d_inv.p : nullptr;
  a.row_base = (const int*)d_base.p; a.row_rem = (const int*)d_rem.p;
  a.part = (double*)d_part.p; a.dpart = want_d ? (double*)d_dpart.p : nullptr;
  a.n_rows = n_rows; a.tiles = tiles; a.kmax = kmax;
  HIP_OK(allow_lds(kstep_sindy_kernel<T>, lds_bytes));
  // grid.y is limited to 65535 workgroups: more models than that go in slices of the same launch geometry
  for (int m0 = 0; m0 < n_models; m0 += 32768) {
    const int nm = std::min(32768, n_models - m0);
    KstepSindyArgs as = a;
    as.part = a.part + (size_t)m0 * tiles * kmax;
    if (want_d) as.dpart = a.dpart + (size_t)m0 * tiles * kmax;
    hipLaunchKernelGGL(kstep_sindy_kernel<T>, dim3(tiles, nm), dim3(kKsRows), lds_bytes, h->stream,
                       (const SindyDev<T>*)d_desc.p + m0, as);
  }
  HIP_OK(hipGetLastError());
  double* out = (double*)d_out.p;
  const int nr = n_models * kmax;
  hipLaunchKernelGGL(kstep_reduce_kernel<T>, dim3((nr + 255) / 256), dim3(256), 0, h->stream, (const double*)d_part.p,
                     out, n_models, tiles, kmax);
  if (want_d)
    hipLaunchKernelGGL(kstep_reduce_kernel<T>, dim3((nr + 255) / 256), dim3(256), 0, h->stream,
                       (const double*)d_dpart.p, out + nr, n_models, tiles, kmax);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(sq_err, out, (size_t)nr * 8, hipMemcpyDeviceToHost, h->stream));
  if (want_d) HIP_OK(hipMemcpyAsync(sq_delta_err, out + nr, (size_t)nr * 8, hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  return 0;
}

template int kstep_sindy_impl<AMPC_T>(ampc_handle* const*, int, int, const int*, const double*, const double*, int,
                                      const double*, double*, double*);

#ifdef AMPC_T_IS_F64
extern template int kstep_sindy_impl<float>(ampc_handle* const*, int, int, const int*, const double*, const double*,
                                            int, const double*, double*, double*);

extern "C" int ampc_kstep_errors_sindy(ampc_handle* const* models, int n_models, int n_traj, const int* traj_len,
                                       int obs_dim, const double* obs, const double* ctrls, int kmax,
                                       const double* inv_std, double* sq_err, double* sq_delta_err) {
  REQUIRE(models && n_models >= 1, "ampc_kstep_errors_sindy: no models");
  REQUIRE(n_traj >= 0 && (n_traj == 0 || traj_len), "ampc_kstep_errors_sindy: NULL trajectory lengths");
  REQUIRE(kmax >= 1, "ampc_kstep_errors_sindy: kmax must be >= 1");
  REQUIRE(sq_err, "ampc_kstep_errors_sindy: NULL sq_err");
  REQUIRE(!sq_delta_err || inv_std, "ampc_kstep_errors_sindy: sq_delta_err needs inv_std");
  ampc_handle* h = models[0];
  REQUIRE(h, "ampc_kstep_errors_sindy: NULL model handle");
  for (int i = 0; i < n_models; ++i) {
    const ampc_handle* m = models[i];
    REQUIRE(m, "ampc_kstep_errors_sindy: NULL model handle");
    REQUIRE(m->has_sindy,
            "ampc_kstep_errors_sindy: SINDy models only (ampc_set_sindy; MLP and linear models are scored by "
            "ampc_kstep_errors / ampc_kstep_errors_linear)");
    REQUIRE(m->device == h->device && m->precision == h->precision,
            "ampc_kstep_errors_sindy: models must share one device and one precision");
    REQUIRE(m->nx == h->nx, "ampc_kstep_errors_sindy: models must share the state dim");
    REQUIRE(m->nu == h->nu, "ampc_kstep_errors_sindy: models must share ctrl_dim");
  }
  REQUIRE(obs_dim == h->nx, "ampc_kstep_errors_sindy: obs_dim must be the models' state dim (the state is the observation)");
  long long total = 0;
  for (int i = 0; i < n_traj; ++i) {
    REQUIRE(traj_len[i] >= 0, "ampc_kstep_errors_sindy: negative trajectory length");
    total += traj_len[i];
  }
  REQUIRE(total == 0 || (obs && ctrls), "ampc_kstep_errors_sindy: NULL obs / ctrls");
  HIP_OK(hipSetDevice(h->device));
  return h->precision == AMPC_F64
             ? kstep_sindy_impl<double>(models, n_models, n_traj, traj_len, obs, ctrls, kmax, inv_std, sq_err,
                                        sq_delta_err)
             : kstep_sindy_impl<float>(models, n_models, n_traj, traj_len, obs, ctrls, kmax, inv_std, sq_err,
                                       sq_delta_err);
}
#endif
