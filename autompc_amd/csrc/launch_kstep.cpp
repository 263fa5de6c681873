// launch_kstep.cpp -- ampc_kstep_errors: k-step prediction error sums of many same-shape models over recorded
// trajectories (kstep_kernels.hpp).  Compiled once per precision (-DAMPC_T=double|float, csrc/build.py); the
// f64 unit also carries the C entry, which dispatches on the models' precision.
#include "host_common.hpp"
#include "kstep_kernels.hpp"

#ifndef AMPC_T
#error "compile with -DAMPC_T=double or -DAMPC_T=float"
#endif

template <typename T>
int kstep_impl(ampc_handle* const* models, int n_models, int n_traj, const int* traj_len, int obs_dim,
               const double* obs, const double* ctrls, const double* init_states, int kmax, const double* inv_std,
               double* sq_err, double* sq_delta_err) {
  ampc_handle* h = models[0];
  const MlpDev<T>& m = model_of<T>(h);
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
  if (n_rows == 0) {
    std::fill(sq_err, sq_err + (size_t)n_models * kmax, 0.0);
    if (sq_delta_err) std::fill(sq_delta_err, sq_delta_err + (size_t)n_models * kmax, 0.0);
    return 0;
  }
  REQUIRE(total < (1LL << 31), "ampc_kstep_errors: more than 2^31 trajectory rows");
  const bool want_d = sq_delta_err != nullptr;
  // error scratch [2][M][obs_dim] + [2][M] doubles behind the tile's own LDS regions; sized for the tallest tile
  auto extra_of = [&](int M) { return (size_t)(2 * M * obs_dim + 2 * M) * (8 / sizeof(T)) + 2; };
  // (the tile height depends on the data only, not on how many models share the call: a model's sums are the
  //  same bits alone or in a batch)
  const int mt = choose_mt<T>(h, m, n_rows, extra_of(64));
  const int M = 16 * mt, tiles = (n_rows + M - 1) / M;
  const size_t extra = extra_of(M);
  TileLds L = tile_lds_for<T>(h, m, M, extra);
  const size_t err_off_bytes = (size_t)L.extra * sizeof(T);        // L.extra is a multiple of 4 elements: 16 B aligned
  REQUIRE(err_off_bytes % 8 == 0, "internal: kstep error scratch misaligned");
  const size_t lds_bytes = err_off_bytes + (size_t)(2 * M * obs_dim + 2 * M) * sizeof(double);
  REQUIRE(lds_bytes <= kLdsLimit, "ampc_kstep_errors: the model's tile does not fit LDS with the error scratch");

  ScopedBuf d_obs, d_ctrl, d_init, d_inv, d_base, d_rem, d_part, d_dpart, d_out;
  HIP_OK(d_obs.reserve((size_t)total * obs_dim * 8));
  HIP_OK(d_ctrl.reserve((size_t)total * nu * 8));
  HIP_OK(d_base.reserve((size_t)n_rows * 4));
  HIP_OK(d_rem.reserve((size_t)n_rows * 4));
  HIP_OK(d_part.reserve((size_t)n_models * tiles * kmax * 8));
  HIP_OK(d_out.reserve((size_t)2 * n_models * kmax * 8));
  HIP_OK(hipMemcpyAsync(d_obs.p, obs, (size_t)total * obs_dim * 8, hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipMemcpyAsync(d_ctrl.p, ctrls, (size_t)total * nu * 8, hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipMemcpyAsync(d_base.p, base.data(), (size_t)n_rows * 4, hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipMemcpyAsync(d_rem.p, rem.data(), (size_t)n_rows * 4, hipMemcpyHostToDevice, h->stream));
  if (init_states) {
    HIP_OK(d_init.reserve((size_t)n_models * total * nx * 8));
    HIP_OK(hipMemcpyAsync(d_init.p, init_states, (size_t)n_models * total * nx * 8, hipMemcpyHostToDevice, h->stream));
  }
  if (want_d) {
    HIP_OK(d_dpart.reserve((size_t)n_models * tiles * kmax * 8));
    HIP_OK(d_inv.reserve((size_t)obs_dim * 8));
    HIP_OK(hipMemcpyAsync(d_inv.p, inv_std, (size_t)obs_dim * 8, hipMemcpyHostToDevice, h->stream));
  }
  KstepArgs a;
  a.obs = (const double*)d_obs.p; a.ctrls = (const double*)d_ctrl.p;
  a.init = init_states ? (const double*)d_init.p : nullptr;
  a.inv_std = want_d ? (const double*)d_inv.p : nullptr;
  a.row_base = (const int*)d_base.p; a.row_rem = (const int*)d_rem.p;
  a.part = (double*)d_part.p; a.dpart = want_d ? (double*)d_dpart.p : nullptr;
  a.total = total; a.n_rows = n_rows; a.tiles = tiles; a.kmax = kmax; a.obs_dim = obs_dim;
  a.err_off = (int)(err_off_bytes / 8);
  // one launch per model, with its own descriptor (same shape: same tile geometry and LDS map; kstep_kernels.hpp)
  AMPC_DISPATCH(h, mt, {
    auto k = kstep_error_kernel<T, NT, MT, W, DynShape, WD>;
    HIP_OK(allow_lds(k, lds_bytes));
    for (int i = 0; i < n_models; ++i)
      hipLaunchKernelGGL(k, dim3(tiles), dim3(64 * W), lds_bytes, h->stream, model_of<T>(models[i]), L, a, i);
  });
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

template int kstep_impl<AMPC_T>(ampc_handle* const*, int, int, const int*, int, const double*, const double*,
                                const double*, int, const double*, double*, double*);

#ifdef AMPC_T_IS_F64
extern template int kstep_impl<float>(ampc_handle* const*, int, int, const int*, int, const double*, const double*,
                                      const double*, int, const double*, double*, double*);

extern "C" int ampc_kstep_errors(ampc_handle* const* models, int n_models, int n_traj, const int* traj_len,
                                 int obs_dim, const double* obs, const double* ctrls, const double* init_states,
                                 int kmax, const double* inv_std, double* sq_err, double* sq_delta_err) {
  REQUIRE(models && n_models >= 1, "ampc_kstep_errors: no models");
  REQUIRE(n_traj >= 0 && (n_traj == 0 || traj_len), "ampc_kstep_errors: NULL trajectory lengths");
  REQUIRE(kmax >= 1, "ampc_kstep_errors: kmax must be >= 1");
  REQUIRE(sq_err, "ampc_kstep_errors: NULL sq_err");
  REQUIRE(!sq_delta_err || inv_std, "ampc_kstep_errors: sq_delta_err needs inv_std");
  ampc_handle* h = models[0];
  REQUIRE(h, "ampc_kstep_errors: NULL model handle");
  REQUIRE(!h->has_sindy && !h->has_lin && h->has_mlp,
          "ampc_kstep_errors: MLP models and linear models of at most 64 states only (SINDy and wide linear "
          "models are scored on the host)");
  for (int i = 0; i < n_models; ++i) {
    REQUIRE(models[i] && !models[i]->has_sindy && !models[i]->has_lin,
            "ampc_kstep_errors: MLP models and linear models of at most 64 states only");
    const int rc = check_same_shape(h, models[i], "ampc_kstep_errors");
    if (rc) return rc;
  }
  REQUIRE(obs_dim >= 1 && obs_dim <= h->nx, "ampc_kstep_errors: obs_dim must be in 1..state dim");
  REQUIRE(init_states || obs_dim == h->nx, "ampc_kstep_errors: a model whose state is not the observation needs init_states");
  long long total = 0;
  for (int i = 0; i < n_traj; ++i) {
    REQUIRE(traj_len[i] >= 0, "ampc_kstep_errors: negative trajectory length");
    total += traj_len[i];
  }
  REQUIRE(total == 0 || (obs && ctrls), "ampc_kstep_errors: NULL obs / ctrls");
  HIP_OK(hipSetDevice(h->device));
  return h->precision == AMPC_F64
             ? kstep_impl<double>(models, n_models, n_traj, traj_len, obs_dim, obs, ctrls, init_states, kmax, inv_std,
                                  sq_err, sq_delta_err)
             : kstep_impl<float>(models, n_models, n_traj, traj_len, obs_dim, obs, ctrls, init_states, kmax, inv_std,
                                 sq_err, sq_delta_err);
}
#endif
