// launch_kstep_linear.cpp -- ampc_kstep_errors_linear: k-step prediction error sums of wide linear models (65..256
// states, any mix of state dimensions) over recorded trajectories in ONE launch (kstep_linear_kernels.hpp).
// Compiled once per precision (-DAMPC_T=double|float, csrc/build.py); the f64 unit also carries the C entry, which
// checks the arguments and dispatches on the models' precision.
#include "host_common.hpp"
#include "kstep_linear_kernels.hpp"

#ifndef AMPC_T
#error "compile with -DAMPC_T=double or -DAMPC_T=float"
#endif

// what the C entry hands to the launcher: every model's state rule, checked
struct KstepLinRule {
  int rule = 0;
  std::vector<KstepLinCol> cols;     // rule 1
  std::vector<double> prog;          // rule 2
  const double* rows = nullptr;      // rule 0 (host pointer; nullptr: state = observation)
};

template <typename T>
int kstep_linear_impl(ampc_handle* const* models, int n_models, int n_traj, const int* traj_len, int obs_dim,
                      const double* obs, const double* ctrls, const std::vector<KstepLinRule>& rules, int kmax,
                      const double* inv_std, double* sq_err, double* sq_delta_err) {
  ampc_handle* h = models[0];
  for (int i = 1; i < n_models; ++i) HIP_OK(hipStreamSynchronize(models[i]->stream));   // (staging done)
  const int nu = h->nu;
  // start points: (trajectory i, t), t = 0 .. L_i - 2
  long long total = 0;
  std::vector<int> base, rem, start;
  for (int i = 0; i < n_traj; ++i) {
    for (int t = 0; t + 1 < traj_len[i]; ++t) {
      base.push_back((int)(total + t));
      rem.push_back(traj_len[i] - 1 - t);
      start.push_back((int)total);
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
  REQUIRE(total < (1LL << 31), "ampc_kstep_errors_linear: more than 2^31 trajectory rows");
  // (the tile height is 16 whatever the call holds, and every LDS offset is the model's own: a model's sums are
  //  the same bits alone or in a batch; only the reserved bytes follow the widest model)
  const int tiles = (n_rows + 15) / 16;
  size_t lds_bytes = 0;
  for (int i = 0; i < n_models; ++i)
    lds_bytes = std::max(lds_bytes, kstep_lin_lds_bytes(obs_dim, want_d, models[i]->l_kp, (int)sizeof(T)));
  REQUIRE(lds_bytes <= kLdsLimit,
          "ampc_kstep_errors_linear: the error blocks of this observation size do not fit LDS beside the widest "
          "model's operand buffers");
  REQUIRE((long long)tiles * n_models * kmax < (1LL << 31), "ampc_kstep_errors_linear: too many partial sums");

  ScopedBuf d_obs, d_ctrl, d_inv, d_base, d_rem, d_start, d_part, d_dpart, d_out, d_desc, d_cols, d_prog;
  std::vector<ScopedBuf> d_rows(n_models);
  HIP_OK(d_obs.reserve((size_t)total * obs_dim * 8));
  HIP_OK(d_ctrl.reserve((size_t)total * nu * 8));
  HIP_OK(d_base.reserve((size_t)n_rows * 4));
  HIP_OK(d_rem.reserve((size_t)n_rows * 4));
  HIP_OK(d_start.reserve((size_t)n_rows * 4));
  HIP_OK(d_part.reserve((size_t)n_models * tiles * kmax * 8));
  HIP_OK(d_out.reserve((size_t)2 * n_models * kmax * 8));
  HIP_OK(hipMemcpyAsync(d_obs.p, obs, (size_t)total * obs_dim * 8, hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipMemcpyAsync(d_ctrl.p, ctrls, (size_t)total * nu * 8, hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipMemcpyAsync(d_base.p, base.data(), (size_t)n_rows * 4, hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipMemcpyAsync(d_rem.p, rem.data(), (size_t)n_rows * 4, hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipMemcpyAsync(d_start.p, start.data(), (size_t)n_rows * 4, hipMemcpyHostToDevice, h->stream));
  if (want_d) {
    HIP_OK(d_dpart.reserve((size_t)n_models * tiles * kmax * 8));
    HIP_OK(d_inv.reserve((size_t)obs_dim * 8));
    HIP_OK(hipMemcpyAsync(d_inv.p, inv_std, (size_t)obs_dim * 8, hipMemcpyHostToDevice, h->stream));
  }
  // the rules' tables, concatenated, and the descriptor table
  std::vector<KstepLinCol> cols;
  std::vector<double> prog;
  std::vector<size_t> col_off(n_models, 0), prog_off(n_models, 0);
  for (int i = 0; i < n_models; ++i) {
    col_off[i] = cols.size();
    prog_off[i] = prog.size();
    cols.insert(cols.end(), rules[i].cols.begin(), rules[i].cols.end());
    prog.insert(prog.end(), rules[i].prog.begin(), rules[i].prog.end());
  }
  HIP_OK(d_cols.reserve(cols.size() * sizeof(KstepLinCol)));
  HIP_OK(d_prog.reserve(prog.size() * 8));
  if (!cols.empty())
    HIP_OK(hipMemcpyAsync(d_cols.p, cols.data(), cols.size() * sizeof(KstepLinCol), hipMemcpyHostToDevice, h->stream));
  if (!prog.empty()) HIP_OK(hipMemcpyAsync(d_prog.p, prog.data(), prog.size() * 8, hipMemcpyHostToDevice, h->stream));
  std::vector<KstepLinDesc> descs(n_models);
  for (int i = 0; i < n_models; ++i) {
    const LinDev<T> m = lin_of<T>(models[i]);
    KstepLinDesc& d = descs[i];
    d.nx = m.nx; d.nu = m.nu; d.kp = m.kp; d.ntile = m.ntile; d.ksn = m.ksn;
    d.rule = rules[i].rule;
    d.wf = m.wf;
    d.rows = nullptr;
    d.cols = (const KstepLinCol*)d_cols.p + col_off[i];
    d.prog = (const double*)d_prog.p + prog_off[i];
    if (rules[i].rule == 0 && rules[i].rows) {
      const size_t bytes = (size_t)total * m.nx * 8;
      HIP_OK(d_rows[i].reserve(bytes));
      HIP_OK(hipMemcpyAsync(d_rows[i].p, rules[i].rows, bytes, hipMemcpyHostToDevice, h->stream));
      d.rows = (const double*)d_rows[i].p;
    }
  }
  HIP_OK(d_desc.reserve(descs.size() * sizeof(KstepLinDesc)));
  HIP_OK(hipMemcpyAsync(d_desc.p, descs.data(), descs.size() * sizeof(KstepLinDesc), hipMemcpyHostToDevice, h->stream));

  KstepLinArgs a;
  a.obs = (const double*)d_obs.p; a.ctrls = (const double*)d_ctrl.p;
  a.inv_std = want_d ? (const double*)d_inv.p : nullptr;
  a.row_base = (const int*)d_base.p; a.row_rem = (const int*)d_rem.p; a.row_start = (const int*)d_start.p;
  a.part = (double*)d_part.p; a.dpart = want_d ? (double*)d_dpart.p : nullptr;
  a.n_rows = n_rows; a.tiles = tiles; a.kmax = kmax; a.obs_dim = obs_dim;
  HIP_OK(allow_lds(kstep_linear_kernel<T>, lds_bytes));
  // grid.y is limited to 65535 workgroups: more models than that go in slices of the same launch geometry
  for (int m0 = 0; m0 < n_models; m0 += 32768) {
    const int nm = std::min(32768, n_models - m0);
    KstepLinArgs as = a;
    as.part = a.part + (size_t)m0 * tiles * kmax;
    if (want_d) as.dpart = a.dpart + (size_t)m0 * tiles * kmax;
    hipLaunchKernelGGL(kstep_linear_kernel<T>, dim3(tiles, nm), dim3(64 * kLinW), lds_bytes, h->stream,
                       (const KstepLinDesc*)d_desc.p + m0, as);
  }
  HIP_OK(hipGetLastError());
  double* out = (double*)d_out.p;
  const int nr = n_models * kmax;
  hipLaunchKernelGGL(kstep_lin_reduce_kernel<T>, dim3((nr + 255) / 256), dim3(256), 0, h->stream,
                     (const double*)d_part.p, out, n_models, tiles, kmax);
  if (want_d)
    hipLaunchKernelGGL(kstep_lin_reduce_kernel<T>, dim3((nr + 255) / 256), dim3(256), 0, h->stream,
                       (const double*)d_dpart.p, out + nr, n_models, tiles, kmax);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(sq_err, out, (size_t)nr * 8, hipMemcpyDeviceToHost, h->stream));
  if (want_d) HIP_OK(hipMemcpyAsync(sq_delta_err, out + nr, (size_t)nr * 8, hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  return 0;
}

template int kstep_linear_impl<AMPC_T>(ampc_handle* const*, int, int, const int*, int, const double*, const double*,
                                       const std::vector<KstepLinRule>&, int, const double*, double*, double*);

#ifdef AMPC_T_IS_F64
extern template int kstep_linear_impl<float>(ampc_handle* const*, int, int, const int*, int, const double*,
                                             const double*, const std::vector<KstepLinRule>&, int, const double*,
                                             double*, double*);

extern "C" int ampc_kstep_errors_linear(ampc_handle* const* models, int n_models, int n_traj, const int* traj_len,
                                        int obs_dim, const double* obs, const double* ctrls, const int* rules,
                                        const int* arx_history, const int* n_basis, const int* lift_kinds,
                                        const double* lift_params, const double* const* init_rows, int kmax,
                                        const double* inv_std, double* sq_err, double* sq_delta_err) {
  REQUIRE(models && n_models >= 1, "ampc_kstep_errors_linear: no models");
  REQUIRE(rules, "ampc_kstep_errors_linear: NULL rules");
  REQUIRE(n_traj >= 0 && (n_traj == 0 || traj_len), "ampc_kstep_errors_linear: NULL trajectory lengths");
  REQUIRE(kmax >= 1, "ampc_kstep_errors_linear: kmax must be >= 1");
  REQUIRE(sq_err, "ampc_kstep_errors_linear: NULL sq_err");
  REQUIRE(!sq_delta_err || inv_std, "ampc_kstep_errors_linear: sq_delta_err needs inv_std");
  ampc_handle* h = models[0];
  REQUIRE(h, "ampc_kstep_errors_linear: NULL model handle");
  for (int i = 0; i < n_models; ++i) {
    const ampc_handle* m = models[i];
    REQUIRE(m, "ampc_kstep_errors_linear: NULL model handle");
    REQUIRE(m->has_lin && m->lin_n == m->nx,
            "ampc_kstep_errors_linear: wide linear models only (ampc_set_linear with 65..256 states; MLP models "
            "and linear models of at most 64 states are scored by ampc_kstep_errors)");
    REQUIRE(m->device == h->device && m->precision == h->precision,
            "ampc_kstep_errors_linear: models must share one device and one precision");
    REQUIRE(m->nu == h->nu, "ampc_kstep_errors_linear: models must share ctrl_dim");
    REQUIRE(obs_dim >= 1 && obs_dim <= m->nx, "ampc_kstep_errors_linear: obs_dim must be in 1..state dim of every model");
  }
  long long total = 0;
  for (int i = 0; i < n_traj; ++i) {
    REQUIRE(traj_len[i] >= 0, "ampc_kstep_errors_linear: negative trajectory length");
    total += traj_len[i];
  }
  REQUIRE(total == 0 || (obs && ctrls), "ampc_kstep_errors_linear: NULL obs / ctrls");
  const int no = obs_dim, nu = h->nu;
  std::vector<KstepLinRule> rl(n_models);
  for (int i = 0, pos = 0; i < n_models; ++i) {
    const int nx = models[i]->nx;
    KstepLinRule& r = rl[i];
    r.rule = rules[i];
    if (r.rule == 0) {
      r.rows = init_rows ? init_rows[i] : nullptr;
      REQUIRE(r.rows || nx == no,
              "ampc_kstep_errors_linear: a rule-0 model whose state is not the observation needs its init_rows");
    } else if (r.rule == 1) {
      REQUIRE(arx_history && arx_history[i] >= 1, "ampc_kstep_errors_linear: rule 1 needs an ARX history >= 1");
      const long long k = arx_history[i];
      REQUIRE(1 + k * (no + nu) - nu == nx,
              "ampc_kstep_errors_linear: the ARX state (1 + history (obs_dim + ctrl_dim) - ctrl_dim) does not have "
              "the handle's state dim");
      for (int j = 0; j < no; ++j) r.cols.push_back(KstepLinCol{1, 0, j});
      for (int lag = 1; lag < (int)k; ++lag) {
        for (int j = 0; j < no; ++j) r.cols.push_back(KstepLinCol{1, lag, j});
        for (int j = 0; j < nu; ++j) r.cols.push_back(KstepLinCol{2, lag, j});
      }
      r.cols.push_back(KstepLinCol{0, 0, 0});
    } else if (r.rule == 2) {
      REQUIRE(n_basis && lift_kinds && lift_params, "ampc_kstep_errors_linear: rule 2 needs the lift (n_basis, kinds, params)");
      const int nb = n_basis[i];
      REQUIRE(nb >= 1 && (long long)nb * no == nx,
              "ampc_kstep_errors_linear: the lift (n_basis * obs_dim) does not have the handle's state dim");
      for (int k = 0; k < nb; ++k, ++pos) {
        const int kind = lift_kinds[pos];
        const double par = lift_params[pos];
        REQUIRE(kind >= 0 && kind <= 3, "ampc_kstep_errors_linear: basis kind must be 0 identity, 1 power, 2 sin, 3 cos");
        REQUIRE(kind != 1 || (par >= 0 && par <= 64 && par == std::floor(par)),
                "ampc_kstep_errors_linear: powers must be integers in 0..64");
        r.prog.push_back(kind);
        r.prog.push_back(par);
      }
    } else {
      return fail("ampc_kstep_errors_linear: rules must be 0 (rows), 1 (ARX) or 2 (lift)");
    }
  }
  HIP_OK(hipSetDevice(h->device));
  return h->precision == AMPC_F64
             ? kstep_linear_impl<double>(models, n_models, n_traj, traj_len, obs_dim, obs, ctrls, rl, kmax, inv_std,
                                         sq_err, sq_delta_err)
             : kstep_linear_impl<float>(models, n_models, n_traj, traj_len, obs_dim, obs, ctrls, rl, kmax, inv_std,
                                        sq_err, sq_delta_err);
}
#endif
