// api_ilqr.cpp -- iLQR plans: batch solves, continuous batching (queue), device-resident iLQR episodes
// Part of the C ABI of libautompc_hip.so (include/autompc_hip.h); see api.cpp for the map of the translation units.
// Built with hipcc for gfx950 only.
#include "host_common.hpp"
#include <mutex>
#include "jit_host.hpp"                // shape plugins compiled at run time
#include "ilqr_table_host.hpp"         // ampc_ilqr_plan_set_model_table: checks and the LDS map without a device call
#include "ilqr_sindy_table_host.hpp"   // ampc_ilqr_plan_set_sindy_models: checks, the selection rule and the LDS maps
#include "ilqr_linear_table_host.hpp"  // ampc_ilqr_plan_set_linear_models: the second kernel argument, LDS maps, launchers

extern template int pred_impl<double>(ampc_handle*, const double*, const double*, double*, double*, double*, int);
extern template int pred_impl<float>(ampc_handle*, const double*, const double*, double*, double*, double*, int);
extern template int surrogate_step<double>(ampc_handle*, ampc_handle*, const void*, const void*, void*, int);
extern template int surrogate_step<float>(ampc_handle*, ampc_handle*, const void*, const void*, void*, int);
extern template int ilqr_refresh_jacobians<double>(ampc_ilqr_plan*);
extern template int ilqr_refresh_jacobians<float>(ampc_ilqr_plan*);
extern template int mppi_solve_impl<double>(ampc_mppi_plan*);
extern template int mppi_solve_impl<float>(ampc_mppi_plan*);
extern template int ilqr_launch_iter<double>(ampc_ilqr_plan*, int);
extern template int ilqr_launch_iter<float>(ampc_ilqr_plan*, int);

// Which line-search kernel the next launches of a many-problem plan take (ampc_ilqr_plan::ls_rb): the
// four-row kernel's launch lasts as many passes as its slowest search, the twelve-row kernel's about 2.4
// passes' time whatever the searches need -- twelve rows once some active slot's last search needed a
// third pass.  (A speed heuristic only: both kernels give the same results bit for bit.)
static int ls_rb_from_poll(const int* active, const int* need, int B) {
  int most = 0;
  for (int b = 0; b < B; ++b)
    if (active[b] != 0 && need[b] > most) most = need[b];
  return most >= 3 ? 3 : 1;
}

template <typename T> static int ilqr_plan_build(ampc_ilqr_plan* p) {
  ampc_handle* h = p->h;
  const MlpDev<T>& m = model_of<T>(h);
  const int nx = h->nx, nu = h->nu, B = p->B, H = p->H;
  const IlqrWork wk = make_ilqr_work(nx, nu, h->cost_stride, h->has_lin);
  p->prog_slots = 0;
  if (h->has_sindy) {
    std::memset(&p->L, 0, sizeof(p->L));
    p->L.xu = 0;
    p->L.xu_stride = nx + nu + 1;
    p->lds_xn = round_up(16 * p->L.xu_stride, 4);
    p->L.extra = round_up(p->lds_xn + 16 * nx + 16 * h->s_ntab, 4);   // xnext + table scratch
  } else if (h->has_prog) {        // [x | u] rows, the outputs' hand-over [16][nx], the forward program's slots [n_slots][16]
    std::memset(&p->L, 0, sizeof(p->L));
    p->L.xu = 0;
    p->L.xu_stride = nx + nu + 1;
    p->lds_xn = round_up(16 * p->L.xu_stride, 4);
    p->L.extra = round_up(p->lds_xn + 16 * nx + 16 * h->p_nslots, 4);
    p->prog_slots = h->p_nslots;
  } else if (h->has_lin) {         // line search: [x | u] rows for lin_tile, next states, compact work map
    std::memset(&p->L, 0, sizeof(p->L));
    p->L.xu = 0;
    p->L.xu_stride = lin_xs(h->l_kp, (int)sizeof(T));
    p->lds_xn = round_up(16 * p->L.xu_stride, 4);
    p->L.extra = round_up(p->lds_xn + 16 * nx, 4);
  } else {
    p->L = tile_lds_for<T>(h, m, 16, (size_t)wk.total + 8);
  }
  p->lds_work = p->L.extra;
  p->lds_bytes = ((size_t)p->lds_work + wk.total) * sizeof(T);
  // a program plan whose full map does not fit (the dense cost block and the sweep's matrices grow with nx^2): the line
  // search on the compact map -- it never touches the sweep's matrices -- and the sweep without its LDS copy of the
  // cost block.  Same results as the full map bit for bit; plans that fit the full map keep it.
  p->prog_compact = 0;
  size_t sweep_bytes = (size_t)wk.total * sizeof(T);
  if (h->has_prog && p->lds_bytes > kLdsLimit) {
    p->prog_compact = 1;
    p->lds_bytes = ((size_t)p->lds_work + make_ilqr_work(nx, nu, h->cost_stride, true).total) * sizeof(T);
    sweep_bytes = (size_t)make_ilqr_work(nx, nu, 0).total * sizeof(T);
  }
  p->use_ls4 = env_int("AMPC_LS4", 1) != 0;
  p->use_mfma_sweep = env_int("AMPC_RICCATI", 1) != 0;
  p->par_passes = env_int("AMPC_LS4_PAR", 1) != 0;
  p->ls_split = env_int("AMPC_LS4_SPLIT", 0) != 0;
  { const int rb = env_int("AMPC_LS4_RB", 0); p->ls_rb = (rb == 1 || rb == 3) ? rb : 0; }
  p->static_shape = -1;
  p->jit = nullptr;
  if (!h->has_sindy && !h->has_lin && !h->has_prog && env_int("AMPC_STATIC", 1) != 0) {
    int sid = static_shape_of<T>(h, m);
    if (sid < 0 && (p->jit = jit::get<T>(h)) != nullptr) sid = 0;      // run-time compiled shape
    if (sid >= 0) {
      const TileLds S = tile_lds_dims((int)sizeof(T), m.hpad, m.k1p, m.nxp, m.n_hidden, 16, h->nw, true, true);
      if (std::memcmp(&S, &p->L, sizeof(TileLds)) == 0) p->static_shape = sid;
    }
    if (p->static_shape < 0) p->jit = nullptr;
  }
  if (h->has_prog)
    REQUIRE(p->lds_bytes <= kLdsLimit && sweep_bytes <= kLdsLimit, "ilqr plan (" + std::to_string(h->p_nslots) + " program slots, " + std::to_string(nx) +
                                           " states)" + kProgIlqrLds);
  REQUIRE(p->lds_bytes <= kLdsLimit, "ilqr plan: model does not fit the 160 KB LDS");
  REQUIRE(sweep_bytes <= kLdsLimit,
          "ilqr plan: the Riccati workspace for this state dimension does not fit the 160 KB LDS");
  if (h->has_lin)
    REQUIRE((size_t)make_wide_lds(nx, nu, h->obs_dim).total * sizeof(T) <= kLdsLimit,
            "ilqr plan: the sweep's workspace for this state / observation dimension does not fit the 160 KB LDS");
  const size_t e = sizeof(T);
  HIP_OK(p->d_cost_idx.reserve(B * sizeof(int)));
  // (initialisation goes through the plan's OWN stream: the handle's stream is non-blocking, so work on the null
  //  stream -- shared by every host thread -- is not ordered against the plan's kernels and may land behind them)
  HIP_OK(hipMemcpyAsync(p->d_cost_idx.p, p->cost_idx.data(), B * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIP_OK(p->states.reserve((size_t)B * (H + 1) * nx * e));
  HIP_OK(p->ctrls.reserve((size_t)B * H * nu * e));
  if (!h->has_lin) {              // (a linear model's Jacobians are the constant [A | B]: LinDev::jp)
    HIP_OK(p->jx.reserve((size_t)B * H * nx * nx * e));
    HIP_OK(p->ju.reserve((size_t)B * H * nx * nu * e));
  } else {
    HIP_OK(p->vj.reserve((size_t)B * h->l_nxp * round_up(nx + nu, 16) * e));
  }
  HIP_OK(p->Ks.reserve((size_t)B * H * nu * nx * e));
  HIP_OK(p->ks.reserve((size_t)B * H * nu * e));
  HIP_OK(hipMemsetAsync(p->Ks.p, 0, (size_t)B * H * nu * nx * e, h->stream));
  HIP_OK(hipMemsetAsync(p->ks.p, 0, (size_t)B * H * nu * e, h->stream));
  HIP_OK(p->ls_states.reserve((size_t)B * p->ls_n * (H + 1) * nx * e));
  HIP_OK(p->ls_ctrls.reserve((size_t)B * p->ls_n * H * nu * e));
  HIP_OK(p->obj.reserve((size_t)B * e));
  HIP_OK(p->flags.reserve((size_t)9 * B * sizeof(int)));
  HIP_OK(hipMemsetAsync(p->flags.p, 0, (size_t)9 * B * sizeof(int), h->stream));
  const int rows = B * H;
  const int n_pad = round_up(rows, 64);
  if (!h->has_sindy && !h->has_lin && !h->has_prog) HIP_OK(p->dz.reserve((size_t)m.n_hidden * n_pad * m.hpad * e));
  HIP_OK(p->ric.reserve((size_t)kRicStride * p->B * e));
  HIP_OK(hipStreamSynchronize(h->stream));
  return 0;
}

extern "C" int ampc_ilqr_plan_create(ampc_handle* h, int B, int horizon, double dt,
                                     const int* cost_index, int clip_to_bounds,
                                     ampc_ilqr_plan** out) {
  REQUIRE(h && out, "ampc_ilqr_plan_create: NULL argument");
  REQUIRE(!h->has_prog || (h->has_jvp && h->prog_ilqr), std::string("ampc_ilqr_plan_create") + kProgNoPlan);
  if (h->has_prog) {     // the opt-in (ampc_program_set_ilqr): the sixteen-row line search on the interpreter, f64
    REQUIRE(h->precision == AMPC_F64, "ampc_ilqr_plan_create: iLQR on an analytic dynamics program is built for f64 "
                                      "handles; this program's handle is f32");
    REQUIRE(h->n_costs == 0 || h->obs_dim == h->nx,
            "ampc_ilqr_plan_create: the program's state is the observation: the cost blocks must be on nx observations");
  }
  if (h->has_lin) {      // wide linear models: ilqr_wide.hpp (V [nx][nx] in LDS, per-thread Quu solves)
    REQUIRE(h->nx <= kLinMaxIlqrNx, "ampc_ilqr_plan_create: iLQR on wide linear models takes up to 128 model states (the "
                                    "value function's Hessian lives in LDS); larger ones run MPPI and the closed loop");
    REQUIRE(h->nu == 1 || h->nu == 2 || h->nu == 3 || h->nu == 4 || h->nu == 6 || h->nu == 8,
            "ampc_ilqr_plan_create: iLQR on wide linear models is built for 1, 2, 3, 4, 6 or 8 controls");
  } else {
    REQUIRE(h->nx + h->nu + 1 <= 64,
            "ampc_ilqr_plan_create: state dim + ctrl dim must be <= 63 (one wave holds the augmented Quu system)");
  }
  REQUIRE(h->has_model() && h->n_costs > 0, "ampc_ilqr_plan_create: model and cost must be set first");
  REQUIRE(h->n_ind == 0, "ampc_ilqr_plan_create: the handle's cost has indicator terms (threshold / box): they have no "
                         "gradient or Hessian, iLQR takes sums of quadratic costs only");
  REQUIRE(B >= 1 && horizon >= 1, "ampc_ilqr_plan_create: B >= 1 and horizon >= 1 required");
  REQUIRE(!clip_to_bounds || h->has_bounds, "ampc_ilqr_plan_create: bounds requested but not set");
  HIP_OK(hipSetDevice(h->device));
  ampc_ilqr_plan* p = new ampc_ilqr_plan();
  h->refs++;
  p->h = h; p->B = B; p->H = horizon; p->dt = dt; p->bounded = clip_to_bounds ? 1 : 0;
  for (int b = 0; b < B; ++b) {
    const int ci = cost_index ? cost_index[b] : 0;
    if (ci < 0 || ci >= h->n_costs) { h->refs--; delete p; return fail("ampc_ilqr_plan_create: bad cost_index"); }
    p->cost_idx.push_back(ci);
  }
  int rc = h->precision == AMPC_F64 ? ilqr_plan_build<double>(p) : ilqr_plan_build<float>(p);
  if (rc) { ampc_ilqr_plan_destroy(p); return rc; }
  *out = p;
  return 0;
}

extern "C" int ampc_ilqr_plan_set_constants(ampc_ilqr_plan* p, double u_threshold, int ls_max_iter, double ls_discount,
                                            double ls_cost_threshold) {
  REQUIRE(p, "ampc_ilqr_plan_set_constants: NULL plan");
  REQUIRE(ls_max_iter >= 1 && ls_max_iter <= kIlqrMaxLs, "ampc_ilqr_plan_set_constants: 1..16 line-search step sizes");
  REQUIRE(u_threshold >= 0.0 && ls_discount > 0.0, "ampc_ilqr_plan_set_constants: u_threshold >= 0 and ls_discount > 0");
  ampc_handle* h = p->h;
  HIP_OK(hipSetDevice(h->device));
  HIP_OK(hipStreamSynchronize(h->stream));            // the candidate buffers below may be re-allocated
  p->u_threshold = u_threshold;
  p->ls_discount = ls_discount;
  p->ls_cost_threshold = ls_cost_threshold;
  p->ls_n = ls_max_iter;
  const size_t e = h->esz();
  const int nxs = std::max(h->nx, p->lqt_nxw);        // (a table of linear models: the widest entry's stride)
  HIP_OK(p->ls_states.reserve((size_t)p->B * p->ls_n * (p->H + 1) * nxs * e));
  HIP_OK(p->ls_ctrls.reserve((size_t)p->B * p->ls_n * p->H * h->nu * e));
  return 0;
}

extern "C" int ampc_ilqr_plan_set_timing(ampc_ilqr_plan* p, int enable) {
  REQUIRE(p, "ampc_ilqr_plan_set_timing: NULL plan");
  p->timing = enable != 0;
  p->timing_stride = enable > 1 ? enable : 1;      // (queue: enable = n > 1 brackets every n-th iteration)
  p->ev_used = 0;
  return 0;
}

extern "C" int ampc_ilqr_plan_timing(ampc_ilqr_plan* p, double* kernel_ms, int* iterations) {
  REQUIRE(p && kernel_ms, "ampc_ilqr_plan_timing: NULL argument");
  HIP_OK(hipSetDevice(p->h->device));
  HIP_OK(hipStreamSynchronize(p->h->stream));
  double acc[4] = {0, 0, 0, 0};
  const size_t n = p->ev_used / 5;
  size_t live = 0;
  for (size_t i = 0; i < n; ++i) {
    if (i < p->ev_live.size() && !p->ev_live[i]) continue;     // queued past convergence: a no-op
    ++live;
    for (int k = 0; k < 4; ++k) {
      float ms = 0;
      HIP_OK(hipEventElapsedTime(&ms, p->ev[5 * i + k], p->ev[5 * i + k + 1]));
      acc[k] += ms;
    }
  }
  for (int k = 0; k < 4; ++k) kernel_ms[k] = live ? acc[k] / live : 0.0;
  if (iterations) *iterations = (int)live;
  p->ev_used = 0;
  p->ev_live.clear();
  return 0;
}

extern "C" int ampc_ilqr_plan_stats(ampc_ilqr_plan* p, long long* iterations, long long* candidate_rows) {
  REQUIRE(p, "ampc_ilqr_plan_stats: NULL plan");
  if (iterations) *iterations = p->last_effective;     // performed (launched: last_iterations)
  if (candidate_rows) *candidate_rows = p->last_ls_rows;
  return 0;
}

extern "C" int ampc_ilqr_plan_set_terminal_goal(ampc_ilqr_plan* p, int use_goal) {
  REQUIRE(p, "ampc_ilqr_plan_set_terminal_goal: NULL plan");
  p->term_goal = use_goal ? 1 : 0;
  return 0;
}

extern "C" int ampc_ilqr_plan_jacobians(ampc_ilqr_plan* p, double* jx, double* ju, int write) {
  REQUIRE(p && jx && ju, "ampc_ilqr_plan_jacobians: NULL argument");
  ampc_handle* h = p->h;
  REQUIRE(!h->has_lin && p->table_n == 0 && p->sindy_n == 0 && p->lqt_n == 0 && p->jx.p && p->ju.p,
          "ampc_ilqr_plan_jacobians: the plan keeps no per-row Jacobians of its handle's model (a linear model's are "
          "constant; a model table keeps its own)");
  HIP_OK(hipSetDevice(h->device));
  HIP_OK(hipStreamSynchronize(h->stream));
  const size_t rows = (size_t)p->B * p->H, nx = h->nx, nu = h->nu;
  if (h->precision == AMPC_F64) {
    if (write) {
      HIP_OK(upload_converted<double>(p->jx.p, jx, rows * nx * nx, h->stream));
      HIP_OK(upload_converted<double>(p->ju.p, ju, rows * nx * nu, h->stream));
      HIP_OK(hipStreamSynchronize(h->stream));
    } else {
      HIP_OK(download_converted<double>(jx, p->jx.p, rows * nx * nx, h->stream));
      HIP_OK(download_converted<double>(ju, p->ju.p, rows * nx * nu, h->stream));
    }
  } else {
    if (write) {
      HIP_OK(upload_converted<float>(p->jx.p, jx, rows * nx * nx, h->stream));
      HIP_OK(upload_converted<float>(p->ju.p, ju, rows * nx * nu, h->stream));
    } else {
      HIP_OK(download_converted<float>(jx, p->jx.p, rows * nx * nx, h->stream));
      HIP_OK(download_converted<float>(ju, p->ju.p, rows * nx * nu, h->stream));
    }
  }
  return 0;
}

extern "C" int ampc_ilqr_plan_destroy(ampc_ilqr_plan* p) {
  if (!p) return 0;
  (void)hipSetDevice(p->h->device);
  (void)hipStreamSynchronize(p->h->stream);
  DevBuf* bufs[] = {&p->d_cost_idx, &p->states, &p->ctrls, &p->jx, &p->ju, &p->Ks, &p->ks,
                    &p->ls_states, &p->ls_ctrls, &p->obj, &p->flags, &p->dz, &p->ric,
                    &p->q_ctl, &p->q_x0, &p->q_u, &p->q_cost, &p->q_states, &p->q_ctrls, &p->q_Ks, &p->q_ks,
                    &p->q_obj, &p->q_flags, &p->c_ints, &p->c_iters, &p->c_stage, &p->c_obs, &p->c_ctl, &p->slot_h, &p->vj};
  for (DevBuf* b : bufs) b->release();
  p->mlp_tab.release(); p->slot_model.release(); p->slot_of.release();
  p->table_models.release(); p->table_stage.release(); p->table_dz.release();
  p->sindy_tab.release();
  p->lqt_buf.release(); p->lqt_tab.release(); p->lqt_rules.release(); p->lqt_prog.release(); p->lqt_xoff.release();
  p->lqt_sim.release(); p->lqt_desc.release();
  for (ampc_handle* mh : p->lqt_models) handle_release(mh);
  for (ampc_handle* mh : p->sindy_models) handle_release(mh);
  for (ampc_handle* mh : p->models) handle_release(mh);
  for (hipEvent_t e : p->ev) (void)hipEventDestroy(e);
  if (p->poll_host) (void)hipHostFree(p->poll_host);
  for (hipEvent_t e : p->poll_ev) if (e) (void)hipEventDestroy(e);
  ampc_handle* h = p->h;
  delete p;
  handle_release(h);
  return 0;
}

template <typename T>
static int ilqr_solve_impl(ampc_ilqr_plan* p, const double* x0, const double* uguess, int max_iter,
                           double* states, double* ctrls, double* Ks, double* ks, int* converged,
                           int* iters, int* status, double* objective) {
  ampc_handle* h = p->h;
  const int nx = h->nx, nu = h->nu, B = p->B, H = p->H;
  // states[:, 0, :] = x0 ; ctrls = uguess
  std::vector<double> st((size_t)B * (H + 1) * nx, 0.0);
  for (int b = 0; b < B; ++b) std::memcpy(&st[(size_t)b * (H + 1) * nx], x0 + (size_t)b * nx, nx * 8);
  HIP_OK(upload_converted<T>(p->states.p, st.data(), st.size(), h->stream));
  HIP_OK(upload_converted<T>(p->ctrls.p, uguess, (size_t)B * H * nu, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  if (int rc = ilqr_launch_iter<T>(p, 0)) return rc;        // rollout of the guess + objective
  if (int rc = ilqr_refresh_jacobians<T>(p)) return rc;
  std::vector<int> flags(7 * B);
  HIP_OK(hipMemsetAsync((int*)p->flags.p + 5 * B, 0, (size_t)4 * B * sizeof(int), h->stream));   // ls_rows, ls_count, ls_pass, ls_need
  p->ls_rb_now = 1;
  if (!p->poll_host) HIP_OK(hipHostMalloc((void**)&p->poll_host, (size_t)4 * B * sizeof(int), hipHostMallocDefault));
  if (!p->poll_ev[0])
    for (int i = 0; i < 2; ++i) HIP_OK(hipEventCreateWithFlags(&p->poll_ev[i], hipEventDisableTiming));
  // Iterations are queued in batches of kPoll; the `active` flags of a batch are copied out behind
  // it and inspected only after the NEXT batch has been queued, so the stream never drains while the
  // host decides.  Iterations queued past convergence are no-ops (retired problems exit at once).
  constexpr int kPoll = 4;
  int it = 0, batch = 0, pending = -1;     // pending: batch whose flags are in flight
  bool done = false;
  p->active_hint = B;
  // (ev_cur points into p->ev: never leave it set behind an early return)
  struct EvGuard { ampc_ilqr_plan* p; ~EvGuard() { p->ev_cur = nullptr; } } ev_guard{p};
  const size_t ev_first = p->ev_used / 5;  // this solve's first timed iteration
  while (it < max_iter && !done) {
    const int n = std::min(kPoll, max_iter - it);
    for (int k = 0; k < n; ++k) {
      if (p->timing) {
        if (p->ev_used + 5 > p->ev.size())
          for (int i = 0; i < 5; ++i) {
            hipEvent_t x;
            HIP_OK(hipEventCreate(&x));
            p->ev.push_back(x);
          }
        p->ev_cur = &p->ev[p->ev_used];
        p->ev_used += 5;
      }
      int rc = ilqr_launch_iter<T>(p, 1);                     // backward sweep + line search + accept
      if (rc == 0) rc = ilqr_refresh_jacobians<T>(p);
      p->ev_cur = nullptr;
      if (rc) { (void)hipStreamSynchronize(h->stream); return rc; }
    }
    it += n;
    const int slot = batch & 1;
    HIP_OK(hipMemcpyAsync(p->poll_host + (size_t)slot * 2 * B, (const int*)p->flags.p + B, (size_t)B * sizeof(int),
                          hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipMemcpyAsync(p->poll_host + (size_t)slot * 2 * B + B, (const int*)p->flags.p + 8 * B,
                          (size_t)B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipEventRecord(p->poll_ev[slot], h->stream));
    if (pending >= 0) {
      const int ps = pending & 1;
      HIP_OK(hipEventSynchronize(p->poll_ev[ps]));
      const int* pa = p->poll_host + (size_t)ps * 2 * B;
      int live = 0;
      for (int b = 0; b < B; ++b) live += pa[b] != 0;
      p->ls_rb_now = ls_rb_from_poll(pa, pa + B, B);
      p->active_hint = live;          // (as of two batches ago: an upper bound of the current count)
      if (live == 0) done = true;
    }
    pending = batch++;
  }
  p->last_iterations = it;
  HIP_OK(hipMemcpyAsync(flags.data(), p->flags.p, flags.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  if (converged) std::memcpy(converged, flags.data(), B * sizeof(int));
  if (iters) std::memcpy(iters, flags.data() + 2 * B, B * sizeof(int));
  if (status) std::memcpy(status, flags.data() + 3 * B, B * sizeof(int));
  p->last_ls_rows = 0;
  for (int b = 0; b < B; ++b) p->last_ls_rows += flags[5 * B + b];
  p->last_effective = 0;
  for (int b = 0; b < B; ++b) p->last_effective = std::max(p->last_effective, flags[2 * B + b]);
  if (p->timing) {           // iterations past the last one any problem performed were no-ops
    p->ev_live.resize(p->ev_used / 5, 1);
    for (size_t i = ev_first + (size_t)p->last_effective; i < p->ev_live.size(); ++i) p->ev_live[i] = 0;
  }
  if (states) HIP_OK(download_converted<T>(states, p->states.p, (size_t)B * (H + 1) * nx, h->stream));
  if (ctrls) HIP_OK(download_converted<T>(ctrls, p->ctrls.p, (size_t)B * H * nu, h->stream));
  if (Ks) HIP_OK(download_converted<T>(Ks, p->Ks.p, (size_t)B * H * nu * nx, h->stream));
  if (ks) HIP_OK(download_converted<T>(ks, p->ks.p, (size_t)B * H * nu, h->stream));
  if (objective) HIP_OK(download_converted<T>(objective, p->obj.p, (size_t)B, h->stream));
  return 0;
}

extern "C" int ampc_ilqr_solve(ampc_ilqr_plan* p, const double* x0, const double* uguess,
                               int max_iter, double* states, double* ctrls, double* Ks, double* ks,
                               int* converged, int* iters, int* status, double* objective) {
  REQUIRE(p && x0 && uguess, "ampc_ilqr_solve: NULL argument");
  REQUIRE(max_iter >= 0, "ampc_ilqr_solve: max_iter < 0");
  if (int rc = ilqr_program_plan_check(p, "ampc_ilqr_solve")) return rc;
  REQUIRE(p->lqt_n == 0, "ampc_ilqr_solve: the plan holds a table of linear models (ampc_ilqr_plan_set_linear_models), whose "
                         "problems name their model: use ampc_ilqr_solve_queue_var");
  HIP_OK(hipSetDevice(p->h->device));
  return p->h->precision == AMPC_F64
             ? ilqr_solve_impl<double>(p, x0, uguess, max_iter, states, ctrls, Ks, ks, converged, iters, status, objective)
             : ilqr_solve_impl<float>(p, x0, uguess, max_iter, states, ctrls, Ks, ks, converged, iters, status, objective);
}

// ---------------------------------------------------------------------------------------------
// More slots than CUs (a finite batch admitted at once, or a wide evaluator plan): the kernels of an iteration
// take their slot through ilqr_slot_of -- the slots with work first -- rebuilt by one small launch per iteration.
// MLP models only (the feature-library and wide-linear kernels keep workgroup b = slot b).
static bool ilqr_wants_compaction(const ampc_ilqr_plan* p) {
  const int force = env_int("AMPC_ILQR_COMPACT", -1);
  if (force == 0 || !p->h->has_mlp || p->h->has_sindy || p->h->has_lin || p->lqt_n > 0) return false;
  return force == 1 || p->B > p->h->n_cus;
}
template <typename T> static int ilqr_compact(ampc_ilqr_plan* p) {
  if (!p->compact_on) return 0;
  IlqrArgs<T> a = make_ilqr_args<T>(p, 1);
  hipLaunchKernelGGL(ilqr_compact_kernel<T>, dim3(1), dim3(256), 0, p->h->stream, a, p->B, (int*)p->slot_of.p);
  HIP_OK(hipGetLastError());
  return 0;
}

// Continuous batching: P problems through the plan's B slots (ilqr_queue_refill_kernel)
// ---------------------------------------------------------------------------------------------
template <typename T>
static int ilqr_solve_queue_impl(ampc_ilqr_plan* p, int P, const double* x0, const double* uguess,
                                 const int* cost_index, const int* horizon, const int* model_index, int max_iter,
                                 double* states, double* ctrls, double* Ks, double* ks, int* converged, int* iters,
                                 int* status, double* objective) {
  ampc_handle* h = p->h;
  // a table of linear models (ampc_ilqr_plan_set_linear_models): nx is the widest entry's -- the stride of every region --
  // and x0 is ragged, problem j's own nx values at x_off[j]
  const bool lt = p->lqt_n > 0;
  const int nx = lt ? p->lqt_nxw : h->nx, nu = h->nu, B = p->B, H = p->H;
  const size_t e = sizeof(T);
  std::vector<int> x_off;
  size_t x0_elems = (size_t)P * nx;
  if (lt) {
    x_off.resize(P);
    x0_elems = 0;
    for (int j = 0; j < P; ++j) { x_off[j] = (int)x0_elems; x0_elems += p->lqt_nx[model_index ? model_index[j] : 0]; }
    REQUIRE(x0_elems < ((size_t)1 << 31), "ampc_ilqr_solve_queue_var: too many states in x0");
  }
  HIP_OK(p->q_ctl.reserve((size_t)(2 + 2 * B) * sizeof(int)));
  HIP_OK(p->q_x0.reserve(x0_elems * e));
  HIP_OK(p->q_u.reserve((size_t)P * H * nu * e));
  HIP_OK(p->q_cost.reserve((size_t)4 * P * sizeof(int)));               // cost block [P], horizon [P], model [P], x_off [P]
  HIP_OK(p->q_states.reserve((size_t)P * (H + 1) * nx * e));
  HIP_OK(p->q_ctrls.reserve((size_t)P * H * nu * e));
  HIP_OK(p->q_Ks.reserve((size_t)P * H * nu * nx * e));
  HIP_OK(p->q_ks.reserve((size_t)P * H * nu * e));
  HIP_OK(p->q_obj.reserve((size_t)P * e));
  HIP_OK(p->q_flags.reserve((size_t)4 * P * sizeof(int)));
  std::vector<int> ctl(2 + 2 * B, 0), cost(P, 0);
  for (int b = 0; b < B; ++b) { ctl[2 + b] = -1; ctl[2 + B + b] = 1; }       // no problem; mode "iterate"
  if (cost_index) std::memcpy(cost.data(), cost_index, (size_t)P * sizeof(int));
  HIP_OK(hipMemcpyAsync(p->q_ctl.p, ctl.data(), ctl.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipMemcpyAsync(p->q_cost.p, cost.data(), (size_t)P * sizeof(int), hipMemcpyHostToDevice, h->stream));
  std::vector<int> slot_h0;
  if (horizon) {
    slot_h0.assign(B, H);
    HIP_OK(p->slot_h.reserve((size_t)B * sizeof(int)));
    HIP_OK(hipMemcpyAsync(p->slot_h.p, slot_h0.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIP_OK(hipMemcpyAsync((int*)p->q_cost.p + P, horizon, (size_t)P * sizeof(int), hipMemcpyHostToDevice, h->stream));
  }
  if (model_index || lt) {
    HIP_OK(p->slot_model.reserve((size_t)B * sizeof(int)));
    HIP_OK(hipMemsetAsync(p->slot_model.p, 0, (size_t)B * sizeof(int), h->stream));
    if (model_index)
      HIP_OK(hipMemcpyAsync((int*)p->q_cost.p + 2 * P, model_index, (size_t)P * sizeof(int), hipMemcpyHostToDevice, h->stream));
    else
      HIP_OK(hipMemsetAsync((int*)p->q_cost.p + 2 * P, 0, (size_t)P * sizeof(int), h->stream));
  }
  if (lt) HIP_OK(hipMemcpyAsync((int*)p->q_cost.p + 3 * P, x_off.data(), (size_t)P * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIP_OK(upload_converted<T>(p->q_x0.p, x0, x0_elems, h->stream));
  if (uguess) HIP_OK(upload_converted<T>(p->q_u.p, uguess, (size_t)P * H * nu, h->stream));
  else HIP_OK(hipMemsetAsync(p->q_u.p, 0, (size_t)P * H * nu * e, h->stream));
  HIP_OK(hipMemsetAsync(p->flags.p, 0, (size_t)9 * B * sizeof(int), h->stream));     // every slot idle
  HIP_OK(hipMemsetAsync(p->states.p, 0, (size_t)B * (H + 1) * nx * e, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  const int npoll = 2 * B + 2;               // active[B], ls_need[B], the queue's two counters
  p->ls_rb_now = 1;
  if (p->poll_host) { (void)hipHostFree(p->poll_host); p->poll_host = nullptr; }
  HIP_OK(hipHostMalloc((void**)&p->poll_host, (size_t)2 * npoll * sizeof(int), hipHostMallocDefault));
  if (!p->poll_ev[0])
    for (int i = 0; i < 2; ++i) HIP_OK(hipEventCreateWithFlags(&p->poll_ev[i], hipEventDisableTiming));
  struct Guard {
    ampc_ilqr_plan* p;
    // (every exit path: no copy into the pinned poll buffer may still be in flight when it is freed, and
    //  the slots' cost blocks are the plan's own again, as ampc_ilqr_solve expects them)
    ~Guard() {
      (void)hipStreamSynchronize(p->h->stream);
      (void)hipMemcpyAsync(p->d_cost_idx.p, p->cost_idx.data(), (size_t)p->B * sizeof(int), hipMemcpyHostToDevice,
                           p->h->stream);
      (void)hipStreamSynchronize(p->h->stream);
      p->queue_on = false; p->var_h = false; p->var_model = false; p->compact_on = false; p->ev_cur = nullptr;
      (void)hipHostFree(p->poll_host); p->poll_host = nullptr;
    }
  } guard{p};
  p->queue_on = true;
  p->var_h = horizon != nullptr;
  p->var_model = model_index != nullptr;
  p->queue_max_iter = max_iter;
  p->active_hint = B;
  p->compact_on = ilqr_wants_compaction(p);
  if (p->compact_on) HIP_OK(p->slot_of.reserve((size_t)(B + 1) * sizeof(int)));
  IlqrQueue<T> q;
  q.P = P; q.B = B; q.H = H; q.nx = nx; q.nu = nu;
  q.horizon = horizon ? (const int*)p->q_cost.p + P : nullptr; q.slot_h = (int*)p->slot_h.p;
  q.model = (model_index || lt) ? (const int*)p->q_cost.p + 2 * P : nullptr; q.slot_model = (int*)p->slot_model.p;
  q.ctl = (int*)p->q_ctl.p; q.slot_prob = q.ctl + 2;
  q.x0 = (const T*)p->q_x0.p; q.uguess = (const T*)p->q_u.p; q.cost = (const int*)p->q_cost.p;
  q.cost_idx = (int*)p->d_cost_idx.p;
  q.out_states = (T*)p->q_states.p; q.out_ctrls = (T*)p->q_ctrls.p; q.out_Ks = (T*)p->q_Ks.p;
  q.out_ks = (T*)p->q_ks.p; q.out_obj = (T*)p->q_obj.p; q.out_flags = (int*)p->q_flags.p;
  // An iteration = refill + sweep + line search (or the guess's rollout, per slot) + Jacobian refresh.
  // The queue's counters and the slots' `active` flags are copied out behind every batch of kPoll
  // iterations and read after the NEXT batch has been queued (the stream never drains); everything
  // is done when P problems have been harvested.  Upper bound on the iterations: every problem takes
  // at most max_iter + 1 slot-iterations (+1: the rollout of its guess).
  constexpr int kPoll = 4;
  const long long bound = ((long long)(P + B - 1) / B) * (max_iter + 2LL) + (long long)P + 4 * kPoll;
  long long it = 0;
  int batch = 0, pending = -1;
  bool done = false;
  const size_t ev_first = p->ev_used / 5;
  int poll_now = kPoll;                      // (2 once every problem has been handed out and the grids follow the
  while (!done && it < bound) {             //  count of slots with work, compact_on: the count is then 4 iterations old)
    for (int k = 0; k < poll_now; ++k) {
      IlqrArgs<T> a = make_ilqr_args<T>(p, 1);
      if (lt) {
        if (int rc = ilqr_linear_table_refill(p, &a, &q, (const int*)p->q_cost.p + 3 * P)) return rc;
      } else {
        hipLaunchKernelGGL(ilqr_queue_refill_kernel<T>, dim3(B), dim3(256), 0, h->stream, a, q);
        HIP_OK(hipGetLastError());
      }
      if (int rc = ilqr_compact<T>(p)) return rc;
      if (p->timing && (it + k) % p->timing_stride == 0) {
        if (p->ev_used + 5 > p->ev.size())
          for (int i = 0; i < 5; ++i) {
            hipEvent_t x;
            HIP_OK(hipEventCreate(&x));
            p->ev.push_back(x);
          }
        p->ev_cur = &p->ev[p->ev_used];
        p->ev_used += 5;
      }
      int rc = ilqr_launch_iter<T>(p, 1);
      if (rc == 0) rc = ilqr_refresh_jacobians<T>(p);
      p->ev_cur = nullptr;
      if (rc) { (void)hipStreamSynchronize(h->stream); return rc; }
    }
    it += poll_now;
    const int slot = batch & 1;
    int* ph = p->poll_host + (size_t)slot * npoll;
    HIP_OK(hipMemcpyAsync(ph, (const int*)p->flags.p + B, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipMemcpyAsync(ph + B, (const int*)p->flags.p + 8 * B, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipMemcpyAsync(ph + 2 * B, p->q_ctl.p, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipEventRecord(p->poll_ev[slot], h->stream));
    if (pending >= 0) {
      const int* pp = p->poll_host + (size_t)(pending & 1) * npoll;
      HIP_OK(hipEventSynchronize(p->poll_ev[pending & 1]));
      int live = 0;
      for (int b = 0; b < B; ++b) live += pp[b] != 0;
      p->ls_rb_now = ls_rb_from_poll(pp, pp + B, B);
      // while the queue still holds problems every slot is (about to be) busy
      p->active_hint = pp[2 * B] < P ? B : std::max(live, 1);
      if (p->compact_on && pp[2 * B] >= P) poll_now = 2;
      if (pp[2 * B + 1] >= P) done = true;
    }
    pending = batch++;
  }
  HIP_OK(hipStreamSynchronize(h->stream));
  p->last_queue_launches = it;
  p->last_iterations = (int)std::min<long long>(it, 1 << 30);
  int fin[2] = {0, 0};
  HIP_OK(hipMemcpy(fin, p->q_ctl.p, sizeof(fin), hipMemcpyDeviceToHost));
  if (fin[1] < P) return fail("ampc_ilqr_solve_queue: internal: the queue did not drain");
  std::vector<int> fl((size_t)4 * P);
  HIP_OK(hipMemcpy(fl.data(), p->q_flags.p, fl.size() * sizeof(int), hipMemcpyDeviceToHost));
  p->last_ls_rows = 0;
  p->last_effective = (int)std::min<long long>(it, 1 << 30);
  for (int j = 0; j < P; ++j) {
    if (converged) converged[j] = fl[4 * j];
    if (iters) iters[j] = fl[4 * j + 1];
    if (status) status[j] = fl[4 * j + 2];
    p->last_ls_rows += fl[4 * j + 3];
  }
  if (p->timing) p->ev_live.resize(p->ev_used / 5, 1);
  (void)ev_first;
  if (states) HIP_OK(download_converted<T>(states, p->q_states.p, (size_t)P * (H + 1) * nx, h->stream));
  if (ctrls) HIP_OK(download_converted<T>(ctrls, p->q_ctrls.p, (size_t)P * H * nu, h->stream));
  if (Ks) HIP_OK(download_converted<T>(Ks, p->q_Ks.p, (size_t)P * H * nu * nx, h->stream));
  if (ks) HIP_OK(download_converted<T>(ks, p->q_ks.p, (size_t)P * H * nu, h->stream));
  if (objective) HIP_OK(download_converted<T>(objective, p->q_obj.p, (size_t)P, h->stream));
  return 0;      // (Guard: the slots' cost blocks as given at plan creation)
}

static int check_horizons(const ampc_ilqr_plan* p, int n, const int* horizon, const char* who) {
  if (horizon)
    for (int j = 0; j < n; ++j)
      REQUIRE(horizon[j] >= 1 && horizon[j] <= p->H, std::string(who) + ": horizons must lie in [1, the plan's horizon]");
  return 0;
}

static int check_models(const ampc_ilqr_plan* p, int n, const int* model_index, const char* who) {
  if (model_index) {
    REQUIRE(p->prog_slots == 0, std::string(who) + ": model_index given" + kProgIlqrNoTable);
    REQUIRE(!p->models.empty() || p->table_n > 0 || p->sindy_n > 0 || p->lqt_n > 0,
            std::string(who) + ": model_index given but the plan has no model table (ampc_ilqr_plan_set_models)");
    const int n_models = p->table_n > 0 ? p->table_n : p->sindy_n > 0 ? p->sindy_n : p->lqt_n > 0 ? p->lqt_n : (int)p->models.size();
    for (int j = 0; j < n; ++j)
      REQUIRE(model_index[j] >= 0 && model_index[j] < n_models, std::string(who) + ": bad model_index");
  }
  return 0;
}

extern "C" int ampc_ilqr_plan_set_models(ampc_ilqr_plan* p, int n_models, ampc_handle* const* models) {
  REQUIRE(p, "ampc_ilqr_plan_set_models: NULL plan");
  HIP_OK(hipSetDevice(p->h->device));
  if (n_models == 0) {
    HIP_OK(hipStreamSynchronize(p->h->stream));
    for (ampc_handle* mh : p->models) handle_release(mh);
    p->models.clear();
    return 0;
  }
  REQUIRE(n_models >= 1 && models, "ampc_ilqr_plan_set_models: NULL argument");
  REQUIRE(p->prog_slots == 0, std::string("ampc_ilqr_plan_set_models") + kProgIlqrNoTable);
  REQUIRE(p->table_n == 0, "ampc_ilqr_plan_set_models: the plan holds a table of MLP models of mixed shapes "
                           "(ampc_ilqr_plan_set_model_table); remove it first");
  REQUIRE(p->sindy_n == 0, "ampc_ilqr_plan_set_models: the plan holds a table of SINDy models "
                           "(ampc_ilqr_plan_set_sindy_models); remove it first");
  REQUIRE(p->lqt_n == 0, "ampc_ilqr_plan_set_models: the plan holds a table of linear models "
                         "(ampc_ilqr_plan_set_linear_models); remove it first");
  for (int i = 0; i < n_models; ++i)
    if (int rc = check_same_shape(p->h, models[i], "ampc_ilqr_plan_set_models")) return rc;
  if (p->static_shape < 0) {
    const bool ready = jit::eligible(p->h) && (p->h->precision == AMPC_F64 ? jit::get<double>(p->h, true) != nullptr
                                                                           : jit::get<float>(p->h, true) != nullptr);
    if (ready) {
      HIP_OK(hipStreamSynchronize(p->h->stream));
      if (int rc = p->h->precision == AMPC_F64 ? ilqr_plan_build<double>(p) : ilqr_plan_build<float>(p)) return rc;
    }
    REQUIRE(p->static_shape >= 0, std::string("ampc_ilqr_plan_set_models") + kNeedStatic);
  }
  return p->h->precision == AMPC_F64 ? build_model_table<double>(p->h, n_models, models, &p->mlp_tab, &p->models)
                                     : build_model_table<float>(p->h, n_models, models, &p->mlp_tab, &p->models);
}

// ---------------------------------------------------------------------------------------------
// MLP models of any mix of depth, widths and activation in one plan (ilqr_table_kernels.hpp)
// ---------------------------------------------------------------------------------------------
size_t kstep_mlp_model_bytes();
void kstep_mlp_pack_model(void* dst, int n_layers, int act, const int* dims, const double* const* w,
                          const double* const* b, const double* const* norm);

extern "C" int ampc_ilqr_plan_set_model_table(ampc_ilqr_plan* p, int n_models, const int* n_hidden, const int* dims,
                                              const int* activations, const double* const* weights,
                                              const double* const* biases, const double* const* norms,
                                              const int* on_device) {
  if (!p) return ilqr_table_fail("NULL plan");
  ampc_handle* h = p->h;
  if (n_models == 0) {                               // back to the handle's own model and its kernels
    if (p->table_n == 0) return 0;
    HIP_OK(hipSetDevice(h->device));
    HIP_OK(hipStreamSynchronize(h->stream));
    p->table_n = 0; p->table_wmax = 0; p->table_hidden = 0;
    p->table_models.release(); p->table_stage.release(); p->table_dz.release();
    return ilqr_plan_build<double>(p);               // (the kernel choices of the handle's shape)
  }
  if (p->prog_slots > 0) return fail(std::string("ampc_ilqr_plan_set_model_table") + kProgIlqrNoTable);
  if (p->sindy_n > 0)
    return ilqr_table_fail("the plan holds a table of SINDy models (ampc_ilqr_plan_set_sindy_models); remove it first");
  if (p->lqt_n > 0)
    return ilqr_table_fail("the plan holds a table of linear models (ampc_ilqr_plan_set_linear_models); remove it first");
  IlqrTablePlanView v;
  v.f64 = h->precision == AMPC_F64;
  v.has_mlp = h->has_mlp && !h->has_sindy && !h->has_lin && h->lin_n == 0;    // (a small linear model is staged as a network)
  v.nx = h->nx; v.nu = h->nu; v.obs_dim = h->obs_dim;
  v.n_shape_models = (int)p->models.size(); v.cost_stride = h->cost_stride;
  KstepMlpPrep prep;
  if (int rc = ilqr_table_check(v, n_models, n_hidden, dims, activations, weights, biases, norms, on_device,
                                ilqr_table_lds_base(), kLdsLimit, &prep))
    return rc;
  HIP_OK(hipSetDevice(h->device));
  const int ML = prep.max_layers;
  auto resident = [&](const void* q) -> int {
    hipPointerAttribute_t attr;
    const hipError_t e = hipPointerGetAttributes(&attr, q);
    if (e != hipSuccess) (void)hipGetLastError();     // (a host address is an error of the query: not left behind)
    if (!(e == hipSuccess && attr.type == hipMemoryTypeDevice && attr.device == h->device))
      return ilqr_table_fail("a model flagged as device-resident has a parameter that is not device memory of the "
                             "plan's device");
    return 0;
  };
  for (int k = 0; k < n_models; ++k) {
    if (!on_device[k]) continue;
    for (int l = 0; l <= n_hidden[k]; ++l) {
      if (int rc = resident(weights[(size_t)k * ML + l])) return rc;
      if (int rc = resident(biases[(size_t)k * ML + l])) return rc;
    }
    for (int i = 0; i < 4; ++i)
      if (int rc = resident(norms[(size_t)k * 4 + i])) return rc;
  }
  // (a running solve may read the table being replaced)
  HIP_OK(hipStreamSynchronize(h->stream));
  // From here on the plan holds NO table until the new one is complete: a failure below leaves the plan on its
  // handle's own model, never on entries that point into memory this call has overwritten or released.
  p->table_n = 0; p->table_wmax = 0; p->table_hidden = 0;
  p->static_shape = -1;
  p->jit = nullptr;
  int wmax = 0, hmax = 0;
  ilqr_table_extent(n_models, n_hidden, dims, ML, &wmax, &hmax);
  const size_t mb = kstep_mlp_model_bytes();
  HIP_OK(p->table_dz.reserve((size_t)hmax * p->B * round_up(p->H, 16) * wmax * 8));
  HIP_OK(p->table_models.reserve((size_t)n_models * mb));
  if (!prep.stage.empty()) {
    HIP_OK(p->table_stage.reserve(prep.stage.size() * 8));
    HIP_OK(hipMemcpy(p->table_stage.p, prep.stage.data(), prep.stage.size() * 8, hipMemcpyHostToDevice));
  }
  std::vector<char> table((size_t)n_models * mb);
  const double* sb = (const double*)p->table_stage.p;
  for (int k = 0; k < n_models; ++k) {
    const double* w[8] = {nullptr};
    const double* b[8] = {nullptr};
    const double* nm[4];
    for (int l = 0; l <= n_hidden[k]; ++l) {
      const size_t e = (size_t)k * ML + l;
      w[l] = on_device[k] ? weights[e] : sb + prep.w_off[e];
      b[l] = on_device[k] ? biases[e] : sb + prep.b_off[e];
    }
    for (int i = 0; i < 4; ++i) nm[i] = on_device[k] ? norms[(size_t)k * 4 + i] : sb + prep.n_off[(size_t)k * 4 + i];
    kstep_mlp_pack_model(table.data() + (size_t)k * mb, n_hidden[k] + 1, activations[k], dims + (size_t)k * (ML + 1),
                         w, b, nm);
  }
  HIP_OK(hipMemcpy(p->table_models.p, table.data(), table.size(), hipMemcpyHostToDevice));
  // (the run-time-shape sweep serves every model of the table; no shape-specialised kernel or plugin is involved:
  //  static_shape / jit were cleared above)
  p->table_n = n_models; p->table_wmax = wmax; p->table_hidden = hmax;
  return 0;
}

// ---------------------------------------------------------------------------------------------
// SINDy models of any mix of feature libraries in one plan (ilqr_sindy_table_kernels.hpp)
// ---------------------------------------------------------------------------------------------
static IlqrSindyView ilqr_sindy_view(const ampc_handle* h) {
  IlqrSindyView v;
  v.f64 = h->precision == AMPC_F64; v.has_sindy = h->has_sindy ? 1 : 0; v.device = h->device;
  v.nx = h->nx; v.nu = h->nu; v.obs_dim = h->obs_dim;
  v.n_feat = h->s_nfeat; v.n_trig = h->s_ntrig; v.n_pow = h->s_npow; v.n_mon = h->s_nmon; v.n_pool = h->s_npool;
  v.n_tab = h->s_ntab;
  v.stage = (h->has_sindy && v.f64 && sindy_stage_bytes<double>(h) > 0) ? 1 : 0;
  return v;
}

static void ilqr_sindy_table_drop(ampc_ilqr_plan* p) {
  for (ampc_handle* mh : p->sindy_models) handle_release(mh);
  p->sindy_models.clear();
  p->sindy_n = 0;
  p->sindy_lds = 0;
}

extern "C" int ampc_ilqr_plan_set_sindy_models(ampc_ilqr_plan* p, int n_models, ampc_handle* const* models) {
  if (!p) return ilqr_sindy_table_fail("NULL plan");
  ampc_handle* h = p->h;
  if (n_models == 0) {                               // back to the handle's own model and its kernels
    if (p->sindy_n == 0) return 0;
    HIP_OK(hipSetDevice(h->device));
    HIP_OK(hipStreamSynchronize(h->stream));
    ilqr_sindy_table_drop(p);
    return 0;
  }
  if (n_models < 1 || !models) return ilqr_sindy_table_fail("NULL argument");
  if (p->prog_slots > 0) return fail(std::string("ampc_ilqr_plan_set_sindy_models") + kProgIlqrNoTable);
  if (p->lqt_n > 0)
    return ilqr_sindy_table_fail("the plan holds a table of linear models (ampc_ilqr_plan_set_linear_models); remove it first");
  const IlqrSindyView pv = ilqr_sindy_view(h);
  std::vector<IlqrSindyView> views((size_t)n_models);
  std::vector<const IlqrSindyView*> vp((size_t)n_models, nullptr);
  for (int i = 0; i < n_models; ++i)
    if (models[i]) { views[i] = ilqr_sindy_view(models[i]); vp[i] = &views[i]; }
  size_t need = 0;
  if (int rc = ilqr_sindy_table_check(pv, h->cost_stride, (int)p->models.size(), p->table_n, n_models, vp.data(), kLdsLimit,
                                      &need))
    return rc;
  for (int i = 0; i < n_models; ++i) {
    const IlqrSindyView& v = views[i];
    if (v.stage && ilqr_sindy_prog_elems(v.nx, v.n_feat, v.n_trig, v.n_pow, v.n_mon, v.n_pool) * 8 <
                       sindy_stage_bytes<double>(models[i]))
      return ilqr_sindy_table_fail("internal: the staged program's size");
  }
  HIP_OK(hipSetDevice(h->device));
  // (a running solve may read the table being replaced; the models' staging has finished before a kernel reads it)
  HIP_OK(hipStreamSynchronize(h->stream));
  for (int i = 0; i < n_models; ++i) HIP_OK(hipStreamSynchronize(models[i]->stream));
  // From here on the plan holds NO table until the new one is complete: a failure below leaves the plan on its
  // handle's own model.
  ilqr_sindy_table_drop(p);
  std::vector<SindyDev<double>> descs((size_t)n_models);
  for (int i = 0; i < n_models; ++i) descs[i] = sindy_of<double>(models[i]);
  HIP_OK(p->sindy_tab.reserve(descs.size() * sizeof(SindyDev<double>)));
  HIP_OK(hipMemcpyAsync(p->sindy_tab.p, descs.data(), descs.size() * sizeof(SindyDev<double>), hipMemcpyHostToDevice,
                        h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));           // (descs lives until here)
  p->sindy_models.assign(models, models + n_models);
  for (ampc_handle* mh : p->sindy_models) mh->refs++;
  p->sindy_n = n_models;
  p->sindy_lds = need;
  return 0;
}

extern "C" int ampc_ilqr_solve_queue_var(ampc_ilqr_plan* p, int n_problems, const double* x0, const double* uguess,
                                         const int* cost_index, const int* horizon, const int* model_index,
                                         int max_iter, double* states, double* ctrls, double* Ks, double* ks,
                                         int* converged, int* iters, int* status, double* objective) {
  REQUIRE(p && x0, "ampc_ilqr_solve_queue_var: NULL argument");
  REQUIRE(n_problems >= 1, "ampc_ilqr_solve_queue_var: n_problems < 1");
  REQUIRE(max_iter >= 1, "ampc_ilqr_solve_queue_var: max_iter < 1");
  if (cost_index)
    for (int j = 0; j < n_problems; ++j)
      REQUIRE(cost_index[j] >= 0 && cost_index[j] < p->h->n_costs, "ampc_ilqr_solve_queue_var: bad cost_index");
  if (int rc = check_horizons(p, n_problems, horizon, "ampc_ilqr_solve_queue_var")) return rc;
  if (int rc = check_models(p, n_problems, model_index, "ampc_ilqr_solve_queue_var")) return rc;
  if (int rc = ilqr_program_plan_check(p, "ampc_ilqr_solve_queue_var")) return rc;
  HIP_OK(hipSetDevice(p->h->device));
  return p->h->precision == AMPC_F64
             ? ilqr_solve_queue_impl<double>(p, n_problems, x0, uguess, cost_index, horizon, model_index, max_iter, states,
                                             ctrls, Ks, ks, converged, iters, status, objective)
             : ilqr_solve_queue_impl<float>(p, n_problems, x0, uguess, cost_index, horizon, model_index, max_iter, states,
                                            ctrls, Ks, ks, converged, iters, status, objective);
}

extern "C" int ampc_ilqr_solve_queue(ampc_ilqr_plan* p, int n_problems, const double* x0, const double* uguess,
                                     const int* cost_index, int max_iter, double* states, double* ctrls,
                                     double* Ks, double* ks, int* converged, int* iters, int* status,
                                     double* objective) {
  REQUIRE(p && x0, "ampc_ilqr_solve_queue: NULL argument");
  REQUIRE(n_problems >= 1, "ampc_ilqr_solve_queue: n_problems < 1");
  REQUIRE(max_iter >= 1, "ampc_ilqr_solve_queue: max_iter < 1");
  if (int rc = ilqr_program_plan_check(p, "ampc_ilqr_solve_queue")) return rc;
  if (cost_index)
    for (int j = 0; j < n_problems; ++j)
      REQUIRE(cost_index[j] >= 0 && cost_index[j] < p->h->n_costs, "ampc_ilqr_solve_queue: bad cost_index");
  HIP_OK(hipSetDevice(p->h->device));
  return p->h->precision == AMPC_F64
             ? ilqr_solve_queue_impl<double>(p, n_problems, x0, uguess, cost_index, nullptr, nullptr, max_iter, states, ctrls,
                                             Ks, ks, converged, iters, status, objective)
             : ilqr_solve_queue_impl<float>(p, n_problems, x0, uguess, cost_index, nullptr, nullptr, max_iter, states, ctrls,
                                            Ks, ks, converged, iters, status, objective);
}

// ---------------------------------------------------------------------------------------------
// Device-resident closed loops of iLQR controllers (ilqr_chain_*_kernel)
// ---------------------------------------------------------------------------------------------
template <typename T>
static int ilqr_closed_loop_impl(ampc_ilqr_plan* p, ampc_handle* sur, int C, const double* init_obs,
                                 const int* cost_index, const int* horizon, const int* model_index, int n_steps,
                                 int max_iter, double* traj_obs,
                                 double* traj_ctrls, int* failed, int* steps_done, long long* iterations) {
  ampc_handle* h = p->h;
  const int nx = h->nx, nu = h->nu, B = p->B, H = p->H, T1 = n_steps + 1;
  const size_t e = sizeof(T);
  // ints: ctl[2] | slot_mode[B] (where make_ilqr_args expects it: q_ctl + 2 + B) ...
  HIP_OK(p->q_ctl.reserve((size_t)(2 + 2 * B) * sizeof(int)));
  HIP_OK(p->c_ints.reserve((size_t)(2 * B + 5 * C) * sizeof(int)));      // need[B] slot_chain[B] chain_t[C] chain_fail[C] cost[C] horizon[C] model[C]
  HIP_OK(p->c_iters.reserve((size_t)C * sizeof(long long)));
  HIP_OK(p->c_stage.reserve((size_t)B * (2 * nx + nu) * e));
  HIP_OK(p->c_obs.reserve((size_t)C * T1 * nx * e));
  HIP_OK(p->c_ctl.reserve((size_t)C * T1 * nu * e));
  HIP_OK(p->q_x0.reserve((size_t)C * nx * e));
  std::vector<int> ctl(2 + 2 * B, 0), ci(2 * B + 5 * C, 0), slot_h0(B, H);
  for (int b = 0; b < B; ++b) { ctl[2 + b] = -1; ctl[2 + B + b] = 1; ci[B + b] = -1; }
  if (cost_index) std::memcpy(ci.data() + 2 * B + 2 * C, cost_index, (size_t)C * sizeof(int));
  if (horizon) {
    std::memcpy(ci.data() + 2 * B + 3 * C, horizon, (size_t)C * sizeof(int));
    HIP_OK(p->slot_h.reserve((size_t)B * sizeof(int)));
    HIP_OK(hipMemcpyAsync(p->slot_h.p, slot_h0.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice, h->stream));
  }
  if (model_index) {
    std::memcpy(ci.data() + 2 * B + 4 * C, model_index, (size_t)C * sizeof(int));
    HIP_OK(p->slot_model.reserve((size_t)B * sizeof(int)));
    HIP_OK(hipMemsetAsync(p->slot_model.p, 0, (size_t)B * sizeof(int), h->stream));
  }
  HIP_OK(hipMemcpyAsync(p->q_ctl.p, ctl.data(), ctl.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipMemcpyAsync(p->c_ints.p, ci.data(), ci.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipMemsetAsync(p->c_iters.p, 0, (size_t)C * sizeof(long long), h->stream));
  HIP_OK(hipMemsetAsync(p->c_obs.p, 0, (size_t)C * T1 * nx * e, h->stream));
  HIP_OK(hipMemsetAsync(p->c_ctl.p, 0, (size_t)C * T1 * nu * e, h->stream));
  HIP_OK(hipMemsetAsync(p->c_stage.p, 0, (size_t)B * (2 * nx + nu) * e, h->stream));
  HIP_OK(upload_converted<T>(p->q_x0.p, init_obs, (size_t)C * nx, h->stream));
  HIP_OK(hipMemsetAsync(p->flags.p, 0, (size_t)9 * B * sizeof(int), h->stream));
  HIP_OK(hipMemsetAsync(p->states.p, 0, (size_t)B * (H + 1) * nx * e, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  if (p->poll_host) { (void)hipHostFree(p->poll_host); p->poll_host = nullptr; }
  const int npoll = 2 * B + 3;               // active[B], ls_need[B], the chains' two counters, slots with work
  HIP_OK(hipHostMalloc((void**)&p->poll_host, (size_t)2 * npoll * sizeof(int), hipHostMallocDefault));
  if (!p->poll_ev[0])
    for (int i = 0; i < 2; ++i) HIP_OK(hipEventCreateWithFlags(&p->poll_ev[i], hipEventDisableTiming));
  struct Guard {
    ampc_ilqr_plan* p;
    ~Guard() {
      (void)hipStreamSynchronize(p->h->stream);
      (void)hipMemcpyAsync(p->d_cost_idx.p, p->cost_idx.data(), (size_t)p->B * sizeof(int), hipMemcpyHostToDevice,
                           p->h->stream);
      (void)hipStreamSynchronize(p->h->stream);
      p->queue_on = false; p->var_h = false; p->var_model = false; p->compact_on = false; p->ev_cur = nullptr;
      (void)hipHostFree(p->poll_host); p->poll_host = nullptr;
    }
  } guard{p};
  p->queue_on = true;
  p->var_h = horizon != nullptr;
  p->var_model = model_index != nullptr;
  p->queue_max_iter = max_iter;
  p->active_hint = B;
  p->ls_rb_now = 1;
  p->compact_on = ilqr_wants_compaction(p);
  if (p->compact_on) HIP_OK(p->slot_of.reserve((size_t)(B + 1) * sizeof(int)));
  IlqrChains<T> q;
  q.C = C; q.B = B; q.H = H; q.nx = nx; q.nu = nu; q.n_steps = n_steps; q.max_iter = max_iter;
  q.ctl = (int*)p->q_ctl.p;
  int* ints = (int*)p->c_ints.p;
  q.need = ints; q.slot_chain = ints + B; q.chain_t = ints + 2 * B; q.chain_fail = ints + 2 * B + C;
  q.cost = ints + 2 * B + 2 * C;
  q.horizon = horizon ? ints + 2 * B + 3 * C : nullptr; q.slot_h = (int*)p->slot_h.p;
  q.model = model_index ? ints + 2 * B + 4 * C : nullptr; q.slot_model = (int*)p->slot_model.p;
  q.chain_iters = (long long*)p->c_iters.p;
  q.x0 = (const T*)p->q_x0.p; q.cost_idx = (int*)p->d_cost_idx.p;
  q.stage_x = (T*)p->c_stage.p; q.stage_u = q.stage_x + (size_t)B * nx; q.stage_next = q.stage_u + (size_t)B * nu;
  q.traj_obs = (T*)p->c_obs.p; q.traj_ctrls = (T*)p->c_ctl.p;
  // Upper bound on the plan iterations: every control step of every chain takes at most max_iter + 2.
  constexpr int kPoll = 4;
  const long long bound = ((long long)(C + B - 1) / B) * n_steps * (max_iter + 2LL) + (long long)C + 4 * kPoll;
  long long it = 0;
  int batch = 0, pending = -1;
  bool done = false;
  int poll_now = kPoll;                      // (2 once every chain has been handed out: the grids follow the count of
  while (!done && it < bound) {             //  slots whose chain is unfinished, compact_on)
    for (int k = 0; k < poll_now; ++k) {
      IlqrArgs<T> a = make_ilqr_args<T>(p, 1);
      hipLaunchKernelGGL(ilqr_chain_pre_kernel<T>, dim3(B), dim3(64), 0, h->stream, a, q);
      HIP_OK(hipGetLastError());
      if (int rc = surrogate_step<T>(h, sur, q.stage_x, q.stage_u, q.stage_next, B)) return rc;
      hipLaunchKernelGGL(ilqr_chain_post_kernel<T>, dim3(B), dim3(256), 0, h->stream, a, q);
      HIP_OK(hipGetLastError());
      if (int rc = ilqr_compact<T>(p)) return rc;
      int rc = ilqr_launch_iter<T>(p, 1);
      if (rc == 0) rc = ilqr_refresh_jacobians<T>(p);
      if (rc) { (void)hipStreamSynchronize(h->stream); return rc; }
    }
    it += poll_now;
    const int slot = batch & 1;
    int* ph = p->poll_host + (size_t)slot * npoll;
    HIP_OK(hipMemcpyAsync(ph, (const int*)p->flags.p + B, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipMemcpyAsync(ph + B, (const int*)p->flags.p + 8 * B, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipMemcpyAsync(ph + 2 * B, p->q_ctl.p, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (p->compact_on)
      HIP_OK(hipMemcpyAsync(ph + 2 * B + 2, (const int*)p->slot_of.p + B, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipEventRecord(p->poll_ev[slot], h->stream));
    if (pending >= 0) {
      const int* pp = p->poll_host + (size_t)(pending & 1) * npoll;
      HIP_OK(hipEventSynchronize(p->poll_ev[pending & 1]));
      p->ls_rb_now = ls_rb_from_poll(pp, pp + B, B);
      // every chain handed out: the slots with work (an unfinished chain: solving, or its next control step just
      // loaded -- counted by ilqr_compact_kernel) can only become fewer
      if (p->compact_on && pp[2 * B] >= C) {
        p->active_hint = std::min(B, std::max(pp[2 * B + 2], 1));
        poll_now = 2;
      }
      if (pp[2 * B + 1] >= C) done = true;
    }
    pending = batch++;
  }
  HIP_OK(hipStreamSynchronize(h->stream));
  p->last_queue_launches = it;
  p->last_iterations = (int)std::min<long long>(it, 1 << 30);
  int fin[2] = {0, 0};
  HIP_OK(hipMemcpy(fin, p->q_ctl.p, sizeof(fin), hipMemcpyDeviceToHost));
  if (fin[1] < C) return fail("ampc_ilqr_closed_loop: internal: the chains did not finish");
  std::vector<int> back((size_t)2 * B + 3 * C);
  HIP_OK(hipMemcpy(back.data(), p->c_ints.p, back.size() * sizeof(int), hipMemcpyDeviceToHost));
  if (steps_done) std::memcpy(steps_done, back.data() + 2 * B, (size_t)C * sizeof(int));
  if (failed) std::memcpy(failed, back.data() + 2 * B + C, (size_t)C * sizeof(int));
  if (iterations) HIP_OK(hipMemcpy(iterations, p->c_iters.p, (size_t)C * sizeof(long long), hipMemcpyDeviceToHost));
  if (traj_obs) HIP_OK(download_converted<T>(traj_obs, p->c_obs.p, (size_t)C * T1 * nx, h->stream));
  if (traj_ctrls) HIP_OK(download_converted<T>(traj_ctrls, p->c_ctl.p, (size_t)C * T1 * nu, h->stream));
  return 0;
}

extern "C" int ampc_ilqr_closed_loop(ampc_ilqr_plan* p, ampc_handle* surrogate, int n_chains, const double* init_obs,
                                     const int* cost_index, int n_steps, int max_iter, double* traj_obs,
                                     double* traj_ctrls, int* failed, int* steps_done, long long* iterations) {
  return ampc_ilqr_closed_loop_var(p, surrogate, n_chains, init_obs, cost_index, nullptr, nullptr, n_steps, max_iter,
                                   traj_obs, traj_ctrls, failed, steps_done, iterations);
}

extern "C" int ampc_ilqr_closed_loop_var(ampc_ilqr_plan* p, ampc_handle* surrogate, int n_chains, const double* init_obs,
                                         const int* cost_index, const int* horizon, const int* model_index,
                                         int n_steps, int max_iter, double* traj_obs, double* traj_ctrls, int* failed,
                                         int* steps_done, long long* iterations) {
  REQUIRE(p && init_obs, "ampc_ilqr_closed_loop: NULL argument");
  REQUIRE(p->lqt_n == 0, "ampc_ilqr_closed_loop: the plan holds a table of linear models (ampc_ilqr_plan_set_linear_models), "
                         "whose controller states are not the observation: use ampc_ilqr_closed_loop_linear");
  if (int rc = check_horizons(p, n_chains, horizon, "ampc_ilqr_closed_loop_var")) return rc;
  if (int rc = check_models(p, n_chains, model_index, "ampc_ilqr_closed_loop_var")) return rc;
  if (int rc = ilqr_program_plan_check(p, "ampc_ilqr_closed_loop")) return rc;
  REQUIRE(n_chains >= 1 && n_steps >= 1 && max_iter >= 1, "ampc_ilqr_closed_loop: n_chains, n_steps, max_iter must be >= 1");
  ampc_handle* sur = surrogate ? surrogate : p->h;
  REQUIRE(sur->has_model() && sur->nx == p->h->nx && sur->nu == p->h->nu,
          "ampc_ilqr_closed_loop: surrogate model must have the controller model's dimensions");
  REQUIRE(sur->precision == p->h->precision && sur->device == p->h->device,
          "ampc_ilqr_closed_loop: surrogate must share the plan's device and precision");
  if (cost_index)
    for (int j = 0; j < n_chains; ++j)
      REQUIRE(cost_index[j] >= 0 && cost_index[j] < p->h->n_costs, "ampc_ilqr_closed_loop: bad cost_index");
  HIP_OK(hipSetDevice(p->h->device));
  return p->h->precision == AMPC_F64
             ? ilqr_closed_loop_impl<double>(p, sur, n_chains, init_obs, cost_index, horizon, model_index, n_steps, max_iter,
                                             traj_obs, traj_ctrls, failed, steps_done, iterations)
             : ilqr_closed_loop_impl<float>(p, sur, n_chains, init_obs, cost_index, horizon, model_index, n_steps, max_iter,
                                            traj_obs, traj_ctrls, failed, steps_done, iterations);
}

// ---------------------------------------------------------------------------------------------
// Linear models of mixed state dimension in one plan (ilqr_linear_table_kernels.hpp)
// ---------------------------------------------------------------------------------------------
static int ilqr_linear_table_fail(const std::string& msg, int rc = -1) {
  g_err = "ampc_ilqr_plan_set_linear_models: " + msg;
  return rc;
}

// Where ampc_ilqr_plan_set_linear_models puts things (no device call; the call itself packs by these numbers).
extern "C" int ampc_ilqr_linear_table_layout(int n_models, const int* nx, int nu, int obs_dim, int B, int H, int ls_n,
                                             long long* entry_off, long long* strides) {
  REQUIRE(n_models >= 1 && nx && entry_off && strides, "ampc_ilqr_linear_table_layout: NULL argument");
  REQUIRE(nu >= 1 && obs_dim >= 1 && B >= 1 && H >= 1 && ls_n >= 1, "ampc_ilqr_linear_table_layout: bad dimensions");
  long long o = 0;
  int w = 0;
  for (int i = 0; i < n_models; ++i) {
    REQUIRE(nx[i] >= 1, "ampc_ilqr_linear_table_layout: bad state dimension");
    const long long n = nx[i], k = n + nu, nxp = round_up(nx[i], 16), ksn = round_up((int)k, 4) / 4, ldj = round_up((int)k, 16);
    entry_off[3 * i] = o;                                       // fragments [ntile][ksn][64]
    entry_off[3 * i + 1] = o + (nxp / 16) * ksn * 64;           // plain rows [nx][nx + nu], padded to four values
    entry_off[3 * i + 2] = entry_off[3 * i + 1] + round_up((int)(n * k), 4);   // jp [nxp][ldj]
    o = entry_off[3 * i + 2] + nxp * ldj;
    w = std::max(w, nx[i]);
  }
  const long long W = w;
  strides[0] = (long long)(H + 1) * W;                          // states, per slot / per problem
  strides[1] = (long long)H * nu;                               // ctrls
  strides[2] = (long long)H * nu * W;                           // Ks
  strides[3] = (long long)H * nu;                               // ks
  strides[4] = (long long)ls_n * (H + 1) * W;                   // ls_states
  strides[5] = (long long)ls_n * H * nu;                        // ls_ctrls
  strides[6] = (long long)round_up(w, 16) * round_up(w + nu, 16);   // vj
  strides[7] = o;                                               // values in the table buffer
  strides[8] = (long long)ilqr_linear_table_sweep_bytes(w, nu, obs_dim);                                  // LDS of the sweep
  strides[9] = (long long)ilqr_linear_table_ls_map(w, nu, cost_block_stride(obs_dim, nu), nullptr, nullptr);   // ... line search
  return 0;
}

extern "C" int ampc_ilqr_plan_set_linear_models(ampc_ilqr_plan* p, int n_models, ampc_handle* const* models,
                                                const int* rules, const int* n_basis, const int* lift_kinds,
                                                const double* lift_params) {
  if (!p) return ilqr_linear_table_fail("NULL plan");
  ampc_handle* h = p->h;
  if (n_models == 0) {                               // back to the handle's own model and its kernels
    if (p->lqt_n == 0) return 0;
    HIP_OK(hipSetDevice(h->device));
    HIP_OK(hipStreamSynchronize(h->stream));
    for (ampc_handle* mh : p->lqt_models) handle_release(mh);
    p->lqt_models.clear(); p->lqt_nx.clear();
    p->lqt_n = 0; p->lqt_nxw = 0; p->lqt_loop = false; p->lqt_sweep_bytes = 0; p->lqt_ls_bytes = 0;
    return ilqr_plan_build<double>(p);               // (the kernel choices and buffers of the handle's own model)
  }
  if (n_models < 1 || !models) return ilqr_linear_table_fail("NULL argument");
  if (p->prog_slots > 0) return fail(std::string("ampc_ilqr_plan_set_linear_models") + kProgIlqrNoTable);
  if (h->precision != AMPC_F64) return ilqr_linear_table_fail("the table kernels are f64 only; this plan's handle is f32");
  if (!(h->lin_n > 0 && h->lin_n == h->nx))
    return ilqr_linear_table_fail("the plan handle's model is not a linear model (ampc_set_linear)");
  if (!p->models.empty())
    return ilqr_linear_table_fail("the plan holds per-problem models of one shape (ampc_ilqr_plan_set_models); remove them first");
  if (p->table_n > 0)
    return ilqr_linear_table_fail("the plan holds a table of MLP models (ampc_ilqr_plan_set_model_table); remove it first");
  if (p->sindy_n > 0)
    return ilqr_linear_table_fail("the plan holds a table of SINDy models (ampc_ilqr_plan_set_sindy_models); remove it first");
  const int nu = h->nu, no = h->obs_dim;
  if (!(nu == 1 || nu == 2 || nu == 3 || nu == 4 || nu == 6 || nu == 8))
    return ilqr_linear_table_fail("the sweep on linear models is built for 1, 2, 3, 4, 6 or 8 controls");
  int n_lift = 0, nxw = 0;
  std::vector<int> lift_off(n_models, 0);
  for (int i = 0; i < n_models; ++i) {
    const ampc_handle* m = models[i];
    if (!m) return ilqr_linear_table_fail("NULL model handle");
    if (!(m->lin_n > 0 && m->lin_n == m->nx && (int)m->lin_ab_host.size() == m->nx * (m->nx + m->nu)))
      return ilqr_linear_table_fail("a model handle holds no linear model (ampc_set_linear)");
    if (m->precision != AMPC_F64) return ilqr_linear_table_fail("the table kernels are f64 only; a model's handle is f32");
    if (m->device != h->device) return ilqr_linear_table_fail("models must share the plan's device");
    if (m->nu != nu) return ilqr_linear_table_fail("models must have the plan handle's control dimension");
    if (m->nx < no) return ilqr_linear_table_fail("a model has fewer states than the cost's observation (nx < obs_dim)");
    if (m->nx > kLinMaxIlqrNx)
      return ilqr_linear_table_fail("iLQR on linear models takes up to 128 model states (the value function's Hessian lives "
                                    "in LDS); a model has more");
    nxw = std::max(nxw, m->nx);
    if (!rules) continue;
    if (rules[i] < 0 || rules[i] > 2) return ilqr_linear_table_fail("rule must be 0 observation, 1 ARX shift, 2 lift");
    if (rules[i] == 0 && m->nx != no) return ilqr_linear_table_fail("rule 0 (state = observation) needs nx == obs_dim");
    if (rules[i] == 2) {
      if (!(n_basis && lift_kinds && lift_params)) return ilqr_linear_table_fail("rule 2 needs n_basis, lift_kinds and lift_params");
      if (!(n_basis[i] >= 1 && no >= 1 && n_basis[i] * no == m->nx))
        return ilqr_linear_table_fail("n_basis * obs_dim must be the model's state dimension");
      lift_off[i] = 2 * n_lift;
      for (int k = n_lift; k < n_lift + n_basis[i]; ++k) {
        if (lift_kinds[k] < 0 || lift_kinds[k] > 3) return ilqr_linear_table_fail("lift kind must be 0 identity, 1 power, 2 sin, 3 cos");
        if (lift_kinds[k] == 1 && !(lift_params[k] >= 0 && lift_params[k] <= 64 && lift_params[k] == std::floor(lift_params[k])))
          return ilqr_linear_table_fail("powers must be integers in 0..64");
      }
      n_lift += n_basis[i];
    }
  }
  int lds_xn = 0, lds_work = 0;
  std::vector<int> nxs_in(n_models);
  for (int i = 0; i < n_models; ++i) nxs_in[i] = models[i]->nx;
  std::vector<long long> lay_off(3 * (size_t)n_models), lay(10);
  if (int rc = ampc_ilqr_linear_table_layout(n_models, nxs_in.data(), nu, no, p->B, p->H, p->ls_n, lay_off.data(), lay.data()))
    return rc;
  const size_t sweep_bytes = (size_t)lay[8];
  const size_t ls_bytes = ilqr_linear_table_ls_map(nxw, nu, h->cost_stride, &lds_xn, &lds_work);
  if (ls_bytes != (size_t)lay[9]) return ilqr_linear_table_fail("internal: the cost block's stride");
  if (sweep_bytes > kLdsLimit || ls_bytes > kLdsLimit)
    return ilqr_linear_table_fail("the widest model's sweep workspace or line-search rows and cost block need more than 160 KB "
                                  "of LDS", -3);
  if ((size_t)p->B * (p->H + 1) * nxw >= ((size_t)1 << 31)) return ilqr_linear_table_fail("the plan's state regions exceed 2^31 values");
  HIP_OK(hipSetDevice(h->device));
  // Pack every entry from its handle's exact f64 [A | B]: the fragments in set_linear_wide's order, the plain rows, the
  // sweep's zero-padded jp [nxp][ldj] -- into buffers of this call, installed only once everything is on the device.
  std::vector<size_t> off(n_models + 1, 0);
  for (int i = 0; i < n_models; ++i) off[i] = (size_t)lay_off[3 * i];
  off[n_models] = (size_t)lay[7];
  std::vector<double> buf(off[n_models], 0.0);
  DevBuf nbuf, ntab, nrules, nprog;
  struct Drop { DevBuf* b[4]; bool armed = true; ~Drop() { if (armed) for (DevBuf* x : b) x->release(); } } drop{{&nbuf, &ntab, &nrules, &nprog}};
  HIP_OK(nbuf.reserve(buf.size() * 8));
  std::vector<LinDev<double>> tab(n_models);
  for (int i = 0; i < n_models; ++i) {
    const std::vector<double>& ab = models[i]->lin_ab_host;
    const int nx = models[i]->nx, k = nx + nu, nxp = round_up(nx, 16), kp = round_up(k, 4), ntile = nxp / 16, ksn = kp / 4;
    const int ldj = round_up(k, 16), plain_sz = round_up(nx * k, 4);
    double* wf = buf.data() + off[i];
    auto Mat = [&](int row, int col) -> double { return (row >= nx || col >= k) ? 0.0 : ab[(size_t)row * k + col]; };
    for (int nt = 0; nt < ntile; ++nt)
      for (int ks = 0; ks < ksn; ++ks)
        for (int l = 0; l < 64; ++l) wf[((size_t)nt * ksn + ks) * 64 + l] = Mat(16 * nt + (l & 15), 4 * ks + (l >> 4));
    double* plain = buf.data() + lay_off[3 * i + 1];
    for (size_t e = 0; e < (size_t)nx * k; ++e) plain[e] = ab[e];
    double* jp = buf.data() + lay_off[3 * i + 2];
    for (int r = 0; r < nx; ++r)
      for (int c = 0; c < k; ++c) jp[(size_t)r * ldj + c] = ab[(size_t)r * k + c];
    LinDev<double>& m = tab[i];
    m.nx = nx; m.nu = nu; m.nxp = nxp; m.kp = kp; m.ntile = ntile; m.ksn = ksn;
    m.wf = (const double*)nbuf.p + off[i];
    m.plain = (const double*)nbuf.p + lay_off[3 * i + 1];
    m.jp = (const double*)nbuf.p + lay_off[3 * i + 2]; m.ldj = ldj;
  }
  std::vector<int> rl(3 * (size_t)n_models, 0);
  std::vector<double> prog;
  for (int i = 0, k = 0; i < n_models; ++i) {
    rl[i] = rules ? rules[i] : 0;
    const int nb = rules && rules[i] == 2 ? n_basis[i] : 0;
    rl[n_models + i] = nb;
    rl[2 * n_models + i] = lift_off[i];
    for (int j = 0; j < nb; ++j, ++k) { prog.push_back(lift_kinds[k]); prog.push_back(lift_params[k]); }
  }
  HIP_OK(ntab.reserve(tab.size() * sizeof(LinDev<double>)));
  HIP_OK(nrules.reserve(rl.size() * sizeof(int)));
  HIP_OK(nprog.reserve((prog.size() + 2) * 8));
  // (a running solve may read the table being replaced; everything below goes through the plan's OWN stream: the
  //  handle's stream is non-blocking, so the null stream is not ordered against the plan's kernels)
  HIP_OK(hipStreamSynchronize(h->stream));
  HIP_OK(hipMemcpyAsync(nbuf.p, buf.data(), buf.size() * 8, hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipMemcpyAsync(ntab.p, tab.data(), tab.size() * sizeof(LinDev<double>), hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipMemcpyAsync(nrules.p, rl.data(), rl.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
  if (!prog.empty()) HIP_OK(hipMemcpyAsync(nprog.p, prog.data(), prog.size() * 8, hipMemcpyHostToDevice, h->stream));
  // the per-slot buffers at the widest entry's stride (grown only; what a solve reads of them it has written before)
  const int B = p->B, H = p->H, nxs = std::max(nxw, h->nx);
  HIP_OK(p->states.reserve((size_t)B * std::max<size_t>(lay[0], (size_t)(H + 1) * nxs) * 8));
  HIP_OK(p->ctrls.reserve((size_t)B * lay[1] * 8));
  HIP_OK(p->Ks.reserve((size_t)B * std::max<size_t>(lay[2], (size_t)H * nu * nxs) * 8));
  HIP_OK(p->ks.reserve((size_t)B * lay[3] * 8));
  HIP_OK(p->ls_states.reserve((size_t)B * std::max<size_t>(lay[4], (size_t)p->ls_n * (H + 1) * nxs) * 8));
  HIP_OK(p->ls_ctrls.reserve((size_t)B * lay[5] * 8));
  HIP_OK(p->vj.reserve((size_t)B * lay[6] * 8));
  HIP_OK(hipMemsetAsync(p->Ks.p, 0, (size_t)B * H * nu * nxs * 8, h->stream));
  HIP_OK(hipMemsetAsync(p->ks.p, 0, (size_t)B * H * nu * 8, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));           // (buf, tab, rl, prog live until here)
  // complete: the new table in, the old handles back
  std::swap(p->lqt_buf, nbuf); std::swap(p->lqt_tab, ntab); std::swap(p->lqt_rules, nrules); std::swap(p->lqt_prog, nprog);
  std::vector<ampc_handle*> old;
  old.swap(p->lqt_models);
  p->lqt_models.assign(models, models + n_models);
  for (ampc_handle* mh : p->lqt_models) mh->refs++;
  for (ampc_handle* mh : old) handle_release(mh);
  p->lqt_nx.clear();
  for (int i = 0; i < n_models; ++i) p->lqt_nx.push_back(models[i]->nx);
  p->lqt_n = n_models; p->lqt_nxw = nxw; p->lqt_loop = rules != nullptr;
  p->lqt_lds_xn = lds_xn; p->lqt_lds_work = lds_work; p->lqt_sweep_bytes = sweep_bytes; p->lqt_ls_bytes = ls_bytes;
  p->static_shape = -1;                              // (no shape-specialised kernel or plugin runs on a table plan)
  p->jit = nullptr;
  return 0;                                          // (Drop releases the OLD table's buffers, swapped into the locals)
}

// simulate() with IterativeLQR controllers on a table of linear models, device resident: ilqr_closed_loop_impl with a
// surrogate state per slot beside the controller state and the controller-state rules between surrogate step and post.
static int ilqr_closed_loop_linear_impl(ampc_ilqr_plan* p, ampc_handle* sur, int C, const double* init_states,
                                        const double* init_sim, const int* cost_index, const int* horizon,
                                        const int* model_index, int n_steps, int max_iter, double* traj_obs,
                                        double* traj_ctrls, int* failed, int* steps_done, long long* iterations) {
  using T = double;
  ampc_handle* h = p->h;
  const int nxw = p->lqt_nxw, nu = h->nu, B = p->B, H = p->H, T1 = n_steps + 1, snx = sur->nx, NM = p->lqt_n;
  const size_t e = sizeof(T), db = ilqr_linear_table_desc_bytes();
  std::vector<int> x_off(C);
  size_t sum_nx = 0;
  for (int c = 0; c < C; ++c) { x_off[c] = (int)sum_nx; sum_nx += p->lqt_nx[model_index ? model_index[c] : 0]; }
  REQUIRE(sum_nx < ((size_t)1 << 31), "ampc_ilqr_closed_loop_linear: too many states in init_states");
  HIP_OK(p->q_ctl.reserve((size_t)(2 + 2 * B) * sizeof(int)));
  // ints: need[B] slot_chain[B] chain_t[C] chain_fail[C] cost[C] horizon[C] model[C] x_off[C]
  HIP_OK(p->c_ints.reserve((size_t)(2 * B + 6 * C) * sizeof(int)));
  HIP_OK(p->c_iters.reserve((size_t)C * sizeof(long long)));
  HIP_OK(p->c_stage.reserve((size_t)B * (nu + snx) * e));                // stage_u [B][nu] | stage_next [B][snx]
  // sim [B][snx] | sim0 [C][snx] | zero controls [C][nu] (u_prev of the first run())
  HIP_OK(p->lqt_sim.reserve(((size_t)B * snx + (size_t)C * snx + (size_t)C * nu) * e));
  HIP_OK(p->lqt_desc.reserve((size_t)(B + C) * db));                     // per slot | per chain (the first run())
  HIP_OK(p->c_obs.reserve((size_t)C * T1 * snx * e));
  HIP_OK(p->c_ctl.reserve((size_t)C * T1 * nu * e));
  HIP_OK(p->q_x0.reserve(sum_nx * e));
  HIP_OK(p->slot_h.reserve((size_t)B * sizeof(int)));
  HIP_OK(p->slot_model.reserve((size_t)B * sizeof(int)));
  std::vector<int> ctl(2 + 2 * B, 0), ci(2 * B + 6 * C, 0), slot_h0(B, H);
  for (int b = 0; b < B; ++b) { ctl[2 + b] = -1; ctl[2 + B + b] = 1; ci[B + b] = -1; }
  if (cost_index) std::memcpy(ci.data() + 2 * B + 2 * C, cost_index, (size_t)C * sizeof(int));
  if (horizon) std::memcpy(ci.data() + 2 * B + 3 * C, horizon, (size_t)C * sizeof(int));
  if (model_index) std::memcpy(ci.data() + 2 * B + 4 * C, model_index, (size_t)C * sizeof(int));
  std::memcpy(ci.data() + 2 * B + 5 * C, x_off.data(), (size_t)C * sizeof(int));
  // the chains' first run(): state <- rule(traj_to_state, u_prev = 0, first observation), all chains in one launch
  const std::vector<int> rl_host = [&] {
    std::vector<int> v(3 * (size_t)NM);
    (void)hipMemcpy(v.data(), p->lqt_rules.p, v.size() * sizeof(int), hipMemcpyDeviceToHost);
    return v;
  }();
  std::vector<char> desc((size_t)(B + C) * db, 0);
  for (int b = 0; b < B; ++b) ilqr_linear_table_desc_fill(desc.data(), b, 0, 0, 0, 0, 0, 0);
  for (int c = 0; c < C; ++c) {
    const int mi = model_index ? model_index[c] : 0;
    ilqr_linear_table_desc_fill(desc.data(), B + c, p->lqt_nx[mi], rl_host[mi], rl_host[NM + mi], mi, x_off[c], rl_host[2 * NM + mi]);
  }
  T* sim = (T*)p->lqt_sim.p; T* sim0 = sim + (size_t)B * snx; T* u_zero = sim0 + (size_t)C * snx;
  HIP_OK(hipMemcpyAsync(p->slot_h.p, slot_h0.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipMemsetAsync(p->slot_model.p, 0, (size_t)B * sizeof(int), h->stream));
  HIP_OK(hipMemcpyAsync(p->q_ctl.p, ctl.data(), ctl.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipMemcpyAsync(p->c_ints.p, ci.data(), ci.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipMemcpyAsync(p->lqt_desc.p, desc.data(), desc.size(), hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipMemsetAsync(p->c_iters.p, 0, (size_t)C * sizeof(long long), h->stream));
  HIP_OK(hipMemsetAsync(p->c_obs.p, 0, (size_t)C * T1 * snx * e, h->stream));
  HIP_OK(hipMemsetAsync(p->c_ctl.p, 0, (size_t)C * T1 * nu * e, h->stream));
  HIP_OK(hipMemsetAsync(p->c_stage.p, 0, (size_t)B * (nu + snx) * e, h->stream));
  HIP_OK(hipMemsetAsync(p->lqt_sim.p, 0, ((size_t)B * snx + (size_t)C * snx + (size_t)C * nu) * e, h->stream));
  HIP_OK(upload_converted<T>(p->q_x0.p, init_states, sum_nx, h->stream));
  HIP_OK(upload_converted<T>(sim0, init_sim, (size_t)C * snx, h->stream));
  HIP_OK(hipMemsetAsync(p->flags.p, 0, (size_t)9 * B * sizeof(int), h->stream));
  HIP_OK(hipMemsetAsync(p->states.p, 0, (size_t)B * (H + 1) * nxw * e, h->stream));
  if (int rc = ilqr_linear_table_ctrl_state(p, C, (const char*)p->lqt_desc.p + (size_t)B * db, (T*)p->q_x0.p, sim0, snx, u_zero))
    return rc;
  HIP_OK(hipStreamSynchronize(h->stream));
  if (p->poll_host) { (void)hipHostFree(p->poll_host); p->poll_host = nullptr; }
  const int npoll = 2 * B + 3;
  HIP_OK(hipHostMalloc((void**)&p->poll_host, (size_t)2 * npoll * sizeof(int), hipHostMallocDefault));
  if (!p->poll_ev[0])
    for (int i = 0; i < 2; ++i) HIP_OK(hipEventCreateWithFlags(&p->poll_ev[i], hipEventDisableTiming));
  struct Guard {
    ampc_ilqr_plan* p;
    ~Guard() {
      (void)hipStreamSynchronize(p->h->stream);
      (void)hipMemcpyAsync(p->d_cost_idx.p, p->cost_idx.data(), (size_t)p->B * sizeof(int), hipMemcpyHostToDevice,
                           p->h->stream);
      (void)hipStreamSynchronize(p->h->stream);
      p->queue_on = false; p->var_h = false; p->var_model = false; p->compact_on = false; p->ev_cur = nullptr;
      (void)hipHostFree(p->poll_host); p->poll_host = nullptr;
    }
  } guard{p};
  p->queue_on = true;
  p->var_h = true;                    // (slot_h is always filled here: H without `horizon`)
  p->var_model = true;
  p->queue_max_iter = max_iter;
  p->active_hint = B;
  p->ls_rb_now = 1;
  p->compact_on = false;
  IlqrLinChains q;
  q.C = C; q.B = B; q.H = H; q.nxw = nxw; q.nu = nu; q.snx = snx; q.n_steps = n_steps; q.max_iter = max_iter;
  q.ctl = (int*)p->q_ctl.p;
  int* ints = (int*)p->c_ints.p;
  q.need = ints; q.slot_chain = ints + B; q.chain_t = ints + 2 * B; q.chain_fail = ints + 2 * B + C;
  q.cost = ints + 2 * B + 2 * C;
  q.horizon = horizon ? ints + 2 * B + 3 * C : nullptr; q.slot_h = (int*)p->slot_h.p;
  q.model = ints + 2 * B + 4 * C; q.slot_model = (int*)p->slot_model.p;
  q.x_off = ints + 2 * B + 5 * C;
  const int* rl = (const int*)p->lqt_rules.p;
  q.rule = rl; q.n_basis = rl + NM; q.lift_off = rl + 2 * NM;
  q.chain_iters = (long long*)p->c_iters.p;
  q.x0 = (const T*)p->q_x0.p; q.sim0 = sim0; q.cost_idx = (int*)p->d_cost_idx.p;
  q.sim = sim; q.stage_u = (T*)p->c_stage.p; q.stage_next = q.stage_u + (size_t)B * nu;
  q.desc = (LinCtrlDesc*)p->lqt_desc.p;
  q.traj_obs = (T*)p->c_obs.p; q.traj_ctrls = (T*)p->c_ctl.p;
  constexpr int kPoll = 4;
  const long long bound = ((long long)(C + B - 1) / B) * n_steps * (max_iter + 2LL) + (long long)C + 4 * kPoll;
  long long it = 0;
  int batch = 0, pending = -1;
  bool done = false;
  while (!done && it < bound) {
    for (int k = 0; k < kPoll; ++k) {
      IlqrArgs<T> a = make_ilqr_args<T>(p, 1);
      if (int rc = ilqr_linear_table_chain_pre(p, &a, &q)) return rc;
      if (int rc = surrogate_step<T>(h, sur, q.sim, q.stage_u, q.stage_next, B)) return rc;
      if (int rc = ilqr_linear_table_ctrl_state(p, B, p->lqt_desc.p, (T*)p->states.p, q.stage_next, snx, q.stage_u)) return rc;
      if (int rc = ilqr_linear_table_chain_post(p, &a, &q)) return rc;
      int rc = ilqr_launch_iter<T>(p, 1);
      if (rc == 0) rc = ilqr_refresh_jacobians<T>(p);
      if (rc) { (void)hipStreamSynchronize(h->stream); return rc; }
    }
    it += kPoll;
    const int slot = batch & 1;
    int* ph = p->poll_host + (size_t)slot * npoll;
    HIP_OK(hipMemcpyAsync(ph, (const int*)p->flags.p + B, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipMemcpyAsync(ph + B, (const int*)p->flags.p + 8 * B, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipMemcpyAsync(ph + 2 * B, p->q_ctl.p, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipEventRecord(p->poll_ev[slot], h->stream));
    if (pending >= 0) {
      const int* pp = p->poll_host + (size_t)(pending & 1) * npoll;
      HIP_OK(hipEventSynchronize(p->poll_ev[pending & 1]));
      if (pp[2 * B + 1] >= C) done = true;
    }
    pending = batch++;
  }
  HIP_OK(hipStreamSynchronize(h->stream));
  p->last_queue_launches = it;
  p->last_iterations = (int)std::min<long long>(it, 1 << 30);
  int fin[2] = {0, 0};
  HIP_OK(hipMemcpy(fin, p->q_ctl.p, sizeof(fin), hipMemcpyDeviceToHost));
  if (fin[1] < C) return fail("ampc_ilqr_closed_loop_linear: internal: the chains did not finish");
  std::vector<int> back((size_t)2 * B + 2 * C);
  HIP_OK(hipMemcpy(back.data(), p->c_ints.p, back.size() * sizeof(int), hipMemcpyDeviceToHost));
  if (steps_done) std::memcpy(steps_done, back.data() + 2 * B, (size_t)C * sizeof(int));
  if (failed) std::memcpy(failed, back.data() + 2 * B + C, (size_t)C * sizeof(int));
  if (iterations) HIP_OK(hipMemcpy(iterations, p->c_iters.p, (size_t)C * sizeof(long long), hipMemcpyDeviceToHost));
  if (traj_obs) HIP_OK(download_converted<T>(traj_obs, p->c_obs.p, (size_t)C * T1 * snx, h->stream));
  if (traj_ctrls) HIP_OK(download_converted<T>(traj_ctrls, p->c_ctl.p, (size_t)C * T1 * nu, h->stream));
  return 0;
}

extern "C" int ampc_ilqr_closed_loop_linear(ampc_ilqr_plan* p, ampc_handle* surrogate, int n_chains,
                                            const double* init_states, const double* init_sim, const int* cost_index,
                                            const int* horizon, const int* model_index, int n_steps, int max_iter,
                                            double* traj_obs, double* traj_ctrls, int* failed, int* steps_done,
                                            long long* iterations) {
  static const std::string w = "ampc_ilqr_closed_loop_linear";
  REQUIRE(p && init_states && init_sim, w + ": NULL argument");
  REQUIRE(p->lqt_n > 0, w + ": the plan holds no table of linear models (ampc_ilqr_plan_set_linear_models)");
  REQUIRE(p->lqt_loop, w + ": the table was set without rules (solves only)");
  REQUIRE(n_chains >= 1 && n_steps >= 1 && max_iter >= 1, w + ": n_chains, n_steps, max_iter must be >= 1");
  if (int rc = check_horizons(p, n_chains, horizon, "ampc_ilqr_closed_loop_linear")) return rc;
  if (int rc = check_models(p, n_chains, model_index, "ampc_ilqr_closed_loop_linear")) return rc;
  const ampc_handle* h = p->h;
  ampc_handle* sur = surrogate ? surrogate : p->h;
  REQUIRE(sur->has_model() && sur->nu == h->nu && sur->nx >= h->obs_dim,
          w + ": the surrogate must have the plan's controls and a state that starts with the observation");
  REQUIRE(sur->precision == h->precision && sur->device == h->device,
          w + ": surrogate must share the plan's device and precision");
  if (cost_index)
    for (int j = 0; j < n_chains; ++j)
      REQUIRE(cost_index[j] >= 0 && cost_index[j] < h->n_costs, w + ": bad cost_index");
  HIP_OK(hipSetDevice(h->device));
  return ilqr_closed_loop_linear_impl(p, sur, n_chains, init_states, init_sim, cost_index, horizon, model_index, n_steps,
                                      max_iter, traj_obs, traj_ctrls, failed, steps_done, iterations);
}
