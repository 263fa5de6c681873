// api_lqr.cpp -- LQR plans (reference: autompc/control/lqr.py:35-47 _finite_horz_dt_lqr, :139-192 FiniteHorizonLQR;
// :22-33 _inf_horz_dt_lqr, :96-136 InfiniteHorizonLQR): batched Riccati gains of controller models of any state dimension up to 256 in
// one launch, and the device-resident closed loop simulate() runs with those gains (utils/simulation.py:44-63).
// f64 only; kernels in lqr_kernels.hpp, launchers in launch_lqr.cpp.
#include "host_common.hpp"

#include <numeric>

extern template int surrogate_step<double>(ampc_handle*, ampc_handle*, const void*, const void*, void*, int);

int lqr_launch_gains(hipStream_t st, int n, const void* descs, const void* order, void* ws, const void* cost,
                     void* kout, void* status);
int lqr_launch_ctrl(hipStream_t st, int B, const void* descs, void* states, int cur, const void* sim, int snx,
                    int no, int nu, void* u, const void* kbuf, const void* gbuf, const void* lbuf, const void* lo,
                    const void* hi);
int lqr_launch_record(hipStream_t st, int B, const void* next, const void* u, void* sim, void* tobs, void* tctl,
                      int snx, int no, int nu, int T1, int step);
size_t lqr_desc_bytes();
size_t lqr_loop_desc_bytes();
void lqr_pack_desc(void* dst, int n, int nu, int no, int horizon, int id, const double* ab, long long ws,
                   long long cost, long long k, double threshold, int max_iter);
void lqr_pack_loop_desc(void* dst, int n, int rule, int n_basis, int noclip, const double* ab, long long s,
                        long long k, long long goal, long long lift);

// horizons as LQRFactory's space (lqr.py:214-224): a Riccati step of a 256-state model is ~70 MFLOP in one
// workgroup, so 1000 steps hold a compute unit for well under a second
static constexpr int kLqrPlanMaxN = 256, kLqrPlanMaxNu = 16, kLqrMaxHorizon = 1000;
// the cap of an infinite-horizon problem's max_iter: at about a millisecond per update of a 256-state model, a
// workgroup that never converges gives up after a couple of minutes at the latest
static constexpr int kLqrMaxIterCap = 100000;

struct ampc_lqr_plan {
  int device = 0, B = 0, no = 0, nu = 0;
  hipStream_t stream = nullptr;
  std::vector<ampc_handle*> models;     // one reference held per problem
  std::vector<int> n;                   // state dimension per problem
  std::vector<unsigned> gen;            // the model's lin_gen when it was taken
  std::vector<long long> k_off;         // K [nu][n_i] offsets (doubles), packed in problem order
  long long k_total = 0;
  bool have_gains = false;
  DevBuf descs, order, ws, cost, kbuf, status;   // status: [B] status then [B] update counts
  // closed loop
  bool have_loop = false;
  std::vector<int> rule;
  DevBuf ldescs, states, goal, lift, lo, hi, u, sim, next, tobs, tctl;
};

// A model re-staged after ampc_lqr_plan_set_models (another ampc_set_linear, or a nonlinear model) would leave the
// plan with a stale dimension or stale [A | B]: refused until the models are set again.
static int lqr_check_models(const ampc_lqr_plan* p, const char* who) {
  REQUIRE((int)p->models.size() == p->B, std::string(who) + ": set the models first (ampc_lqr_plan_set_models)");
  for (int i = 0; i < p->B; ++i)
    REQUIRE(p->models[i]->lin_n == p->n[i] && p->models[i]->lin_gen == p->gen[i],
            std::string(who) + ": a model was re-staged after ampc_lqr_plan_set_models; set the models again");
  return 0;
}

static void lqr_drop_models(ampc_lqr_plan* p) {
  for (ampc_handle* m : p->models) handle_release(m);
  p->models.clear();
}

extern "C" int ampc_lqr_plan_create(int device, int n_problems, int obs_dim, int ctrl_dim, ampc_lqr_plan** out) {
  REQUIRE(out, "ampc_lqr_plan_create: NULL out");
  *out = nullptr;
  REQUIRE(n_problems >= 1, "ampc_lqr_plan_create: n_problems < 1");
  REQUIRE(obs_dim >= 1 && obs_dim <= kLqrPlanMaxN, "ampc_lqr_plan_create: obs_dim must be in 1..256");
  REQUIRE(ctrl_dim >= 1 && ctrl_dim <= kLqrPlanMaxNu, "ampc_lqr_plan_create: ctrl_dim must be in 1..16");
  HIP_OK(hipSetDevice(device));
  ampc_lqr_plan* p = new ampc_lqr_plan();
  p->device = device; p->B = n_problems; p->no = obs_dim; p->nu = ctrl_dim;
  hipError_t e = hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    delete p;
    return fail(std::string("hipStreamCreate: ") + hipGetErrorString(e));
  }
  *out = p;
  return 0;
}

extern "C" int ampc_lqr_plan_destroy(ampc_lqr_plan* p) {
  if (!p) return 0;
  (void)hipSetDevice(p->device);
  (void)hipStreamSynchronize(p->stream);
  for (DevBuf* b : {&p->descs, &p->order, &p->ws, &p->cost, &p->kbuf, &p->status, &p->ldescs, &p->states, &p->goal,
                    &p->lift, &p->lo, &p->hi, &p->u, &p->sim, &p->next, &p->tobs, &p->tctl})
    b->release();
  (void)hipStreamDestroy(p->stream);
  lqr_drop_models(p);
  delete p;
  return 0;
}

extern "C" int ampc_lqr_plan_set_models(ampc_lqr_plan* p, ampc_handle* const* models) {
  REQUIRE(p && models, "ampc_lqr_plan_set_models: NULL argument");
  for (int i = 0; i < p->B; ++i) {
    const ampc_handle* m = models[i];
    REQUIRE(m, "ampc_lqr_plan_set_models: NULL model handle");
    REQUIRE(!m->has_prog, std::string("ampc_lqr_plan_set_models") + kProgNoPlan);
    REQUIRE(m->lin_n > 0 && m->has_model(),
            "ampc_lqr_plan_set_models: LQR needs a linear model (ampc_set_linear; the reference's is_compatible, "
            "lqr.py:161-168)");
    REQUIRE(m->precision == AMPC_F64, "ampc_lqr_plan_set_models: LQR is f64 only (f32 handles are refused)");
    REQUIRE(m->device == p->device, "ampc_lqr_plan_set_models: models must be on the plan's device");
    REQUIRE(m->nu == p->nu, "ampc_lqr_plan_set_models: a model's control dimension differs from the plan's");
    REQUIRE(m->lin_n >= p->no && m->lin_n <= kLqrPlanMaxN,
            "ampc_lqr_plan_set_models: model state dimension must be in obs_dim..256");
  }
  HIP_OK(hipSetDevice(p->device));
  (void)hipStreamSynchronize(p->stream);
  lqr_drop_models(p);
  p->n.assign(p->B, 0);
  p->gen.assign(p->B, 0);
  p->k_off.assign(p->B, 0);
  long long k = 0;
  for (int i = 0; i < p->B; ++i) {
    ampc_handle* m = models[i];
    m->refs++;
    p->models.push_back(m);
    HIP_OK(hipStreamSynchronize(m->stream));      // (staging done)
    if (m->lin_ab_gen != m->lin_gen) {            // first plan on this staging: upload its exact [A | B]
      HIP_OK(m->lin_ab.reserve(m->lin_ab_host.size() * 8));
      HIP_OK(hipMemcpy(m->lin_ab.p, m->lin_ab_host.data(), m->lin_ab_host.size() * 8, hipMemcpyHostToDevice));
      m->lin_ab_gen = m->lin_gen;
    }
    p->n[i] = m->lin_n;
    p->gen[i] = m->lin_gen;
    p->k_off[i] = k;
    k += (long long)p->nu * p->n[i];
  }
  p->k_total = k;
  HIP_OK(p->kbuf.reserve((size_t)k * 8));
  p->have_gains = p->have_loop = false;
  return 0;
}

// horizons[i] == 0: infinite horizon (thresholds[i], max_iters[i]); who: the entry point, for the messages
static int lqr_gains_impl(ampc_lqr_plan* p, const char* who, const int* horizons, const double* thresholds,
                          const int* max_iters, const double* Q, const double* R, const double* F, double* K,
                          int* status, int* iters) {
  if (int rc = lqr_check_models(p, who)) return rc;
  const int B = p->B, no = p->no, nu = p->nu;
  const bool ex = thresholds != nullptr;
  for (int i = 0; i < B; ++i) {
    if (!ex) {
      REQUIRE(horizons[i] >= 1 && horizons[i] <= kLqrMaxHorizon,
              std::string(who) + ": horizon must be in 1..1000 (LQRFactory's range, lqr.py:214-224)");
      continue;
    }
    REQUIRE(horizons[i] >= 0 && horizons[i] <= kLqrMaxHorizon,
            std::string(who) + ": horizon must be 0 (infinite) or in 1..1000 (LQRFactory's range, lqr.py:214-224)");
    if (horizons[i] != 0) continue;
    REQUIRE(std::isfinite(thresholds[i]) && thresholds[i] > 0.0,
            std::string(who) + ": the threshold of an infinite-horizon problem must be finite and > 0");
    REQUIRE(max_iters[i] >= 1 && max_iters[i] <= kLqrMaxIterCap,
            std::string(who) + ": max_iter of an infinite-horizon problem must be in 1..100000");
  }
  HIP_OK(hipSetDevice(p->device));
  const size_t dsz = lqr_desc_bytes();
  const long long csz = 2LL * no * no + (long long)nu * nu;
  std::vector<char> descs((size_t)B * dsz);
  long long ws = 0;
  for (int i = 0; i < B; ++i) {
    const int n = p->n[i], m = n + nu;
    const bool inf = horizons[i] == 0;
    lqr_pack_desc(descs.data() + (size_t)i * dsz, n, nu, no, horizons[i], i, (const double*)p->models[i]->lin_ab.p,
                  ws, (long long)i * csz, p->k_off[i], inf ? thresholds[i] : 0.0, inf ? max_iters[i] : 0);
    ws += (long long)n * n + (long long)n * m + (long long)m * m;
  }
  // heaviest problem first: (horizon + 2) * n^3 decides how long a workgroup runs; an infinite-horizon problem's
  // length is not known before it runs, so it is placed as if it were the longest horizon
  std::vector<int> order(B);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
    const double ha = horizons[a] == 0 ? kLqrMaxHorizon : horizons[a];
    const double hb = horizons[b] == 0 ? kLqrMaxHorizon : horizons[b];
    const double wa = (ha + 2.0) * p->n[a] * p->n[a] * (p->n[a] + nu);
    const double wb = (hb + 2.0) * p->n[b] * p->n[b] * (p->n[b] + nu);
    return wa > wb;
  });
  std::vector<double> cost((size_t)B * csz);
  for (int i = 0; i < B; ++i) {
    double* c = cost.data() + (size_t)i * csz;
    std::memcpy(c, Q + (size_t)i * no * no, (size_t)no * no * 8);
    std::memcpy(c + no * no, R + (size_t)i * nu * nu, (size_t)nu * nu * 8);
    std::memcpy(c + no * no + nu * nu, F + (size_t)i * no * no, (size_t)no * no * 8);
  }
  HIP_OK(p->descs.reserve(descs.size()));
  HIP_OK(p->order.reserve((size_t)B * 4));
  HIP_OK(p->ws.reserve((size_t)ws * 8));
  HIP_OK(p->cost.reserve(cost.size() * 8));
  HIP_OK(p->status.reserve((size_t)B * 8));
  HIP_OK(hipMemcpyAsync(p->descs.p, descs.data(), descs.size(), hipMemcpyHostToDevice, p->stream));
  HIP_OK(hipMemcpyAsync(p->order.p, order.data(), (size_t)B * 4, hipMemcpyHostToDevice, p->stream));
  HIP_OK(hipMemcpyAsync(p->cost.p, cost.data(), cost.size() * 8, hipMemcpyHostToDevice, p->stream));
  if (int rc = lqr_launch_gains(p->stream, B, p->descs.p, p->order.p, p->ws.p, p->cost.p, p->kbuf.p, p->status.p))
    return rc;
  if (K) HIP_OK(hipMemcpyAsync(K, p->kbuf.p, (size_t)p->k_total * 8, hipMemcpyDeviceToHost, p->stream));
  std::vector<int> st(2 * (size_t)B);
  HIP_OK(hipMemcpyAsync(st.data(), p->status.p, (size_t)B * 8, hipMemcpyDeviceToHost, p->stream));
  HIP_OK(hipStreamSynchronize(p->stream));
  if (status) std::copy(st.begin(), st.begin() + B, status);
  if (iters) std::copy(st.begin() + B, st.end(), iters);
  p->have_gains = true;
  return 0;
}

extern "C" int ampc_lqr_gains(ampc_lqr_plan* p, const int* horizons, const double* Q, const double* R,
                              const double* F, double* K, int* status) {
  REQUIRE(p && horizons && Q && R && F, "ampc_lqr_gains: NULL argument");
  return lqr_gains_impl(p, "ampc_lqr_gains", horizons, nullptr, nullptr, Q, R, F, K, status, nullptr);
}

extern "C" int ampc_lqr_gains_ex(ampc_lqr_plan* p, const int* horizons, const double* thresholds,
                                 const int* max_iters, const double* Q, const double* R, const double* F, double* K,
                                 int* status, int* iters) {
  REQUIRE(p && horizons && thresholds && max_iters && Q && R && F, "ampc_lqr_gains_ex: NULL argument");
  return lqr_gains_impl(p, "ampc_lqr_gains_ex", horizons, thresholds, max_iters, Q, R, F, K, status, iters);
}

// clip[i] == 0: problem i's control is not clipped (NULL: every problem clips)
static int lqr_set_loop_impl(ampc_lqr_plan* p, const int* rules, const int* n_basis, const int* lift_kinds,
                             const double* lift_params, const double* goal, const double* ctrl_lo,
                             const double* ctrl_hi, const int* clip) {
  if (int rc = lqr_check_models(p, "ampc_lqr_plan_set_loop")) return rc;
  const int B = p->B, no = p->no, nu = p->nu;
  std::vector<double> prog;
  std::vector<long long> lift_off(B, 0);
  int kpos = 0;
  for (int i = 0; i < B; ++i) {
    const int n = p->n[i];
    REQUIRE(rules[i] >= 0 && rules[i] <= 2, "ampc_lqr_plan_set_loop: rule must be 0 observation, 1 ARX shift, 2 lift");
    REQUIRE(rules[i] != 0 || n == no, "ampc_lqr_plan_set_loop: rule 0 needs a model whose state is the observation");
    if (rules[i] == 2) {
      REQUIRE(n_basis && lift_kinds && lift_params, "ampc_lqr_plan_set_loop: rule 2 needs the lift program");
      const int nb = n_basis[i];
      REQUIRE(nb >= 1 && nb * no == n, "ampc_lqr_plan_set_loop: n_basis * obs_dim must be the model's state dimension");
      lift_off[i] = (long long)prog.size();
      for (int k = 0; k < nb; ++k, ++kpos) {
        const int kind = lift_kinds[kpos];
        const double par = lift_params[kpos];
        REQUIRE(kind >= 0 && kind <= 3, "ampc_lqr_plan_set_loop: lift kind must be 0 identity, 1 power, 2 sin, 3 cos");
        REQUIRE(kind != 1 || (par >= 0 && par <= 64 && par == std::floor(par)),
                "ampc_lqr_plan_set_loop: powers must be integers in 0..64");
        prog.push_back(kind);
        prog.push_back(par);
      }
    }
  }
  if (prog.empty()) prog.push_back(0.0);
  const size_t dsz = lqr_loop_desc_bytes();
  std::vector<char> descs((size_t)B * dsz);
  long long s = 0;
  for (int i = 0; i < B; ++i) {
    lqr_pack_loop_desc(descs.data() + (size_t)i * dsz, p->n[i], rules[i], rules[i] == 2 ? n_basis[i] : 0,
                       clip && clip[i] == 0 ? 1 : 0, (const double*)p->models[i]->lin_ab.p, s, p->k_off[i], (long long)i * no, lift_off[i]);
    s += 2LL * p->n[i];
  }
  HIP_OK(hipSetDevice(p->device));
  HIP_OK(p->ldescs.reserve(descs.size()));
  HIP_OK(p->states.reserve((size_t)s * 8));
  HIP_OK(p->goal.reserve((size_t)B * no * 8));
  HIP_OK(p->lift.reserve(prog.size() * 8));
  HIP_OK(p->lo.reserve((size_t)nu * 8));
  HIP_OK(p->hi.reserve((size_t)nu * 8));
  HIP_OK(p->u.reserve((size_t)B * nu * 8));
  HIP_OK(hipMemcpyAsync(p->ldescs.p, descs.data(), descs.size(), hipMemcpyHostToDevice, p->stream));
  HIP_OK(hipMemcpyAsync(p->goal.p, goal, (size_t)B * no * 8, hipMemcpyHostToDevice, p->stream));
  HIP_OK(hipMemcpyAsync(p->lift.p, prog.data(), prog.size() * 8, hipMemcpyHostToDevice, p->stream));
  HIP_OK(hipMemcpyAsync(p->lo.p, ctrl_lo, (size_t)nu * 8, hipMemcpyHostToDevice, p->stream));
  HIP_OK(hipMemcpyAsync(p->hi.p, ctrl_hi, (size_t)nu * 8, hipMemcpyHostToDevice, p->stream));
  HIP_OK(hipStreamSynchronize(p->stream));
  p->rule.assign(rules, rules + B);
  p->have_loop = true;
  return 0;
}

extern "C" int ampc_lqr_plan_set_loop(ampc_lqr_plan* p, const int* rules, const int* n_basis, const int* lift_kinds,
                                      const double* lift_params, const double* goal, const double* ctrl_lo,
                                      const double* ctrl_hi) {
  REQUIRE(p && rules && goal && ctrl_lo && ctrl_hi, "ampc_lqr_plan_set_loop: NULL argument");
  return lqr_set_loop_impl(p, rules, n_basis, lift_kinds, lift_params, goal, ctrl_lo, ctrl_hi, nullptr);
}

extern "C" int ampc_lqr_plan_set_loop_ex(ampc_lqr_plan* p, const int* rules, const int* n_basis,
                                         const int* lift_kinds, const double* lift_params, const double* goal,
                                         const double* ctrl_lo, const double* ctrl_hi, const int* clip) {
  REQUIRE(p && rules && goal && ctrl_lo && ctrl_hi, "ampc_lqr_plan_set_loop_ex: NULL argument");
  return lqr_set_loop_impl(p, rules, n_basis, lift_kinds, lift_params, goal, ctrl_lo, ctrl_hi, clip);
}

static int lqr_closed_loop_impl(ampc_lqr_plan* p, ampc_handle* sur, const double* init_state,
                                const double* init_sim, int n_steps, double* traj_obs, double* traj_ctrls,
                                int n_terms, const int* kinds, const double* params, double* scores) {
  REQUIRE(p->have_gains && p->have_loop, "ampc_lqr_closed_loop: compute the gains (ampc_lqr_gains) and set the loop "
                                         "(ampc_lqr_plan_set_loop) first");
  if (int rc = lqr_check_models(p, "ampc_lqr_closed_loop")) return rc;
  REQUIRE(sur && sur->has_model(), "ampc_lqr_closed_loop: the surrogate handle holds no model");
  REQUIRE(sur->precision == AMPC_F64 && sur->device == p->device,
          "ampc_lqr_closed_loop: the surrogate must be f64 on the plan's device");
  REQUIRE(sur->nu == p->nu && sur->nx >= p->no,
          "ampc_lqr_closed_loop: the surrogate must have the plan's controls and a state that starts with the "
          "observation");
  const int B = p->B, no = p->no, nu = p->nu, snx = sur->nx, T1 = n_steps + 1;
  HIP_OK(hipSetDevice(p->device));
  HIP_OK(hipStreamSynchronize(p->stream));
  HIP_OK(hipStreamSynchronize(sur->stream));
  hipStream_t st = p->stream;
  // controller state [modelstate, u_prev] of simulate()'s first step (traj_to_state, lqr.py:170-172);
  // u_prev = the one-row trajectory's control, zero
  long long s_total = 0;
  for (int i = 0; i < B; ++i) s_total += p->n[i];
  std::vector<double> st0(2 * (size_t)s_total, 0.0);
  long long s = 0, src = 0;
  for (int i = 0; i < B; ++i) {
    std::memcpy(st0.data() + s, init_state + src, (size_t)p->n[i] * 8);
    s += 2LL * p->n[i];
    src += p->n[i];
  }
  HIP_OK(p->sim.reserve((size_t)B * snx * 8));
  HIP_OK(p->next.reserve((size_t)B * snx * 8));
  HIP_OK(p->tobs.reserve((size_t)B * T1 * no * 8));
  HIP_OK(p->tctl.reserve((size_t)B * T1 * nu * 8));
  HIP_OK(hipMemcpyAsync(p->states.p, st0.data(), st0.size() * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(p->sim.p, init_sim, (size_t)B * snx * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemsetAsync(p->u.p, 0, (size_t)B * nu * 8, st));
  HIP_OK(hipMemsetAsync(p->tctl.p, 0, (size_t)B * T1 * nu * 8, st));
  // traj_obs[:, 0, :] = init_sim[:, :no]
  HIP_OK(hipMemcpy2DAsync(p->tobs.p, (size_t)T1 * no * 8, p->sim.p, (size_t)snx * 8, (size_t)no * 8, B,
                          hipMemcpyDeviceToDevice, st));
  // the surrogate step is enqueued on the surrogate handle's stream: run the whole loop there
  HIP_OK(hipStreamSynchronize(st));
  st = sur->stream;
  int rc = 0;
  for (int step = 0; step < n_steps && rc == 0; ++step) {
    rc = lqr_launch_ctrl(st, B, p->ldescs.p, p->states.p, step & 1, p->sim.p, snx, no, nu, p->u.p, p->kbuf.p,
                         p->goal.p, p->lift.p, p->lo.p, p->hi.p);
    if (rc) break;
    rc = surrogate_step<double>(sur, sur, p->sim.p, p->u.p, p->next.p, B);   // simstate = sim_model.pred(simstate, u)
    if (rc) break;
    rc = lqr_launch_record(st, B, p->next.p, p->u.p, p->sim.p, p->tobs.p, p->tctl.p, snx, no, nu, T1, step);
  }
  if (rc == 0 && traj_obs)
    rc = hipMemcpyAsync(traj_obs, p->tobs.p, (size_t)B * T1 * no * 8, hipMemcpyDeviceToHost, st) == hipSuccess
             ? 0 : fail("ampc_lqr_closed_loop: download failed");
  if (rc == 0 && traj_ctrls)
    rc = hipMemcpyAsync(traj_ctrls, p->tctl.p, (size_t)B * T1 * nu * 8, hipMemcpyDeviceToHost, st) == hipSuccess
             ? 0 : fail("ampc_lqr_closed_loop: download failed");
  if (rc == 0 && scores)
    rc = score_device_f64(sur, p->tobs.p, p->tctl.p, B, T1, no, nu, no, n_terms, kinds, params, scores);
  (void)hipStreamSynchronize(st);
  return rc;
}

extern "C" int ampc_lqr_closed_loop(ampc_lqr_plan* p, ampc_handle* surrogate, const double* init_state,
                                    const double* init_sim, int n_steps, double* traj_obs, double* traj_ctrls) {
  REQUIRE(p && surrogate && init_state && init_sim, "ampc_lqr_closed_loop: NULL argument");
  REQUIRE(n_steps >= 1, "ampc_lqr_closed_loop: n_steps < 1");
  return lqr_closed_loop_impl(p, surrogate, init_state, init_sim, n_steps, traj_obs, traj_ctrls, 0, nullptr, nullptr,
                              nullptr);
}

extern "C" int ampc_lqr_closed_loop_scored(ampc_lqr_plan* p, ampc_handle* surrogate, const double* init_state,
                                           const double* init_sim, int n_steps, int n_terms, const int* kinds,
                                           const double* params, double* scores, double* traj_obs,
                                           double* traj_ctrls) {
  REQUIRE(p && surrogate && init_state && init_sim && scores, "ampc_lqr_closed_loop_scored: NULL argument");
  REQUIRE(n_steps >= 1, "ampc_lqr_closed_loop_scored: n_steps < 1");
  REQUIRE(n_terms >= 1 && kinds && params, "ampc_lqr_closed_loop_scored: empty cost specification");
  return lqr_closed_loop_impl(p, surrogate, init_state, init_sim, n_steps, traj_obs, traj_ctrls, n_terms, kinds,
                              params, scores);
}
