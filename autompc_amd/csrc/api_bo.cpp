// api_bo.cpp -- ampc_bo_propose: one Bayesian-optimisation proposal (tuning/proposer.py) in one call: a Matern-5/2 GP
// fitted for every row of the hyperparameter table, the row of largest log marginal likelihood chosen on the host, its
// posterior over the pool, q greedy expected-improvement picks with the believer update.  f64 only; kernels in
// bo_kernels.hpp, launchers in launch_bo.cpp.  Stateless: every buffer lives for the call.
#include "fit_host.hpp"

int bo_max_n();
int bo_max_d();
int bo_max_g();
int bo_max_m();
int bo_max_q();
int bo_pool_block();
int bo_launch_fit(hipStream_t st, int n, int d, int G, const void* X, const void* z, const void* hw, const void* hnoise,
                  void* Kall, void* lml, void* status);
int bo_launch_posterior(hipStream_t st, const void* L, const void* X, const void* w, const void* pool, int n, int d,
                        int m, int Mp, double zmin, void* V, void* mu, void* var0, void* var, void* ei);
int bo_launch_picks(hipStream_t st, int n, int d, int m, int Mp, int q, const void* pool, const void* w, double noise,
                    double zmin, void* V, const void* mu, void* var, void* ei, void* picked, void* picks,
                    void* pick_ei, void* pick_margin);

extern "C" int ampc_bo_propose(int device, int n, int d, const double* X, const double* z, int n_hyper,
                               const double* hyper_w, const double* hyper_noise, int m, const double* pool, int q,
                               double* lml, int* hyper_status, int* chosen, int* picks, double* pick_ei,
                               double* pick_margin, double* mu, double* var) {
  REQUIRE(X && z && hyper_w && hyper_noise && pool, "ampc_bo_propose: NULL input");
  REQUIRE(lml && hyper_status && chosen && picks && pick_ei && pick_margin && mu && var, "ampc_bo_propose: NULL output");
  REQUIRE(n >= 1 && n <= bo_max_n(), "ampc_bo_propose: n (observations) must be in 1..2048");
  REQUIRE(d >= 1 && d <= bo_max_d(), "ampc_bo_propose: d (dimensions) must be in 1..64");
  REQUIRE(n_hyper >= 1 && n_hyper <= bo_max_g(), "ampc_bo_propose: n_hyper (hyperparameter rows) must be in 1..64");
  REQUIRE(m >= 1 && m <= bo_max_m(), "ampc_bo_propose: m (pool points) must be in 1..65536");
  REQUIRE(q >= 1 && q <= bo_max_q() && q <= m, "ampc_bo_propose: q (picks) must be in 1..min(m, 256)");
  const int G = n_hyper;
  const int Mp = (m + bo_pool_block() - 1) / bo_pool_block() * bo_pool_block();
  const size_t block = (size_t)(n + 1) * n;
  const double nan = std::nan("");

  REQUIRE(ampc_device_count() > 0, "ampc_bo_propose: no HIP device");
  HIP_OK(hipSetDevice(device));
  StreamGuard sg;
  HIP_OK(hipStreamCreateWithFlags(&sg.s, hipStreamNonBlocking));
  hipStream_t st = sg.s;
  ScopedBuf d_X, d_z, d_hw, d_hn, d_pool, d_K, d_lml, d_status, d_V, d_mu, d_var0, d_var, d_ei, d_picked, d_picks,
      d_pei, d_pmar;
  HIP_OK(d_X.reserve((size_t)n * d * 8));
  HIP_OK(d_z.reserve((size_t)n * 8));
  HIP_OK(d_hw.reserve((size_t)G * d * 8));
  HIP_OK(d_hn.reserve((size_t)G * 8));
  HIP_OK(d_K.reserve((size_t)G * block * 8));
  HIP_OK(d_lml.reserve((size_t)G * 8));
  HIP_OK(d_status.reserve((size_t)G * 4));
  HIP_OK(hipMemcpyAsync(d_X.p, X, (size_t)n * d * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_z.p, z, (size_t)n * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_hw.p, hyper_w, (size_t)G * d * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_hn.p, hyper_noise, (size_t)G * 8, hipMemcpyHostToDevice, st));
  if (int rc = bo_launch_fit(st, n, d, G, d_X.p, d_z.p, d_hw.p, d_hn.p, d_K.p, d_lml.p, d_status.p)) return rc;
  // (the pool travels while the rows are factored)
  HIP_OK(d_pool.reserve((size_t)m * d * 8));
  HIP_OK(hipMemcpyAsync(d_pool.p, pool, (size_t)m * d * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(lml, d_lml.p, (size_t)G * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(hyper_status, d_status.p, (size_t)G * 4, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));

  // the accepted row of largest lml, lowest index on ties
  int best = -1;
  for (int g = 0; g < G; ++g)
    if (hyper_status[g] == 0 && std::isfinite(lml[g]) && (best < 0 || lml[g] > lml[best])) best = g;
  *chosen = best;
  if (best < 0) {                  // every row declined: the statuses, and no picks
    for (int i = 0; i < q; ++i) { picks[i] = -1; pick_ei[i] = nan; pick_margin[i] = nan; }
    for (int i = 0; i < m; ++i) { mu[i] = nan; var[i] = nan; }
    return 0;
  }
  double zmin = z[0];
  for (int i = 1; i < n; ++i) zmin = z[i] < zmin ? z[i] : zmin;

  HIP_OK(d_V.reserve((size_t)(n + q) * Mp * 8));
  HIP_OK(d_mu.reserve((size_t)m * 8));
  HIP_OK(d_var0.reserve((size_t)m * 8));
  HIP_OK(d_var.reserve((size_t)m * 8));
  HIP_OK(d_ei.reserve((size_t)m * 8));
  HIP_OK(d_picked.reserve((size_t)m * 4));
  HIP_OK(d_picks.reserve((size_t)q * 4));
  HIP_OK(d_pei.reserve((size_t)q * 8));
  HIP_OK(d_pmar.reserve((size_t)q * 8));
  HIP_OK(hipMemsetAsync(d_picked.p, 0, (size_t)m * 4, st));
  const double* L = (const double*)d_K.p + (size_t)best * block;
  const double* w = (const double*)d_hw.p + (size_t)best * d;
  if (int rc = bo_launch_posterior(st, L, d_X.p, w, d_pool.p, n, d, m, Mp, zmin, d_V.p, d_mu.p, d_var0.p, d_var.p,
                                   d_ei.p))
    return rc;
  if (int rc = bo_launch_picks(st, n, d, m, Mp, q, d_pool.p, w, hyper_noise[best], zmin, d_V.p, d_mu.p, d_var.p,
                               d_ei.p, d_picked.p, d_picks.p, d_pei.p, d_pmar.p))
    return rc;
  HIP_OK(hipMemcpyAsync(mu, d_mu.p, (size_t)m * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(var, d_var0.p, (size_t)m * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(picks, d_picks.p, (size_t)q * 4, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(pick_ei, d_pei.p, (size_t)q * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(pick_margin, d_pmar.p, (size_t)q * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  return 0;
}
