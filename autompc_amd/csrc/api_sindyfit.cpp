// api_sindyfit.cpp -- ampc_sindy_fit: sequentially-thresholded least-squares fits of SINDy configurations of one data
// set in one call (what sysid/sindy.py SINDy.train does per model on the host).  One Gram launch for all designs
// (distinct feature libraries) -- a configuration's every iteration and target only needs a sub-matrix of its
// design's Gram Theta'[Theta | Y] -- then one solve workgroup per (configuration, target).
// f64 only; kernels in sindyfit_kernels.hpp, launchers in launch_sindyfit.cpp.
#include "fit_host.hpp"

size_t sindyfit_col_bytes();
size_t sindyfit_design_bytes();
size_t sindyfit_desc_bytes();
int sindyfit_max_state();
int sindyfit_max_ctrl();
int sindyfit_zero_kind();
int sindyfit_next_obs_kind();
int sindyfit_ycont_kind();
void sindyfit_pack_col(void* dst, int kind, int a0, int a1, double par);
void sindyfit_pack_design(void* dst, const void* cols, const void* pool, const void* tiles, double* part, double* G,
                          int nf, int w, int n_tiles);
void sindyfit_pack_desc(void* dst, int n, int tcol, int id, const double* g, long long ldg, long long ws,
                        long long out, double threshold);
int sindyfit_launch_gram(hipStream_t st, int R, int nx, int nu, const void* obs, const void* ctrls,
                         const void* ycont, const void* row_start, const void* designs, int n_designs,
                         int max_tiles, int max_wp, int max_entries);
int sindyfit_launch_solve(hipStream_t st, int n, const void* descs, const void* order, void* ws, void* coef,
                          void* bad, void* min_pivot, void* min_margin, void* iters, double alpha, int max_iter);

namespace {
struct Design {
  int nf = 0, w = 0, wp = 0, nfp = 0;
  bool disc = false, cont = false;
  int tcol_disc = 0, tcol_cont = 0;
  FitCols<int, int, int, double> cols{sindyfit_col_bytes(), sindyfit_pack_col};     // (kind, a0, a1, par)
  std::vector<int> pool, tiles;
  long long g_off = 0, part_off = 0;      // doubles
};
}  // namespace

extern "C" int ampc_sindy_fit(int device, int n_traj, const int* traj_len, int obs_dim, int ctrl_dim,
                              const double* obs, const double* ctrls, const double* ycont, int n_designs,
                              const int* feat_off, const int* pair_off, const int* kind, const int* a0, const int* a1,
                              const double* par, const int* pair_var, const int* pair_exp, int n_configs,
                              const int* cfg_design, const int* cfg_continuous, const double* cfg_threshold,
                              double alpha, int max_iter, double* coeffs, int* status, double* min_pivot,
                              double* min_margin, int* iterations) {
  REQUIRE(traj_len && obs && ctrls && coeffs && status && min_pivot && min_margin && iterations,
          "ampc_sindy_fit: NULL argument");
  REQUIRE(feat_off && pair_off && kind && a0 && a1 && par && pair_var && pair_exp, "ampc_sindy_fit: NULL library");
  REQUIRE(cfg_design && cfg_continuous && cfg_threshold, "ampc_sindy_fit: NULL configuration array");
  REQUIRE(n_traj >= 1, "ampc_sindy_fit: n_traj < 1");
  REQUIRE(obs_dim >= 1 && obs_dim <= sindyfit_max_state(), "ampc_sindy_fit: obs_dim must be in 1..64");
  REQUIRE(ctrl_dim >= 1 && ctrl_dim <= sindyfit_max_ctrl(), "ampc_sindy_fit: ctrl_dim must be in 1..16");
  REQUIRE(n_designs >= 1 && n_configs >= 1, "ampc_sindy_fit: no design or no configuration");
  REQUIRE(max_iter >= 1, "ampc_sindy_fit: max_iter < 1");
  REQUIRE(alpha >= 0.0 && std::isfinite(alpha), "ampc_sindy_fit: alpha must be finite and >= 0");
  const int nx = obs_dim, nu = ctrl_dim, nv = nx + nu;
  FitData data;
  if (int rc = data.index("ampc_sindy_fit", n_traj, traj_len)) return rc;
  const long long R = data.R;

  std::vector<Design> designs(n_designs);
  for (int c = 0; c < n_configs; ++c) {
    REQUIRE(cfg_design[c] >= 0 && cfg_design[c] < n_designs, "ampc_sindy_fit: configuration names no design");
    REQUIRE(cfg_threshold[c] >= 0.0 && std::isfinite(cfg_threshold[c]),
            "ampc_sindy_fit: threshold must be finite and >= 0");
    REQUIRE(!cfg_continuous[c] || ycont, "ampc_sindy_fit: a continuous configuration needs continuous targets");
    (cfg_continuous[c] ? designs[cfg_design[c]].cont : designs[cfg_design[c]].disc) = true;
  }
  REQUIRE(feat_off[0] == 0 && pair_off[0] == 0, "ampc_sindy_fit: offsets must start at 0");
  int max_tiles = 0, max_wp = 0, max_entries = 0;
  const int splits = data.splits;
  long long g_total = 0, part_total = 0;
  for (int di = 0; di < n_designs; ++di) {
    Design& d = designs[di];
    const int f0 = feat_off[di], p0 = pair_off[di], np = pair_off[di + 1] - p0;
    d.nf = feat_off[di + 1] - f0;
    REQUIRE(d.nf >= 1 && d.nf <= kFitMaxFeat, "ampc_sindy_fit: a design must have 1..272 features");
    REQUIRE(np >= 0, "ampc_sindy_fit: pair offsets must not decrease");
    for (int j = 0; j < np; ++j) {
      REQUIRE(pair_var[p0 + j] >= 0 && pair_var[p0 + j] < nv, "ampc_sindy_fit: monomial variable out of range");
      REQUIRE(pair_exp[p0 + j] >= 1 && pair_exp[p0 + j] <= 64, "ampc_sindy_fit: monomial exponents must be in 1..64");
      d.pool.push_back(pair_var[p0 + j]);
      d.pool.push_back(pair_exp[p0 + j]);
    }
    for (int k = f0; k < f0 + d.nf; ++k) {
      REQUIRE(kind[k] >= SF_ID && kind[k] <= SF_MONO, "ampc_sindy_fit: feature kind must be in 0..6");
      if (kind[k] == SF_MONO)
        REQUIRE(a0[k] >= 0 && a1[k] >= 1 && a1[k] <= 10 && a0[k] + a1[k] <= np,
                "ampc_sindy_fit: monomial feature names pairs outside its design's pool");
      else
        REQUIRE(a0[k] >= 0 && a0[k] < nv && a1[k] >= 0 && a1[k] < nv, "ampc_sindy_fit: feature variable out of range");
      REQUIRE(std::isfinite(par[k]), "ampc_sindy_fit: feature parameter not finite");
      d.cols.add(kind[k], a0[k], a1[k], par[k]);
    }
    d.tcol_disc = d.nf;
    d.tcol_cont = d.nf + (d.disc ? nx : 0);
    if (d.disc)
      for (int j = 0; j < nx; ++j) d.cols.add(sindyfit_next_obs_kind(), j, 0, 0.0);
    if (d.cont)
      for (int j = 0; j < nx; ++j) d.cols.add(sindyfit_ycont_kind(), j, 0, 0.0);
    d.w = d.cols.n;
    d.wp = d.cols.pad16(sindyfit_zero_kind(), 0, 0, 0.0);
    d.nfp = (d.nf + 15) / 16 * 16;
    if (d.pool.empty()) d.pool.assign(2, 0);
    d.tiles = upper_tiles(d.nfp, d.wp);
    max_tiles = std::max(max_tiles, (int)d.tiles.size());
    max_wp = std::max(max_wp, d.wp);
    max_entries = std::max(max_entries, d.nf * d.w);
    d.g_off = g_total;
    d.part_off = part_total;
    g_total += (long long)d.nfp * d.wp;
    part_total += (long long)splits * d.nfp * d.wp;
  }
  REQUIRE(part_total <= (1LL << 31), "ampc_sindy_fit: the Gram workspace would exceed 16 GiB (too many rows or designs)");

  // pairs (configuration, target), their workspace and output offsets
  const size_t dsz = sindyfit_desc_bytes();
  std::vector<long long> cfg_out(n_configs + 1, 0), cfg_pair(n_configs + 1, 0);
  long long ws = 0;
  for (int c = 0; c < n_configs; ++c) {
    const int nf = designs[cfg_design[c]].nf;
    cfg_out[c + 1] = cfg_out[c] + (long long)nx * nf;
    cfg_pair[c + 1] = cfg_pair[c] + nx;
    ws += (long long)nx * (nf + 1) * nf;
  }
  const int P = (int)cfg_pair[n_configs];
  REQUIRE(ws <= (1LL << 31), "ampc_sindy_fit: the solve workspace would exceed 16 GiB (too many configurations)");

  if (int rc = data.stage("ampc_sindy_fit", device, nx, nu, obs, ctrls, ycont)) return rc;
  hipStream_t st = data.sg.s;
  ScopedBuf d_part, d_g, d_designs, d_descs, d_order, d_ws, d_coef, d_bad, d_piv, d_mar, d_it;
  std::vector<ScopedBuf> d_cols(n_designs), d_pool(n_designs), d_tiles(n_designs);
  HIP_OK(d_part.reserve((size_t)part_total * 8));
  HIP_OK(d_g.reserve((size_t)g_total * 8));
  const size_t gsz = sindyfit_design_bytes();
  std::vector<char> dtab((size_t)n_designs * gsz);
  for (int i = 0; i < n_designs; ++i) {
    const Design& d = designs[i];
    if (int rc = fit_upload(d_cols[i], d.cols.bytes, st)) return rc;
    if (int rc = fit_upload(d_pool[i], d.pool, st)) return rc;
    if (int rc = fit_upload(d_tiles[i], d.tiles, st)) return rc;
    sindyfit_pack_design(dtab.data() + (size_t)i * gsz, d_cols[i].p, d_pool[i].p, d_tiles[i].p,
                         (double*)d_part.p + d.part_off, (double*)d_g.p + d.g_off, d.nf, d.w, (int)d.tiles.size());
  }
  if (int rc = fit_upload(d_designs, dtab, st)) return rc;
  if (int rc = sindyfit_launch_gram(st, (int)R, nx, nu, data.d_obs.p, data.d_ctrls.p, data.d_ycont.p,
                                    data.d_row_start.p, d_designs.p, n_designs, max_tiles, max_wp, max_entries))
    return rc;

  std::vector<char> descs((size_t)P * dsz);
  std::vector<int> pair_nf(P);
  long long wo = 0;
  for (int c = 0; c < n_configs; ++c) {
    const Design& d = designs[cfg_design[c]];
    const int tcol = cfg_continuous[c] ? d.tcol_cont : d.tcol_disc;
    for (int j = 0; j < nx; ++j) {
      const int id = (int)cfg_pair[c] + j;
      sindyfit_pack_desc(descs.data() + (size_t)id * dsz, d.nf, tcol + j, id, (const double*)d_g.p + d.g_off, d.wp,
                         wo, cfg_out[c] + (long long)j * d.nf, cfg_threshold[c]);
      pair_nf[id] = d.nf;
      wo += (long long)(d.nf + 1) * d.nf;
    }
  }
  // widest pair first: the first, all-features factorisation decides how long a workgroup runs
  std::vector<int> order(P);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return pair_nf[a] > pair_nf[b]; });
  const long long out = cfg_out[n_configs];
  if (int rc = fit_upload(d_descs, descs, st)) return rc;
  if (int rc = fit_upload(d_order, order, st)) return rc;
  HIP_OK(d_ws.reserve((size_t)ws * 8));
  HIP_OK(d_coef.reserve((size_t)out * 8));
  HIP_OK(d_bad.reserve((size_t)P * 4));
  HIP_OK(d_piv.reserve((size_t)P * 8));
  HIP_OK(d_mar.reserve((size_t)P * 8));
  HIP_OK(d_it.reserve((size_t)P * 4));
  if (int rc = sindyfit_launch_solve(st, P, d_descs.p, d_order.p, d_ws.p, d_coef.p, d_bad.p, d_piv.p, d_mar.p, d_it.p,
                                     alpha, max_iter))
    return rc;
  std::vector<int> bad(P), its(P);
  std::vector<double> piv(P), mar(P);
  HIP_OK(hipMemcpyAsync(coeffs, d_coef.p, (size_t)out * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(bad.data(), d_bad.p, (size_t)P * 4, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(piv.data(), d_piv.p, (size_t)P * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(mar.data(), d_mar.p, (size_t)P * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(its.data(), d_it.p, (size_t)P * 4, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  // a configuration's pairs folded in target order
  for (int c = 0; c < n_configs; ++c) {
    int any_bad = 0, it = 0;
    double p = INFINITY, m = INFINITY;
    for (long long i = cfg_pair[c]; i < cfg_pair[c + 1]; ++i) {
      any_bad |= bad[i];
      it = std::max(it, its[i]);
      if (piv[i] < p || piv[i] != piv[i]) p = piv[i];
      if (mar[i] < m) m = mar[i];
    }
    status[c] = any_bad ? 1 : (m < 0x1p-20 ? 2 : 0);
    min_pivot[c] = p;
    min_margin[c] = m;
    iterations[c] = it;
  }
  return 0;
}
