// api_sindyfit.cpp -- ampc_sindy_fit / ampc_sindy_fit_wide: sequentially-thresholded least-squares fits of SINDy configurations of one data
// set in one call (what sysid/sindy.py SINDy.train does per model on the host).  One Gram launch for all designs
// (distinct feature libraries) -- a configuration's every iteration and target only needs a sub-matrix of its
// design's Gram Theta'[Theta | Y] -- then one solve workgroup per (configuration, target).
// f64 only; kernels in sindyfit_kernels.hpp, launchers in launch_sindyfit.cpp.
// ampc_sindy_fit_wide is the same call for designs of up to 2048 features on the kernels of sindyfit_wide_kernels.hpp
// (launch_sindyfit_wide.cpp): the Gram pass and the solve run in waves under a memory budget of AMPC_SINDY_WIDE_BUDGET_MB
// MiB (default 8192) for the Grams, the materialised [Theta | Y] of a wave and the workspaces of a wave's pairs.  A
// Gram wave is a list of (design, run of row splits): the running sum of a design's tile is continued from G in split
// order, so its bits do not depend on the cut; a solve wave is a run of the width-sorted pairs, which are independent.
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
size_t sindyfit_wide_design_bytes();
size_t sindyfit_wide_item_bytes();
int sindyfit_wide_max_feat();
int sindyfit_wide_acc();
void sindyfit_wide_pack_design(void* dst, const void* cols, const void* pool, const void* groups, double* G, int nf,
                               int w, int n_groups);
void sindyfit_wide_pack_item(void* dst, int design, int s0, int s1, int first, long long theta);
int sindyfit_wide_launch_gram(hipStream_t st, int R, int nx, int nu, const void* obs, const void* ctrls,
                              const void* ycont, const void* row_start, const void* designs, const void* items,
                              int n_items, int max_splits, int max_wp, int max_groups, void* theta);
int sindyfit_wide_launch_solve(hipStream_t st, int first, int count, int maxn, const void* descs, const void* order,
                               void* ws, void* coef, void* bad, void* min_pivot, void* min_margin, void* iters,
                               double alpha, int max_iter);

namespace {
struct Design {
  int nf = 0, w = 0, wp = 0, nfp = 0;
  bool disc = false, cont = false;
  int tcol_disc = 0, tcol_cont = 0;
  FitCols<int, int, int, double> cols{sindyfit_col_bytes(), sindyfit_pack_col};     // (kind, a0, a1, par)
  std::vector<int> pool, tiles;           // tiles: the wide call's groups (ti | first tj << 16) instead
  long long g_off = 0, part_off = 0;      // doubles
};

// A wave of the wide Gram pass: items [i0, i1) of the call's item list.
struct GramWave {
  int i0 = 0, i1 = 0, max_splits = 0, max_wp = 0, max_groups = 0;
};

// Tile row and first tile column of every wave's run of up to `acc` tiles on or right of the diagonal.
std::vector<int> upper_groups(int nfp, int wp, int acc) {
  std::vector<int> groups;
  for (int ti = 0; ti < nfp / 16; ++ti)
    for (int tj = ti; tj < wp / 16; tj += acc) groups.push_back(ti | (tj << 16));
  return groups;
}
}  // namespace

static int sindy_fit_call(const bool wide, int device, int n_traj, const int* traj_len, int obs_dim, int ctrl_dim,
                              const double* obs, const double* ctrls, const double* ycont, int n_designs,
                              const int* feat_off, const int* pair_off, const int* kind, const int* a0, const int* a1,
                              const double* par, const int* pair_var, const int* pair_exp, int n_configs,
                              const int* cfg_design, const int* cfg_continuous, const double* cfg_threshold,
                              double alpha, int max_iter, double* coeffs, int* status, double* min_pivot,
                              double* min_margin, int* iterations) {
  const std::string nm = wide ? "ampc_sindy_fit_wide" : "ampc_sindy_fit";
  REQUIRE(traj_len && obs && ctrls && coeffs && status && min_pivot && min_margin && iterations,
          nm + ": NULL argument");
  REQUIRE(feat_off && pair_off && kind && a0 && a1 && par && pair_var && pair_exp, nm + ": NULL library");
  REQUIRE(cfg_design && cfg_continuous && cfg_threshold, nm + ": NULL configuration array");
  REQUIRE(n_traj >= 1, nm + ": n_traj < 1");
  REQUIRE(obs_dim >= 1 && obs_dim <= sindyfit_max_state(), nm + ": obs_dim must be in 1..64");
  REQUIRE(ctrl_dim >= 1 && ctrl_dim <= sindyfit_max_ctrl(), nm + ": ctrl_dim must be in 1..16");
  REQUIRE(n_designs >= 1 && n_configs >= 1, nm + ": no design or no configuration");
  REQUIRE(max_iter >= 1, nm + ": max_iter < 1");
  REQUIRE(alpha >= 0.0 && std::isfinite(alpha), nm + ": alpha must be finite and >= 0");
  const int nx = obs_dim, nu = ctrl_dim, nv = nx + nu;
  FitData data;
  if (int rc = data.index(nm, n_traj, traj_len)) return rc;
  const long long R = data.R;

  std::vector<Design> designs(n_designs);
  for (int c = 0; c < n_configs; ++c) {
    REQUIRE(cfg_design[c] >= 0 && cfg_design[c] < n_designs, nm + ": configuration names no design");
    REQUIRE(cfg_threshold[c] >= 0.0 && std::isfinite(cfg_threshold[c]),
            nm + ": threshold must be finite and >= 0");
    REQUIRE(!cfg_continuous[c] || ycont, nm + ": a continuous configuration needs continuous targets");
    (cfg_continuous[c] ? designs[cfg_design[c]].cont : designs[cfg_design[c]].disc) = true;
  }
  REQUIRE(feat_off[0] == 0 && pair_off[0] == 0, nm + ": offsets must start at 0");
  int max_tiles = 0, max_wp = 0, max_entries = 0;
  const int splits = data.splits;
  long long g_total = 0, part_total = 0;
  for (int di = 0; di < n_designs; ++di) {
    Design& d = designs[di];
    const int f0 = feat_off[di], p0 = pair_off[di], np = pair_off[di + 1] - p0;
    d.nf = feat_off[di + 1] - f0;
    REQUIRE(d.nf >= 1 && d.nf <= (wide ? sindyfit_wide_max_feat() : kFitMaxFeat),
            nm + (wide ? ": a design must have 1..2048 features" : ": a design must have 1..272 features"));
    REQUIRE(np >= 0, nm + ": pair offsets must not decrease");
    for (int j = 0; j < np; ++j) {
      REQUIRE(pair_var[p0 + j] >= 0 && pair_var[p0 + j] < nv, nm + ": monomial variable out of range");
      REQUIRE(pair_exp[p0 + j] >= 1 && pair_exp[p0 + j] <= 64, nm + ": monomial exponents must be in 1..64");
      d.pool.push_back(pair_var[p0 + j]);
      d.pool.push_back(pair_exp[p0 + j]);
    }
    for (int k = f0; k < f0 + d.nf; ++k) {
      REQUIRE(kind[k] >= SF_ID && kind[k] <= SF_MONO, nm + ": feature kind must be in 0..6");
      if (kind[k] == SF_MONO)
        REQUIRE(a0[k] >= 0 && a1[k] >= 1 && a1[k] <= 10 && a0[k] + a1[k] <= np,
                nm + ": monomial feature names pairs outside its design's pool");
      else
        REQUIRE(a0[k] >= 0 && a0[k] < nv && a1[k] >= 0 && a1[k] < nv, nm + ": feature variable out of range");
      REQUIRE(std::isfinite(par[k]), nm + ": feature parameter not finite");
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
    d.tiles = wide ? upper_groups(d.nfp, d.wp, sindyfit_wide_acc()) : upper_tiles(d.nfp, d.wp);
    max_tiles = std::max(max_tiles, (int)d.tiles.size());
    max_wp = std::max(max_wp, d.wp);
    max_entries = std::max(max_entries, d.nf * d.w);
    d.g_off = g_total;
    d.part_off = part_total;
    g_total += (long long)d.nfp * d.wp;
    part_total += (long long)splits * d.nfp * d.wp;
  }
  REQUIRE(wide || part_total <= (1LL << 31), nm + ": the Gram workspace would exceed 16 GiB (too many rows or designs)");

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
  REQUIRE(wide || ws <= (1LL << 31), nm + ": the solve workspace would exceed 16 GiB (too many configurations)");

  if (int rc = data.stage(nm, device, nx, nu, obs, ctrls, ycont)) return rc;
  hipStream_t st = data.sg.s;
  ScopedBuf d_part, d_g, d_designs, d_descs, d_order, d_ws, d_coef, d_bad, d_piv, d_mar, d_it, d_items, d_theta;
  std::vector<ScopedBuf> d_cols(n_designs), d_pool(n_designs), d_tiles(n_designs);
  // the wide call's budget (doubles) for the Grams plus the scratch of one wave
  const long long budget = (long long)std::max(1, env_int("AMPC_SINDY_WIDE_BUDGET_MB", 8192)) * (1LL << 17);
  REQUIRE(!wide || g_total <= budget, nm + ": the Grams alone would exceed the memory budget (too many designs)");
  const long long scratch = budget - g_total;     // a wave holds one split of one design / one pair at the least
  if (!wide) HIP_OK(d_part.reserve((size_t)part_total * 8));
  HIP_OK(d_g.reserve((size_t)g_total * 8));
  const size_t gsz = wide ? sindyfit_wide_design_bytes() : sindyfit_design_bytes();
  std::vector<char> dtab((size_t)n_designs * gsz);
  for (int i = 0; i < n_designs; ++i) {
    const Design& d = designs[i];
    if (int rc = fit_upload(d_cols[i], d.cols.bytes, st)) return rc;
    if (int rc = fit_upload(d_pool[i], d.pool, st)) return rc;
    if (int rc = fit_upload(d_tiles[i], d.tiles, st)) return rc;
    if (wide)
      sindyfit_wide_pack_design(dtab.data() + (size_t)i * gsz, d_cols[i].p, d_pool[i].p, d_tiles[i].p,
                                (double*)d_g.p + d.g_off, d.nf, d.w, (int)d.tiles.size());
    else
      sindyfit_pack_design(dtab.data() + (size_t)i * gsz, d_cols[i].p, d_pool[i].p, d_tiles[i].p,
                           (double*)d_part.p + d.part_off, (double*)d_g.p + d.g_off, d.nf, d.w, (int)d.tiles.size());
  }
  if (int rc = fit_upload(d_designs, dtab, st)) return rc;
  if (!wide) {
    if (int rc = sindyfit_launch_gram(st, (int)R, nx, nu, data.d_obs.p, data.d_ctrls.p, data.d_ycont.p,
                                      data.d_row_start.p, d_designs.p, n_designs, max_tiles, max_wp, max_entries))
      return rc;
  } else {
    // Gram waves: designs in order, each as runs of row splits; a design that continues does so in the next wave
    // (its running sum is read back from G), so no wave holds two runs of one design
    const size_t isz = sindyfit_wide_item_bytes();
    std::vector<char> items;
    std::vector<GramWave> waves(1);
    long long used = 0, theta_max = 0;
    auto flush = [&]() {
      GramWave& w = waves.back();
      if (w.i1 == w.i0) return;
      theta_max = std::max(theta_max, used);
      used = 0;
      GramWave next;
      next.i0 = next.i1 = w.i1;
      waves.push_back(next);
    };
    for (int di = 0; di < n_designs; ++di) {
      const Design& d = designs[di];
      const long long slab = (long long)kFitSplitRows * d.wp;
      for (int s = 0; s < splits;) {
        const long long fit = (scratch - used) / slab;
        if (fit < 1 && waves.back().i1 > waves.back().i0) { flush(); continue; }
        const int take = (int)std::max(1LL, std::min({fit, (long long)(splits - s), 1024LL}));
        items.resize(items.size() + isz);
        sindyfit_wide_pack_item(items.data() + items.size() - isz, di, s, s + take, s == 0 ? 1 : 0, used);
        GramWave& w = waves.back();
        ++w.i1;
        w.max_splits = std::max(w.max_splits, take);
        w.max_wp = std::max(w.max_wp, d.wp);
        w.max_groups = std::max(w.max_groups, (int)d.tiles.size());
        used += take * slab;
        s += take;
        if (s < splits || w.i1 - w.i0 == 65535) flush();
      }
    }
    flush();
    if (int rc = fit_upload(d_items, items, st)) return rc;
    HIP_OK(d_theta.reserve((size_t)theta_max * 8));
    for (const GramWave& w : waves) {
      if (w.i1 == w.i0) continue;
      if (int rc = sindyfit_wide_launch_gram(st, (int)R, nx, nu, data.d_obs.p, data.d_ctrls.p, data.d_ycont.p,
                                             data.d_row_start.p, d_designs.p, (const char*)d_items.p + w.i0 * isz,
                                             w.i1 - w.i0, w.max_splits, w.max_wp, w.max_groups, d_theta.p))
        return rc;
    }
  }

  std::vector<int> pair_nf(P);
  for (int c = 0; c < n_configs; ++c)
    for (int j = 0; j < nx; ++j) pair_nf[cfg_pair[c] + j] = designs[cfg_design[c]].nf;
  // widest pair first: the first, all-features factorisation decides how long a workgroup runs
  std::vector<int> order(P);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return pair_nf[a] > pair_nf[b]; });
  // workspace offsets: the narrow call holds all pairs' at once; the wide call cuts the sorted pairs into waves whose
  // workspaces fit the budget and reuses the buffer (first pair of every wave in wave_first)
  std::vector<long long> pair_ws(P);
  std::vector<int> wave_first;
  if (!wide) {
    long long wo = 0;
    for (int id = 0; id < P; ++id) { pair_ws[id] = wo; wo += (long long)(pair_nf[id] + 1) * pair_nf[id]; }
  } else {
    long long wo = 0;
    ws = 0;
    for (int k = 0; k < P; ++k) {
      const long long need = (long long)(pair_nf[order[k]] + 1) * pair_nf[order[k]];
      if (k == 0 || wo + need > scratch) { wave_first.push_back(k); wo = 0; }
      pair_ws[order[k]] = wo;
      wo += need;
      ws = std::max(ws, wo);
    }
    wave_first.push_back(P);
  }
  std::vector<char> descs((size_t)P * dsz);
  for (int c = 0; c < n_configs; ++c) {
    const Design& d = designs[cfg_design[c]];
    const int tcol = cfg_continuous[c] ? d.tcol_cont : d.tcol_disc;
    for (int j = 0; j < nx; ++j) {
      const int id = (int)cfg_pair[c] + j;
      sindyfit_pack_desc(descs.data() + (size_t)id * dsz, d.nf, tcol + j, id, (const double*)d_g.p + d.g_off, d.wp,
                         pair_ws[id], cfg_out[c] + (long long)j * d.nf, cfg_threshold[c]);
    }
  }
  const long long out = cfg_out[n_configs];
  if (int rc = fit_upload(d_descs, descs, st)) return rc;
  if (int rc = fit_upload(d_order, order, st)) return rc;
  HIP_OK(d_ws.reserve((size_t)ws * 8));
  HIP_OK(d_coef.reserve((size_t)out * 8));
  HIP_OK(d_bad.reserve((size_t)P * 4));
  HIP_OK(d_piv.reserve((size_t)P * 8));
  HIP_OK(d_mar.reserve((size_t)P * 8));
  HIP_OK(d_it.reserve((size_t)P * 4));
  if (!wide) {
    if (int rc = sindyfit_launch_solve(st, P, d_descs.p, d_order.p, d_ws.p, d_coef.p, d_bad.p, d_piv.p, d_mar.p,
                                       d_it.p, alpha, max_iter))
      return rc;
  } else {
    for (size_t w = 0; w + 1 < wave_first.size(); ++w) {
      const int k0 = wave_first[w], k1 = wave_first[w + 1];
      if (int rc = sindyfit_wide_launch_solve(st, k0, k1 - k0, pair_nf[order[k0]], d_descs.p, d_order.p, d_ws.p,
                                              d_coef.p, d_bad.p, d_piv.p, d_mar.p, d_it.p, alpha, max_iter))
        return rc;
    }
  }
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

extern "C" int ampc_sindy_fit(int device, int n_traj, const int* traj_len, int obs_dim, int ctrl_dim,
                              const double* obs, const double* ctrls, const double* ycont, int n_designs,
                              const int* feat_off, const int* pair_off, const int* kind, const int* a0, const int* a1,
                              const double* par, const int* pair_var, const int* pair_exp, int n_configs,
                              const int* cfg_design, const int* cfg_continuous, const double* cfg_threshold,
                              double alpha, int max_iter, double* coeffs, int* status, double* min_pivot,
                              double* min_margin, int* iterations) {
  return sindy_fit_call(false, device, n_traj, traj_len, obs_dim, ctrl_dim, obs, ctrls, ycont, n_designs, feat_off,
                        pair_off, kind, a0, a1, par, pair_var, pair_exp, n_configs, cfg_design, cfg_continuous,
                        cfg_threshold, alpha, max_iter, coeffs, status, min_pivot, min_margin, iterations);
}

extern "C" int ampc_sindy_fit_wide(int device, int n_traj, const int* traj_len, int obs_dim, int ctrl_dim,
                                   const double* obs, const double* ctrls, const double* ycont, int n_designs,
                                   const int* feat_off, const int* pair_off, const int* kind, const int* a0,
                                   const int* a1, const double* par, const int* pair_var, const int* pair_exp,
                                   int n_configs, const int* cfg_design, const int* cfg_continuous,
                                   const double* cfg_threshold, double alpha, int max_iter, double* coeffs, int* status,
                                   double* min_pivot, double* min_margin, int* iterations) {
  return sindy_fit_call(true, device, n_traj, traj_len, obs_dim, ctrl_dim, obs, ctrls, ycont, n_designs, feat_off,
                        pair_off, kind, a0, a1, par, pair_var, pair_exp, n_configs, cfg_design, cfg_continuous,
                        cfg_threshold, alpha, max_iter, coeffs, status, min_pivot, min_margin, iterations);
}
