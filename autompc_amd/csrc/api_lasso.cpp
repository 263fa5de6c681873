// api_lasso.cpp -- ampc_lasso_fit: lasso fits of Koopman configurations (basis, alpha) of one data set in one call
// (reference: autompc/sysid/koopman.py:150-156, sklearn's Lasso with its defaults).  One Gram pass per basis over the
// design [1 | F | Y] (linfit_gram_kernel), centred through the constant column, then one wave per (configuration,
// target) runs the cyclic coordinate descent on it.  f64 only; kernels in lasso_kernels.hpp, launchers in
// launch_lasso.cpp.
#include "fit_host.hpp"

int linfit_launch_gram_part(hipStream_t st, int R, int no, int nu, const void* obs, const void* ctrls,
                            const void* row_start, const void* cols, const void* prog, const void* tiles, int n_tiles,
                            int wp, int nfp, void* part);
size_t lasso_design_bytes();
size_t lasso_pair_bytes();
void lasso_pack_design(void* dst, const double* part, double* G, double* Qt, double* yy, int* bad, int nf, int nt,
                       int wp, int ldp, int splits, double m);
void lasso_pack_pair(void* dst, const double* G, const double* q, const double* yy, const int* bad, double* out,
                     double alpha, int nf, int ldp, int id);
int lasso_launch_centre(hipStream_t st, const void* designs, int n_designs, int max_entries);
int lasso_launch_cd(hipStream_t st, int n_pairs, const void* pairs, void* status, void* margins, void* sweeps);

namespace {
struct Design {
  int nf = 0, nt = 0, wp = 0, ldp = 0;
  bool used = false;
  LinfitCols cols{linfit_col_bytes(), linfit_pack_col};
  std::vector<double> prog;
  std::vector<int> tiles;
  long long part_off = 0, g_off = 0, q_off = 0, yy_off = 0;      // doubles
};
}  // namespace

extern "C" int ampc_lasso_fit(int device, int n_traj, const int* traj_len, int obs_dim, int ctrl_dim,
                              const double* obs, const double* ctrls, int n_bases, const int* basis_n,
                              const int* basis_kinds, const double* basis_params, int n_configs,
                              const int* cfg_basis, const double* cfg_alpha, double tie, double ratio_tie,
                              double* coeffs, int* status, double* min_margin, int* sweeps) {
  REQUIRE(traj_len && obs && ctrls && coeffs && status && min_margin && sweeps, "ampc_lasso_fit: NULL argument");
  REQUIRE(basis_n && basis_kinds && basis_params && cfg_basis && cfg_alpha, "ampc_lasso_fit: NULL basis or configuration");
  REQUIRE(n_traj >= 1, "ampc_lasso_fit: n_traj < 1");
  REQUIRE(obs_dim >= 1 && obs_dim <= kFitMaxState, "ampc_lasso_fit: obs_dim must be in 1..256");
  REQUIRE(ctrl_dim >= 1 && ctrl_dim <= kFitMaxCtrl, "ampc_lasso_fit: ctrl_dim must be in 1..16");
  REQUIRE(n_bases >= 1 && n_configs >= 1, "ampc_lasso_fit: no basis or no configuration");
  REQUIRE(tie >= 0.0 && ratio_tie >= 0.0, "ampc_lasso_fit: tie margins must be >= 0");
  const int no = obs_dim, nu = ctrl_dim;
  FitData data;
  if (int rc = data.index("ampc_lasso_fit", n_traj, traj_len)) return rc;
  const long long R = data.R, design_rows = data.design_rows;

  std::vector<Design> designs(n_bases);
  for (int c = 0; c < n_configs; ++c) {
    REQUIRE(cfg_basis[c] >= 0 && cfg_basis[c] < n_bases, "ampc_lasso_fit: configuration names no basis");
    REQUIRE(cfg_alpha[c] >= 0.0 && std::isfinite(cfg_alpha[c]), "ampc_lasso_fit: alpha must be finite and >= 0");
    designs[cfg_basis[c]].used = true;
  }
  const int splits = data.splits;
  long long part_total = 0, g_total = 0, q_total = 0, yy_total = 0;
  int max_entries = 0;
  for (int b = 0, pos = 0; b < n_bases; ++b) {
    Design& d = designs[b];
    const int nb = basis_n[b];
    if (int rc = koopman_basis_program("ampc_lasso_fit", nb, basis_kinds + pos, basis_params + pos, no, d.prog))
      return rc;
    pos += nb;
    if (!d.used) continue;
    const int n = nb * no;
    d.nf = n + nu;
    d.nt = n;
    d.cols.add(0, 0, 0, -1);                                       // the constant column
    koopman_columns(d.cols, d.prog, no, nu);
    d.wp = d.cols.pad16(0, -2, 0, -1);
    d.ldp = (d.nf + 63) / 64 * 64;
    // tile rows of [1 | F] against every column on and right of the diagonal; of Y the diagonal tiles
    const int frows = (1 + d.nf + 15) / 16;
    for (int ti = 0; ti < d.wp / 16; ++ti)
      for (int tj = ti; tj < (ti < frows ? d.wp / 16 : ti + 1); ++tj) d.tiles.push_back(ti | (tj << 16));
    d.part_off = part_total; d.g_off = g_total; d.q_off = q_total; d.yy_off = yy_total;
    part_total += (long long)splits * d.wp * d.wp;
    g_total += (long long)d.nf * d.ldp;
    q_total += (long long)d.nt * d.ldp;
    yy_total += d.nt;
    max_entries = std::max(max_entries, (d.nf + d.nt) * d.ldp + d.nt);
  }
  REQUIRE(part_total <= (1LL << 31), "ampc_lasso_fit: the Gram workspace would exceed 16 GiB (too many rows or bases)");

  std::vector<long long> cfg_out(n_configs + 1, 0), cfg_pair(n_configs + 1, 0);
  for (int c = 0; c < n_configs; ++c) {
    const Design& d = designs[cfg_basis[c]];
    cfg_out[c + 1] = cfg_out[c] + (long long)d.nt * d.nf;
    cfg_pair[c + 1] = cfg_pair[c] + d.nt;
  }
  REQUIRE(cfg_pair[n_configs] < (1LL << 24), "ampc_lasso_fit: too many (configuration, target) pairs");
  const int P = (int)cfg_pair[n_configs];
  const long long out = cfg_out[n_configs];

  if (int rc = data.stage("ampc_lasso_fit", device, no, nu, obs, ctrls, nullptr)) return rc;
  hipStream_t st = data.sg.s;
  ScopedBuf d_part, d_g, d_q, d_yy, d_bad, d_designs, d_pairs, d_coef, d_status, d_mar, d_it;
  std::vector<ScopedBuf> d_cols(n_bases), d_prog(n_bases), d_tiles(n_bases);
  HIP_OK(d_part.reserve((size_t)part_total * 8));
  HIP_OK(d_g.reserve((size_t)g_total * 8));
  HIP_OK(d_q.reserve((size_t)q_total * 8));
  HIP_OK(d_yy.reserve((size_t)yy_total * 8));
  HIP_OK(d_bad.reserve((size_t)n_bases * 4));
  HIP_OK(hipMemsetAsync(d_bad.p, 0, (size_t)n_bases * 4, st));
  const size_t gsz = lasso_design_bytes();
  std::vector<char> dtab;
  std::vector<int> design_slot(n_bases, -1);
  for (int b = 0; b < n_bases; ++b) {
    const Design& d = designs[b];
    if (!d.used) continue;
    if (int rc = fit_upload(d_cols[b], d.cols.bytes, st)) return rc;
    if (int rc = fit_upload(d_prog[b], d.prog, st)) return rc;
    if (int rc = fit_upload(d_tiles[b], d.tiles, st)) return rc;
    if (int rc = linfit_launch_gram_part(st, (int)R, no, nu, data.d_obs.p, data.d_ctrls.p, data.d_row_start.p,
                                         d_cols[b].p, d_prog[b].p, d_tiles[b].p, (int)d.tiles.size(), d.wp, d.wp,
                                         (double*)d_part.p + d.part_off))
      return rc;
    design_slot[b] = (int)(dtab.size() / gsz);
    dtab.resize(dtab.size() + gsz);
    lasso_pack_design(dtab.data() + dtab.size() - gsz, (const double*)d_part.p + d.part_off,
                      (double*)d_g.p + d.g_off, (double*)d_q.p + d.q_off, (double*)d_yy.p + d.yy_off,
                      (int*)d_bad.p + b, d.nf, d.nt, d.wp, d.ldp, splits, (double)design_rows);
  }
  if (int rc = fit_upload(d_designs, dtab, st)) return rc;
  if (int rc = lasso_launch_centre(st, d_designs.p, (int)(dtab.size() / gsz), max_entries)) return rc;

  const size_t psz = lasso_pair_bytes();
  std::vector<char> pairs((size_t)P * psz);
  HIP_OK(d_coef.reserve((size_t)out * 8));
  for (int c = 0; c < n_configs; ++c) {
    const int b = cfg_basis[c];
    const Design& d = designs[b];
    for (int t = 0; t < d.nt; ++t) {
      const int id = (int)cfg_pair[c] + t;
      lasso_pack_pair(pairs.data() + (size_t)id * psz, (const double*)d_g.p + d.g_off,
                      (const double*)d_q.p + d.q_off + (long long)t * d.ldp, (const double*)d_yy.p + d.yy_off + t,
                      (const int*)d_bad.p + b, (double*)d_coef.p + cfg_out[c] + (long long)t * d.nf,
                      cfg_alpha[c] * (double)design_rows, d.nf, d.ldp, id);
    }
  }
  if (int rc = fit_upload(d_pairs, pairs, st)) return rc;
  HIP_OK(d_status.reserve((size_t)P * 4));
  HIP_OK(d_mar.reserve((size_t)P * 16));
  HIP_OK(d_it.reserve((size_t)P * 4));
  if (int rc = lasso_launch_cd(st, P, d_pairs.p, d_status.p, d_mar.p, d_it.p)) return rc;
  std::vector<int> bad(P), its(P);
  std::vector<double> mar((size_t)2 * P);
  HIP_OK(hipMemcpyAsync(coeffs, d_coef.p, (size_t)out * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(bad.data(), d_status.p, (size_t)P * 4, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(mar.data(), d_mar.p, (size_t)P * 16, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(its.data(), d_it.p, (size_t)P * 4, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  // a configuration's pairs folded in target order
  for (int c = 0; c < n_configs; ++c) {
    int any_bad = 0, it = 0;
    double mg = INFINITY, mr = INFINITY;
    for (long long i = cfg_pair[c]; i < cfg_pair[c + 1]; ++i) {
      any_bad |= bad[i];
      it = std::max(it, its[i]);
      if (mar[2 * i] < mg) mg = mar[2 * i];
      if (mar[2 * i + 1] < mr) mr = mar[2 * i + 1];
    }
    status[c] = any_bad ? 1 : ((mg <= tie || mr <= ratio_tie) ? 2 : 0);
    min_margin[2 * c] = mg;
    min_margin[2 * c + 1] = mr;
    sweeps[c] = any_bad ? 0 : it;
  }
  return 0;
}
