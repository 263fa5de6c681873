// api_stable.cpp -- ampc_stable_fit: stable fits of Koopman configurations (one per basis) of one data set in one call
// (reference: autompc/sysid/stable_koopman.py:47-167 stabilize_discrete with its default initialisation).  One Gram
// pass per basis over the design [F | Y] (linfit_gram_kernel), the least-squares start by linfit_solve_kernel, then
// one workgroup per basis runs the projected fast-gradient iteration on the Gram.  f64 only; kernels in
// stable_kernels.hpp, launchers in launch_stable.cpp.
#include "fit_host.hpp"

int linfit_launch_gram_part(hipStream_t st, int R, int no, int nu, const void* obs, const void* ctrls,
                            const void* row_start, const void* cols, const void* prog, const void* tiles, int n_tiles,
                            int wp, int nfp, void* part);
size_t linfit_desc_bytes();
void linfit_pack_desc(void* dst, int n, int nt, int tcol, int id, const double* g, long long ldg, long long idx,
                      long long ws, long long out);
int linfit_launch_solve(hipStream_t st, int n, const void* descs, const void* order, const void* idx, void* ws,
                        void* coef, void* status, void* min_pivot);
size_t stable_desc_bytes();
int stable_max_n();
long long stable_scratch_doubles(int n, int nu);
void stable_pack_desc(void* dst, const double* G, const double* W0, const double* yy, const int* w0_status, double* ws,
                      double* out, double tie, int n, int nu, int ldg, int id);
int stable_launch_gram(hipStream_t st, const void* part, void* G, void* yy, int splits, int nf, int nt, int wp);
int stable_launch_fgm(hipStream_t st, int n_configs, const void* descs, void* status, void* error, void* iterations,
                      void* trials, void* margin);

namespace {
struct Design {
  int n = 0, nf = 0, wp = 0;
  LinfitCols cols{linfit_col_bytes(), linfit_pack_col};
  std::vector<double> prog;
  std::vector<int> tiles;
  long long part_off = 0, g_off = 0, yy_off = 0, w0_off = 0, lws_off = 0, ws_off = 0, idx_off = 0;      // doubles / ints
};
}  // namespace

extern "C" int ampc_stable_fit(int device, int n_traj, const int* traj_len, int obs_dim, int ctrl_dim,
                               const double* obs, const double* ctrls, int n_bases, const int* basis_n,
                               const int* basis_kinds, const double* basis_params, double tie, double* coeffs,
                               int* status, double* error, int* iterations, int* trials, double* min_margin) {
  REQUIRE(traj_len && obs && ctrls && coeffs && status && error && iterations && trials && min_margin,
          "ampc_stable_fit: NULL argument");
  REQUIRE(basis_n && basis_kinds && basis_params, "ampc_stable_fit: NULL basis");
  REQUIRE(n_traj >= 1, "ampc_stable_fit: n_traj < 1");
  REQUIRE(obs_dim >= 1 && obs_dim <= stable_max_n(), "ampc_stable_fit: obs_dim must be in 1..64");
  REQUIRE(ctrl_dim >= 1 && ctrl_dim <= kFitMaxCtrl, "ampc_stable_fit: ctrl_dim must be in 1..16");
  REQUIRE(n_bases >= 1, "ampc_stable_fit: no basis");
  REQUIRE(tie >= 0.0, "ampc_stable_fit: the tie margin must be >= 0");
  const int no = obs_dim, nu = ctrl_dim;
  FitData data;
  if (int rc = data.index("ampc_stable_fit", n_traj, traj_len)) return rc;
  const long long R = data.R;
  const int splits = data.splits;

  std::vector<Design> designs(n_bases);
  long long part_total = 0, g_total = 0, yy_total = 0, w0_total = 0, lws_total = 0, ws_total = 0, idx_total = 0;
  for (int b = 0, pos = 0; b < n_bases; ++b) {
    Design& d = designs[b];
    const int nb = basis_n[b];
    REQUIRE(nb >= 1 && (long long)nb * no <= stable_max_n(),
            "ampc_stable_fit: a Koopman lift (n_basis * obs_dim) must have 1..64 states");
    if (int rc = koopman_basis_program("ampc_stable_fit", nb, basis_kinds + pos, basis_params + pos, no, d.prog))
      return rc;
    pos += nb;
    d.n = nb * no;
    d.nf = d.n + nu;
    koopman_columns(d.cols, d.prog, no, nu);
    d.wp = d.cols.pad16(0, -2, 0, -1);
    // tile rows of F against every column on and right of the diagonal; of Y the diagonal tiles
    const int frows = (d.nf + 15) / 16;
    for (int ti = 0; ti < d.wp / 16; ++ti)
      for (int tj = ti; tj < (ti < frows ? d.wp / 16 : ti + 1); ++tj) d.tiles.push_back(ti | (tj << 16));
    d.part_off = part_total; d.g_off = g_total; d.yy_off = yy_total; d.w0_off = w0_total; d.lws_off = lws_total;
    d.ws_off = ws_total; d.idx_off = idx_total;
    part_total += (long long)splits * d.wp * d.wp;
    g_total += (long long)d.nf * d.wp;
    yy_total += d.n;
    w0_total += (long long)d.n * d.nf;
    lws_total += (long long)(d.nf + d.n) * d.nf;
    ws_total += stable_scratch_doubles(d.n, nu);
    idx_total += d.nf;
  }
  REQUIRE(part_total <= (1LL << 31), "ampc_stable_fit: the Gram workspace would exceed 16 GiB (too many rows or bases)");

  if (int rc = data.stage("ampc_stable_fit", device, no, nu, obs, ctrls, nullptr)) return rc;
  hipStream_t st = data.sg.s;
  ScopedBuf d_part, d_g, d_yy, d_w0, d_lws, d_ws, d_ldescs, d_order, d_idx, d_lstatus, d_piv, d_descs, d_coef, d_status,
      d_err, d_it, d_tr, d_mar;
  std::vector<ScopedBuf> d_cols(n_bases), d_prog(n_bases), d_tiles(n_bases);
  HIP_OK(d_part.reserve((size_t)part_total * 8));
  HIP_OK(d_g.reserve((size_t)g_total * 8));
  HIP_OK(d_yy.reserve((size_t)yy_total * 8));
  HIP_OK(d_w0.reserve((size_t)w0_total * 8));
  HIP_OK(d_lws.reserve((size_t)lws_total * 8));
  HIP_OK(d_ws.reserve((size_t)ws_total * 8));
  HIP_OK(d_coef.reserve((size_t)w0_total * 8));
  HIP_OK(d_lstatus.reserve((size_t)n_bases * 4));
  HIP_OK(d_piv.reserve((size_t)n_bases * 8));
  HIP_OK(d_status.reserve((size_t)n_bases * 4));
  HIP_OK(d_err.reserve((size_t)n_bases * 8));
  HIP_OK(d_it.reserve((size_t)n_bases * 4));
  HIP_OK(d_tr.reserve((size_t)n_bases * 4));
  HIP_OK(d_mar.reserve((size_t)n_bases * 8));
  const size_t lsz = linfit_desc_bytes(), ssz = stable_desc_bytes();
  std::vector<char> ldescs((size_t)n_bases * lsz), sdescs((size_t)n_bases * ssz);
  std::vector<int> order(n_bases), idx;
  for (int b = 0; b < n_bases; ++b) {
    const Design& d = designs[b];
    if (int rc = fit_upload(d_cols[b], d.cols.bytes, st)) return rc;
    if (int rc = fit_upload(d_prog[b], d.prog, st)) return rc;
    if (int rc = fit_upload(d_tiles[b], d.tiles, st)) return rc;
    double* part = (double*)d_part.p + d.part_off;
    double* G = (double*)d_g.p + d.g_off;
    double* yy = (double*)d_yy.p + d.yy_off;
    if (int rc = linfit_launch_gram_part(st, (int)R, no, nu, data.d_obs.p, data.d_ctrls.p, data.d_row_start.p,
                                         d_cols[b].p, d_prog[b].p, d_tiles[b].p, (int)d.tiles.size(), d.wp, d.wp, part))
      return rc;
    if (int rc = stable_launch_gram(st, part, G, yy, splits, d.nf, d.n, d.wp)) return rc;
    linfit_pack_desc(ldescs.data() + (size_t)b * lsz, d.nf, d.n, d.nf, b, G, d.wp, d.idx_off, d.lws_off, d.w0_off);
    stable_pack_desc(sdescs.data() + (size_t)b * ssz, G, (const double*)d_w0.p + d.w0_off, yy,
                     (const int*)d_lstatus.p + b, (double*)d_ws.p + d.ws_off, (double*)d_coef.p + d.w0_off, tie, d.n, nu,
                     d.wp, b);
    order[b] = b;
    for (int j = 0; j < d.nf; ++j) idx.push_back(j);
  }
  if (int rc = fit_upload(d_ldescs, ldescs, st)) return rc;
  if (int rc = fit_upload(d_order, order, st)) return rc;
  if (int rc = fit_upload(d_idx, idx, st)) return rc;
  if (int rc = fit_upload(d_descs, sdescs, st)) return rc;
  if (int rc = linfit_launch_solve(st, n_bases, d_ldescs.p, d_order.p, d_idx.p, d_lws.p, d_w0.p, d_lstatus.p, d_piv.p))
    return rc;
  if (int rc = stable_launch_fgm(st, n_bases, d_descs.p, d_status.p, d_err.p, d_it.p, d_tr.p, d_mar.p)) return rc;
  HIP_OK(hipMemcpyAsync(coeffs, d_coef.p, (size_t)w0_total * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(status, d_status.p, (size_t)n_bases * 4, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(error, d_err.p, (size_t)n_bases * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(iterations, d_it.p, (size_t)n_bases * 4, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(trials, d_tr.p, (size_t)n_bases * 4, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(min_margin, d_mar.p, (size_t)n_bases * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  return 0;
}
