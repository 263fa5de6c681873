// api_linfit.cpp -- ampc_linfit_fit: least-squares fits of ARX and Koopman(lstsq) configurations of one data set in one
// call (reference: autompc/sysid/arx.py:62-116 ARX.train, koopman.py:141-154 Koopman.train).  One Gram pass per
// design -- the ARX design of the longest history asked for holds every shorter history's normal equations as a
// sub-matrix; Koopman configurations of one basis share a design -- then one solve workgroup per configuration.
// f64 only; kernels in linfit_kernels.hpp, launchers in launch_linfit.cpp.
#include "fit_host.hpp"

size_t linfit_desc_bytes();
void linfit_pack_desc(void* dst, int n, int nt, int tcol, int id, const double* g, long long ldg, long long idx,
                      long long ws, long long out);
int linfit_launch_gram(hipStream_t st, int R, int no, int nu, const void* obs, const void* ctrls,
                       const void* row_start, const void* cols, const void* prog, const void* tiles, int n_tiles,
                       int nf, int nt, void* part, void* G);
int linfit_launch_solve(hipStream_t st, int n, const void* descs, const void* order, const void* idx, void* ws,
                        void* coef, void* status, void* min_pivot);

namespace {
struct Design {
  int nf = 0, nt = 0, wp = 0, nfp = 0;
  LinfitCols cols{linfit_col_bytes(), linfit_pack_col};
  std::vector<double> prog;
  std::vector<int> tiles;
  long long g_off = 0;      // doubles, into the Gram buffer
  void finish() {
    wp = cols.pad16(0, -2, 0, -1);
    nfp = (nf + 15) / 16 * 16;
    tiles = upper_tiles(nfp, wp);
  }
};
struct Config {
  int design, n, nt, tcol;
  std::vector<int> idx;
  long long out;
};
}  // namespace

extern "C" int ampc_linfit_fit(int device, int n_traj, const int* traj_len, int obs_dim, int ctrl_dim,
                               const double* obs, const double* ctrls, int n_arx, const int* arx_history,
                               int n_koopman, const int* koopman_n_basis, const int* koopman_kinds,
                               const double* koopman_params, double* coeffs, int* status, double* min_pivot) {
  REQUIRE(traj_len && obs && ctrls && coeffs && status && min_pivot, "ampc_linfit_fit: NULL argument");
  REQUIRE(n_traj >= 1, "ampc_linfit_fit: n_traj < 1");
  REQUIRE(obs_dim >= 1 && obs_dim <= kFitMaxState, "ampc_linfit_fit: obs_dim must be in 1..256");
  REQUIRE(ctrl_dim >= 1 && ctrl_dim <= kFitMaxCtrl, "ampc_linfit_fit: ctrl_dim must be in 1..16");
  REQUIRE(n_arx >= 0 && n_koopman >= 0 && n_arx + n_koopman >= 1, "ampc_linfit_fit: no configuration");
  REQUIRE(n_arx == 0 || arx_history, "ampc_linfit_fit: NULL arx_history");
  REQUIRE(n_koopman == 0 || (koopman_n_basis && koopman_kinds && koopman_params),
          "ampc_linfit_fit: NULL Koopman basis");
  const int no = obs_dim, nu = ctrl_dim, m = no + nu;
  FitData data;
  if (int rc = data.index("ampc_linfit_fit", n_traj, traj_len)) return rc;
  const long long R = data.R;

  std::vector<Design> designs;
  std::vector<Config> cfgs;
  long long out = 0;
  if (n_arx > 0) {
    int kmax = 0;
    for (int i = 0; i < n_arx; ++i) {
      REQUIRE(arx_history[i] >= 1, "ampc_linfit_fit: ARX history < 1");
      REQUIRE(1 + arx_history[i] * m - nu <= kFitMaxState,
              "ampc_linfit_fit: ARX model state (1 + history (obs_dim + ctrl_dim) - ctrl_dim) must be at most 256");
      kmax = std::max(kmax, arx_history[i]);
    }
    Design d;
    d.nf = 1 + kmax * m;
    d.nt = no;
    for (int j = 0; j < no; ++j) d.cols.add(1, 0, j, -1);
    for (int i = 1; i < kmax; ++i) {
      for (int j = 0; j < no; ++j) d.cols.add(1, i, j, -1);
      for (int j = 0; j < nu; ++j) d.cols.add(2, i, j, -1);
    }
    d.cols.add(0, 0, 0, -1);
    for (int j = 0; j < nu; ++j) d.cols.add(2, 0, j, -1);
    for (int j = 0; j < no; ++j) d.cols.add(1, -1, j, -1);
    d.prog.assign(2, 0.0);
    d.finish();
    designs.push_back(std::move(d));
    for (int i = 0; i < n_arx; ++i) {
      const int k = arx_history[i];
      Config c;
      c.design = 0; c.n = 1 + k * m; c.nt = no; c.tcol = designs[0].nf; c.out = out;
      for (int j = 0; j < no + (k - 1) * m; ++j) c.idx.push_back(j);
      for (int j = designs[0].nf - nu - 1; j < designs[0].nf; ++j) c.idx.push_back(j);
      out += (long long)c.nt * c.n;
      cfgs.push_back(std::move(c));
    }
  }
  std::vector<std::vector<double>> bases;       // distinct (kind, parameter) programs ...
  std::vector<int> basis_design;                // ... and their designs
  for (int i = 0, pos = 0; i < n_koopman; ++i) {
    const int nb = koopman_n_basis[i];
    std::vector<double> prog;
    if (int rc = koopman_basis_program("ampc_linfit_fit", nb, koopman_kinds + pos, koopman_params + pos, no, prog))
      return rc;
    pos += nb;
    int di = -1;
    for (size_t b = 0; b < bases.size(); ++b)
      if (bases[b] == prog) di = basis_design[b];
    if (di < 0) {
      Design d;
      const int n = nb * no;
      d.nf = n + nu;
      d.nt = n;
      koopman_columns(d.cols, prog, no, nu);
      d.prog = prog;
      d.finish();
      di = (int)designs.size();
      designs.push_back(std::move(d));
      bases.push_back(prog);
      basis_design.push_back(di);
    }
    Config c;
    c.design = di; c.n = designs[di].nf; c.nt = designs[di].nt; c.tcol = designs[di].nf; c.out = out;
    c.idx.resize(c.n);
    std::iota(c.idx.begin(), c.idx.end(), 0);
    out += (long long)c.nt * c.n;
    cfgs.push_back(std::move(c));
  }

  const int splits = data.splits;
  long long g_total = 0, part_max = 0;
  for (Design& d : designs) {
    d.g_off = g_total;
    g_total += (long long)d.nfp * d.wp;
    part_max = std::max(part_max, (long long)splits * d.nfp * d.wp);
  }
  REQUIRE(part_max <= (1LL << 31), "ampc_linfit_fit: the Gram workspace would exceed 16 GiB (too many rows)");

  if (int rc = data.stage("ampc_linfit_fit", device, no, nu, obs, ctrls, nullptr)) return rc;
  hipStream_t st = data.sg.s;
  ScopedBuf d_part, d_g, d_descs, d_order, d_idx, d_ws, d_coef, d_status, d_piv;
  std::vector<ScopedBuf> d_cols(designs.size()), d_prog(designs.size()), d_tiles(designs.size());
  HIP_OK(d_part.reserve((size_t)part_max * 8));
  HIP_OK(d_g.reserve((size_t)g_total * 8));
  for (size_t i = 0; i < designs.size(); ++i) {
    const Design& d = designs[i];
    if (int rc = fit_upload(d_cols[i], d.cols.bytes, st)) return rc;
    if (int rc = fit_upload(d_prog[i], d.prog, st)) return rc;
    if (int rc = fit_upload(d_tiles[i], d.tiles, st)) return rc;
    if (int rc = linfit_launch_gram(st, (int)R, no, nu, data.d_obs.p, data.d_ctrls.p, data.d_row_start.p, d_cols[i].p,
                                    d_prog[i].p, d_tiles[i].p, (int)d.tiles.size(), d.nf, d.nt, d_part.p,
                                    (double*)d_g.p + d.g_off))
      return rc;
  }

  const int C = (int)cfgs.size();
  const size_t dsz = linfit_desc_bytes();
  std::vector<char> descs((size_t)C * dsz);
  std::vector<int> idx;
  long long ws = 0;
  for (int i = 0; i < C; ++i) {
    const Config& c = cfgs[i];
    const Design& d = designs[c.design];
    linfit_pack_desc(descs.data() + (size_t)i * dsz, c.n, c.nt, c.tcol, i, (const double*)d_g.p + d.g_off, d.wp,
                     (long long)idx.size(), ws, c.out);
    idx.insert(idx.end(), c.idx.begin(), c.idx.end());
    ws += (long long)(c.n + c.nt) * c.n;
  }
  // heaviest configuration first: n^2 (n / 3 + targets) decides how long a workgroup runs
  std::vector<int> order(C);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
    const double wa = (double)cfgs[a].n * cfgs[a].n * (cfgs[a].n / 3.0 + cfgs[a].nt);
    const double wb = (double)cfgs[b].n * cfgs[b].n * (cfgs[b].n / 3.0 + cfgs[b].nt);
    return wa > wb;
  });
  if (int rc = fit_upload(d_descs, descs, st)) return rc;
  if (int rc = fit_upload(d_order, order, st)) return rc;
  if (int rc = fit_upload(d_idx, idx, st)) return rc;
  HIP_OK(d_ws.reserve((size_t)ws * 8));
  HIP_OK(d_coef.reserve((size_t)out * 8));
  HIP_OK(d_status.reserve((size_t)C * 4));
  HIP_OK(d_piv.reserve((size_t)C * 8));
  if (int rc = linfit_launch_solve(st, C, d_descs.p, d_order.p, d_idx.p, d_ws.p, d_coef.p, d_status.p, d_piv.p))
    return rc;
  HIP_OK(hipMemcpyAsync(coeffs, d_coef.p, (size_t)out * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(status, d_status.p, (size_t)C * 4, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(min_pivot, d_piv.p, (size_t)C * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  return 0;
}
