// api_linfit.cpp -- ampc_linfit_fit: least-squares fits of ARX and Koopman(lstsq) configurations of one data set in one
// call (reference: autompc/sysid/arx.py:62-116 ARX.train, koopman.py:141-154 Koopman.train).  One Gram pass per
// design -- the ARX design of the longest history asked for holds every shorter history's normal equations as a
// sub-matrix; Koopman configurations of one basis share a design -- then one solve workgroup per configuration.
// f64 only; kernels in linfit_kernels.hpp, launchers in launch_linfit.cpp.
#include "host_common.hpp"

#include <numeric>

size_t linfit_col_bytes();
size_t linfit_desc_bytes();
int linfit_split_rows();
void linfit_pack_col(void* dst, int src, int lag, int j, int fn);
void linfit_pack_desc(void* dst, int n, int nt, int tcol, int id, const double* g, long long ldg, long long idx,
                      long long ws, long long out);
int linfit_launch_gram(hipStream_t st, int R, int no, int nu, const void* obs, const void* ctrls,
                       const void* row_start, const void* cols, const void* prog, const void* tiles, int n_tiles,
                       int nf, int nt, void* part, void* G);
int linfit_launch_solve(hipStream_t st, int n, const void* descs, const void* order, const void* idx, void* ws,
                        void* coef, void* status, void* min_pivot);

static constexpr int kLinfitMaxState = 256, kLinfitMaxCtrl = 16;

namespace {
struct Design {
  int nf = 0, nt = 0, wp = 0, nfp = 0;
  std::vector<char> cols;
  std::vector<double> prog;
  std::vector<int> tiles;
  long long g_off = 0;      // doubles, into the Gram buffer
  void add_col(int src, int lag, int j, int fn) {
    cols.resize(cols.size() + linfit_col_bytes());
    linfit_pack_col(cols.data() + cols.size() - linfit_col_bytes(), src, lag, j, fn);
  }
  void finish() {
    wp = (nf + nt + 15) / 16 * 16;
    nfp = (nf + 15) / 16 * 16;
    for (int c = nf + nt; c < wp; ++c) add_col(0, -2, 0, -1);      // padding columns: zero
    // symmetric part: tiles on and above the diagonal; the target columns follow in the same tile rows
    for (int ti = 0; ti < nfp / 16; ++ti)
      for (int tj = ti; tj < wp / 16; ++tj) tiles.push_back(ti | (tj << 16));
  }
};
struct Config {
  int design, n, nt, tcol;
  std::vector<int> idx;
  long long out;
};
struct StreamGuard {
  hipStream_t s = nullptr;
  ~StreamGuard() { if (s) (void)hipStreamDestroy(s); }
};
}  // namespace

extern "C" int ampc_linfit_fit(int device, int n_traj, const int* traj_len, int obs_dim, int ctrl_dim,
                               const double* obs, const double* ctrls, int n_arx, const int* arx_history,
                               int n_koopman, const int* koopman_n_basis, const int* koopman_kinds,
                               const double* koopman_params, double* coeffs, int* status, double* min_pivot) {
  REQUIRE(traj_len && obs && ctrls && coeffs && status && min_pivot, "ampc_linfit_fit: NULL argument");
  REQUIRE(n_traj >= 1, "ampc_linfit_fit: n_traj < 1");
  REQUIRE(obs_dim >= 1 && obs_dim <= kLinfitMaxState, "ampc_linfit_fit: obs_dim must be in 1..256");
  REQUIRE(ctrl_dim >= 1 && ctrl_dim <= kLinfitMaxCtrl, "ampc_linfit_fit: ctrl_dim must be in 1..16");
  REQUIRE(n_arx >= 0 && n_koopman >= 0 && n_arx + n_koopman >= 1, "ampc_linfit_fit: no configuration");
  REQUIRE(n_arx == 0 || arx_history, "ampc_linfit_fit: NULL arx_history");
  REQUIRE(n_koopman == 0 || (koopman_n_basis && koopman_kinds && koopman_params),
          "ampc_linfit_fit: NULL Koopman basis");
  const int no = obs_dim, nu = ctrl_dim, m = no + nu;
  long long R = 0;
  for (int i = 0; i < n_traj; ++i) {
    REQUIRE(traj_len[i] >= 1, "ampc_linfit_fit: trajectory length < 1");
    R += traj_len[i];
  }
  REQUIRE(R < (1LL << 30), "ampc_linfit_fit: too many rows");
  // first row of every row's trajectory; -1 for a trajectory's last row (it predicts nothing)
  std::vector<int> row_start((size_t)R);
  long long design_rows = 0;
  for (long long g = 0, i = 0; i < n_traj; ++i) {
    const long long s = g;
    for (int t = 0; t < traj_len[i]; ++t, ++g) row_start[g] = t + 1 < traj_len[i] ? (int)s : -1;
    design_rows += traj_len[i] - 1;
  }
  REQUIRE(design_rows >= 1, "ampc_linfit_fit: no trajectory has two rows");

  std::vector<Design> designs;
  std::vector<Config> cfgs;
  long long out = 0;
  if (n_arx > 0) {
    int kmax = 0;
    for (int i = 0; i < n_arx; ++i) {
      REQUIRE(arx_history[i] >= 1, "ampc_linfit_fit: ARX history < 1");
      REQUIRE(1 + arx_history[i] * m - nu <= kLinfitMaxState,
              "ampc_linfit_fit: ARX model state (1 + history (obs_dim + ctrl_dim) - ctrl_dim) must be at most 256");
      kmax = std::max(kmax, arx_history[i]);
    }
    Design d;
    d.nf = 1 + kmax * m;
    d.nt = no;
    for (int j = 0; j < no; ++j) d.add_col(1, 0, j, -1);
    for (int i = 1; i < kmax; ++i) {
      for (int j = 0; j < no; ++j) d.add_col(1, i, j, -1);
      for (int j = 0; j < nu; ++j) d.add_col(2, i, j, -1);
    }
    d.add_col(0, 0, 0, -1);
    for (int j = 0; j < nu; ++j) d.add_col(2, 0, j, -1);
    for (int j = 0; j < no; ++j) d.add_col(1, -1, j, -1);
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
    REQUIRE(nb >= 1 && (long long)nb * no <= kLinfitMaxState,
            "ampc_linfit_fit: a Koopman lift (n_basis * obs_dim) must have 1..256 states");
    std::vector<double> prog;
    for (int k = 0; k < nb; ++k, ++pos) {
      const int kind = koopman_kinds[pos];
      const double par = koopman_params[pos];
      REQUIRE(kind >= 0 && kind <= 3, "ampc_linfit_fit: basis kind must be 0 identity, 1 power, 2 sin, 3 cos");
      REQUIRE(kind != 1 || (par >= 0 && par <= 64 && par == std::floor(par)),
              "ampc_linfit_fit: powers must be integers in 0..64");
      prog.push_back(kind);
      prog.push_back(par);
    }
    int di = -1;
    for (size_t b = 0; b < bases.size(); ++b)
      if (bases[b] == prog) di = basis_design[b];
    if (di < 0) {
      Design d;
      const int n = nb * no;
      d.nf = n + nu;
      d.nt = n;
      for (int f = 0; f < nb; ++f)
        for (int j = 0; j < no; ++j) d.add_col(1, 0, j, prog[2 * f] == 0.0 ? -1 : f);
      for (int j = 0; j < nu; ++j) d.add_col(2, 0, j, -1);
      for (int f = 0; f < nb; ++f)
        for (int j = 0; j < no; ++j) d.add_col(1, -1, j, prog[2 * f] == 0.0 ? -1 : f);
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

  const int splits = (int)((R + linfit_split_rows() - 1) / linfit_split_rows());
  long long g_total = 0, part_max = 0;
  for (Design& d : designs) {
    d.g_off = g_total;
    g_total += (long long)d.nfp * d.wp;
    part_max = std::max(part_max, (long long)splits * d.nfp * d.wp);
  }
  REQUIRE(part_max <= (1LL << 31), "ampc_linfit_fit: the Gram workspace would exceed 16 GiB (too many rows)");

  REQUIRE(ampc_device_count() > 0, "ampc_linfit_fit: no HIP device");
  HIP_OK(hipSetDevice(device));
  StreamGuard sg;
  HIP_OK(hipStreamCreateWithFlags(&sg.s, hipStreamNonBlocking));
  hipStream_t st = sg.s;
  ScopedBuf d_obs, d_ctl, d_rs, d_part, d_g, d_descs, d_order, d_idx, d_ws, d_coef, d_status, d_piv;
  std::vector<ScopedBuf> d_cols(designs.size()), d_prog(designs.size()), d_tiles(designs.size());
  HIP_OK(d_obs.reserve((size_t)R * no * 8));
  HIP_OK(d_ctl.reserve((size_t)R * nu * 8));
  HIP_OK(d_rs.reserve((size_t)R * 4));
  HIP_OK(d_part.reserve((size_t)part_max * 8));
  HIP_OK(d_g.reserve((size_t)g_total * 8));
  HIP_OK(hipMemcpyAsync(d_obs.p, obs, (size_t)R * no * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_ctl.p, ctrls, (size_t)R * nu * 8, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_rs.p, row_start.data(), (size_t)R * 4, hipMemcpyHostToDevice, st));
  for (size_t i = 0; i < designs.size(); ++i) {
    const Design& d = designs[i];
    HIP_OK(d_cols[i].reserve(d.cols.size()));
    HIP_OK(d_prog[i].reserve(d.prog.size() * 8));
    HIP_OK(d_tiles[i].reserve(d.tiles.size() * 4));
    HIP_OK(hipMemcpyAsync(d_cols[i].p, d.cols.data(), d.cols.size(), hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_prog[i].p, d.prog.data(), d.prog.size() * 8, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_tiles[i].p, d.tiles.data(), d.tiles.size() * 4, hipMemcpyHostToDevice, st));
    if (int rc = linfit_launch_gram(st, (int)R, no, nu, d_obs.p, d_ctl.p, d_rs.p, d_cols[i].p, d_prog[i].p,
                                    d_tiles[i].p, (int)d.tiles.size(), d.nf, d.nt, d_part.p,
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
  HIP_OK(d_descs.reserve(descs.size()));
  HIP_OK(d_order.reserve((size_t)C * 4));
  HIP_OK(d_idx.reserve(idx.size() * 4));
  HIP_OK(d_ws.reserve((size_t)ws * 8));
  HIP_OK(d_coef.reserve((size_t)out * 8));
  HIP_OK(d_status.reserve((size_t)C * 4));
  HIP_OK(d_piv.reserve((size_t)C * 8));
  HIP_OK(hipMemcpyAsync(d_descs.p, descs.data(), descs.size(), hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_order.p, order.data(), (size_t)C * 4, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_idx.p, idx.data(), idx.size() * 4, hipMemcpyHostToDevice, st));
  if (int rc = linfit_launch_solve(st, C, d_descs.p, d_order.p, d_idx.p, d_ws.p, d_coef.p, d_status.p, d_piv.p))
    return rc;
  HIP_OK(hipMemcpyAsync(coeffs, d_coef.p, (size_t)out * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(status, d_status.p, (size_t)C * 4, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(min_pivot, d_piv.p, (size_t)C * 8, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  return 0;
}
