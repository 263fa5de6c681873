// fit_host.hpp -- host side shared by the GPU fits (api_linfit.cpp, api_sindyfit.cpp, api_lasso.cpp): the staged data
// set, the packed column list and tile list of a design, the Koopman basis program.  The refusal messages carry the
// entry point's name in front.
#pragma once
#include "host_common.hpp"

#include <numeric>

#include "gram_frame.hpp"

size_t linfit_col_bytes();
void linfit_pack_col(void* dst, int src, int lag, int j, int fn);

static constexpr int kFitMaxState = 256, kFitMaxCtrl = 16;     // (SINDy's own state limit: sindyfit_kernels.hpp)

struct StreamGuard {
  hipStream_t s = nullptr;
  ~StreamGuard() { if (s) (void)hipStreamDestroy(s); }
};

// reserve + asynchronous upload of a host vector
template <class T>
int fit_upload(ScopedBuf& buf, const std::vector<T>& v, hipStream_t st) {
  HIP_OK(buf.reserve(v.size() * sizeof(T)));
  HIP_OK(hipMemcpyAsync(buf.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, st));
  return 0;
}

// The data set of one call: trajectories concatenated by row.  index() is host work only; stage() opens the device,
// creates the call's stream and uploads.  Declare it before the call's other device buffers: the stream outlives them.
struct FitData {
  long long R = 0, design_rows = 0;       // data rows; rows with a successor
  int splits = 0;                         // row splits of the Gram pass
  std::vector<int> row_start;             // [R]: first row of the row's trajectory; -1: a trajectory's last row
  StreamGuard sg;
  ScopedBuf d_obs, d_ctrls, d_ycont, d_row_start;

  int index(const std::string& name, int n_traj, const int* traj_len) {
    for (int i = 0; i < n_traj; ++i) {
      REQUIRE(traj_len[i] >= 1, name + ": trajectory length < 1");
      R += traj_len[i];
    }
    REQUIRE(R < (1LL << 30), name + ": too many rows");
    row_start.resize((size_t)R);
    for (long long g = 0, i = 0; i < n_traj; ++i) {
      const long long s = g;
      for (int t = 0; t < traj_len[i]; ++t, ++g) row_start[g] = t + 1 < traj_len[i] ? (int)s : -1;
      design_rows += traj_len[i] - 1;
    }
    REQUIRE(design_rows >= 1, name + ": no trajectory has two rows");
    splits = (int)((R + kFitSplitRows - 1) / kFitSplitRows);
    return 0;
  }

  // ycont: nullptr or [R][obs_dim]
  int stage(const std::string& name, int device, int obs_dim, int ctrl_dim, const double* obs, const double* ctrls,
            const double* ycont) {
    REQUIRE(ampc_device_count() > 0, name + ": no HIP device");
    HIP_OK(hipSetDevice(device));
    HIP_OK(hipStreamCreateWithFlags(&sg.s, hipStreamNonBlocking));
    HIP_OK(d_obs.reserve((size_t)R * obs_dim * 8));
    HIP_OK(d_ctrls.reserve((size_t)R * ctrl_dim * 8));
    HIP_OK(hipMemcpyAsync(d_obs.p, obs, (size_t)R * obs_dim * 8, hipMemcpyHostToDevice, sg.s));
    HIP_OK(hipMemcpyAsync(d_ctrls.p, ctrls, (size_t)R * ctrl_dim * 8, hipMemcpyHostToDevice, sg.s));
    if (ycont) {
      HIP_OK(d_ycont.reserve((size_t)R * obs_dim * 8));
      HIP_OK(hipMemcpyAsync(d_ycont.p, ycont, (size_t)R * obs_dim * 8, hipMemcpyHostToDevice, sg.s));
    }
    return fit_upload(d_row_start, row_start, sg.s);
  }
};

// The per-column rules of one design, packed for the device by the family's packer (A...: a rule's fields).
template <class... A>
struct FitCols {
  size_t col_bytes;
  void (*pack)(void* dst, A...);
  std::vector<char> bytes;
  int n = 0;
  void add(A... a) {
    bytes.resize(bytes.size() + col_bytes);
    pack(bytes.data() + bytes.size() - col_bytes, a...);
    ++n;
  }
  // pads with the zero column's rule to a multiple of 16 columns; returns that width
  int pad16(A... zero) {
    while (n % 16) add(zero...);
    return n;
  }
};
using LinfitCols = FitCols<int, int, int, int>;     // (src, lag, j, fn): LinfitCol

// Tiles (ti | tj << 16) of F'[F | Y]: of the symmetric part those on and above the diagonal; the target columns follow
// in the same tile rows.
inline std::vector<int> upper_tiles(int nfp, int wp) {
  std::vector<int> tiles;
  for (int ti = 0; ti < nfp / 16; ++ti)
    for (int tj = ti; tj < wp / 16; ++tj) tiles.push_back(ti | (tj << 16));
  return tiles;
}

// Validates one Koopman basis (kinds, params)[nb] and appends it to prog as (kind, parameter) pairs.
inline int koopman_basis_program(const std::string& name, int nb, const int* kinds, const double* params, int obs_dim,
                                 std::vector<double>& prog) {
  REQUIRE(nb >= 1 && (long long)nb * obs_dim <= kFitMaxState,
          name + ": a Koopman lift (n_basis * obs_dim) must have 1..256 states");
  for (int k = 0; k < nb; ++k) {
    REQUIRE(kinds[k] >= 0 && kinds[k] <= 3, name + ": basis kind must be 0 identity, 1 power, 2 sin, 3 cos");
    REQUIRE(kinds[k] != 1 || (params[k] >= 0 && params[k] <= 64 && params[k] == std::floor(params[k])),
            name + ": powers must be integers in 0..64");
    prog.push_back(kinds[k]);
    prog.push_back(params[k]);
  }
  return 0;
}

// Appends the columns of a Koopman design: the lifted observation, the controls, the lifted next observation.
inline void koopman_columns(LinfitCols& cols, const std::vector<double>& prog, int obs_dim, int ctrl_dim) {
  const int nb = (int)prog.size() / 2;
  auto lift = [&](int lag) {
    for (int f = 0; f < nb; ++f)
      for (int j = 0; j < obs_dim; ++j) cols.add(1, lag, j, prog[2 * f] == 0.0 ? -1 : f);
  };
  lift(0);
  for (int j = 0; j < ctrl_dim; ++j) cols.add(2, 0, j, -1);
  lift(-1);
}
