// launch_mlpfit.cpp -- launchers of the MLP training kernels (mlpfit_kernels.hpp).  f64 only: compiled once.
#include "host_common.hpp"
#include "mlpfit_kernels.hpp"

size_t mlpfit_model_bytes() { return sizeof(MlpFitModel); }
int mlpfit_max_layers() { return kFitMaxLayers; }
int mlpfit_max_width() { return kFitMaxWidth; }
int mlpfit_max_in() { return kFitMaxIn; }
int mlpfit_max_out() { return kFitMaxOut; }
int mlpfit_max_batch() { return kFitMaxBatch; }

void mlpfit_pack_model(void* dst, int n_layers, int act, const int* dims, double lr, const long long* w,
                       const long long* b, const long long* a, const long long* g) {
  MlpFitModel m{};
  m.n_layers = n_layers; m.act = act; m.lr = lr;
  for (int l = 0; l <= n_layers; ++l) m.dims[l] = dims[l];
  for (int l = 0; l < n_layers; ++l) { m.w[l] = w[l]; m.b[l] = b[l]; m.a[l] = a[l]; m.g[l] = g[l]; }
  std::memcpy(dst, &m, sizeof m);
}

// One optimiser step on rows [row0, row0 + nb) of every model's epoch order: layers 0 .. n_layers - 1 forward, then
// backward, one launch each.  fwd_tiles[l] / bwd_blocks[l]: the widest model's
// column-tile / input-column-block count of layer l (the backward grid has one more workgroup: the bias').
int mlpfit_launch_step(hipStream_t st, int n_models, int n_layers, const int* fwd_cols, const int* bwd_blocks,
                       const void* models, const double* feed, const double* target, const int* idx, double* params,
                       double* m, double* v, double* abuf, double* gbuf, int n_rows, int row0, int nb, double bc1,
                       double bc2_sqrt) {
  MlpFitArgs a{};
  a.models = (const MlpFitModel*)models;
  a.feed = feed; a.target = target; a.idx = idx; a.params = params; a.m = m; a.v = v; a.abuf = abuf; a.gbuf = gbuf;
  a.n_rows = n_rows; a.row0 = row0; a.nb = nb; a.bc1 = bc1; a.bc2_sqrt = bc2_sqrt;
  const int rt = (nb + 15) / 16;
  for (int l = 0; l < n_layers; ++l) {
    a.layer = l;
    hipLaunchKernelGGL(mlpfit_forward_kernel, dim3(fwd_cols[l] * rt, n_models), dim3(kFitFwdThreads), 0, st, a);
  }
  for (int l = n_layers - 1; l >= 0; --l) {
    a.layer = l;
    hipLaunchKernelGGL(mlpfit_backward_kernel, dim3(bwd_blocks[l] + 1, n_models), dim3(kFitBwdThreads), 0, st, a);
  }
  HIP_OK(hipGetLastError());
  return 0;
}
