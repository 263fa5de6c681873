// api_mlpfit.cpp -- ampc_mlpfit_*: the reference's MLP training loop (autompc/sysid/mlp.py:177-217) for a table of
// models of any mix of depth, widths, activation and learning rate over one data set.  A plan owns Adam's moments, the
// step count and the activation / gradient buffers; the caller owns the data, the row orders and the flat parameter
// buffer (device memory, in practice torch tensors).  One optimiser step is one launch per layer forward and one per
// layer backward on the plan's stream (mlpfit_kernels.hpp, launch_mlpfit.cpp); nothing synchronises.  f64 only.
#include "host_common.hpp"

size_t mlpfit_model_bytes();
int mlpfit_max_layers();
int mlpfit_max_width();
int mlpfit_max_in();
int mlpfit_max_out();
int mlpfit_max_batch();
void mlpfit_pack_model(void* dst, int n_layers, int act, const int* dims, double lr, const long long* w,
                       const long long* b, const long long* a, const long long* g);
int mlpfit_launch_step(hipStream_t st, int n_models, int n_layers, const int* fwd_cols, const int* bwd_blocks,
                       const void* models, const double* feed, const double* target, const int* idx, double* params,
                       double* m, double* v, double* abuf, double* gbuf, int n_rows, int row0, int nb, double bc1,
                       double bc2_sqrt);

struct ampc_mlpfit_plan {
  int device = 0;
  hipStream_t stream = nullptr;
  int n_models = 0, n_rows = 0, n_batch = 0, n_layers = 0;   // n_layers: the deepest model's linear layers
  std::vector<int> fwd_cols, bwd_blocks;                     // per layer: the widest model's tile / block count
  const double* feed = nullptr;
  const double* target = nullptr;
  double* params = nullptr;
  DevBuf models, m, v, abuf, gbuf;
  long long t = 0;                                           // optimiser steps taken
};

static int on_device(const void* p, int device, const char* what) {
  hipPointerAttribute_t attr;
  REQUIRE(hipPointerGetAttributes(&attr, p) == hipSuccess && attr.type == hipMemoryTypeDevice && attr.device == device,
          std::string(what) + " must be device memory of the plan's device");
  return 0;
}

static void mlpfit_free(ampc_mlpfit_plan* p) {
  p->models.release(); p->m.release(); p->v.release(); p->abuf.release(); p->gbuf.release();
  delete p;
}

extern "C" int ampc_mlpfit_create(int device, void* stream, int n_models, const int* n_hidden, const int* dims,
                                  const int* activations, const double* lrs, const long long* param_offsets,
                                  const double* feed_dev, const double* target_dev, int n_rows, int n_batch,
                                  double* params_dev, long long n_params, ampc_mlpfit_plan** out) {
  REQUIRE(out != nullptr, "ampc_mlpfit_create: NULL out");
  *out = nullptr;
  REQUIRE(n_hidden && dims && activations && lrs && param_offsets && feed_dev && target_dev && params_dev,
          "ampc_mlpfit_create: NULL argument");
  REQUIRE(n_models >= 1, "ampc_mlpfit_create: n_models < 1");
  REQUIRE(n_rows >= 1, "ampc_mlpfit_create: n_rows < 1");
  REQUIRE(n_batch >= 1 && n_batch <= mlpfit_max_batch(), "ampc_mlpfit_create: n_batch must be in 1..4096");
  int n_dev = 0;
  REQUIRE(hipGetDeviceCount(&n_dev) == hipSuccess && n_dev > 0, "ampc_mlpfit_create: no HIP device visible");
  REQUIRE(device >= 0 && device < n_dev, "ampc_mlpfit_create: no such device");
  const int ML = mlpfit_max_layers(), stride = ML + 1;
  const int kin = dims[0];
  int deepest = 0;
  std::vector<int> fwd_cols(ML, 0), bwd_blocks(ML, 0);
  std::vector<std::pair<long long, long long>> spans;
  std::vector<char> host((size_t)n_models * mlpfit_model_bytes());
  long long a_total = 0, g_total = 0;
  int nout = 0;
  for (int k = 0; k < n_models; ++k) {
    const int nh = n_hidden[k], L = nh + 1;
    const int* d = dims + (size_t)k * stride;
    REQUIRE(nh >= 1 && nh <= kMaxHidden, "ampc_mlpfit_create: a model must have 1..4 hidden layers");
    REQUIRE(activations[k] >= 0 && activations[k] <= 3, "ampc_mlpfit_create: activation must be relu, tanh, sigmoid or selu");
    REQUIRE(lrs[k] == lrs[k], "ampc_mlpfit_create: a learning rate is NaN");
    REQUIRE(d[0] >= 1 && d[0] <= mlpfit_max_in(), "ampc_mlpfit_create: inputs (nx + nu) must be in 1..80");
    REQUIRE(d[L] >= 1 && d[L] <= mlpfit_max_out(), "ampc_mlpfit_create: outputs (nx) must be in 1..64");
    if (k == 0) nout = d[L];
    REQUIRE(d[0] == kin && d[L] == nout, "ampc_mlpfit_create: the models of a plan share the data's input and output width");
    for (int l = 1; l < L; ++l)
      REQUIRE(d[l] >= 1 && d[l] <= mlpfit_max_width(), "ampc_mlpfit_create: hidden widths must be in 1..256");
    long long w[8], b[8], a[8], g[8];
    long long o = param_offsets[k];
    REQUIRE(o >= 0, "ampc_mlpfit_create: negative parameter offset");
    for (int l = 0; l < L; ++l) {
      w[l] = o; o += (long long)d[l + 1] * d[l];
      b[l] = o; o += d[l + 1];
      a[l] = a_total;
      if (l > 0) a_total += (long long)n_batch * d[l];
      g[l] = g_total; g_total += (long long)n_batch * d[l + 1];
      fwd_cols[l] = std::max(fwd_cols[l], (d[l + 1] + 15) / 16);
      bwd_blocks[l] = std::max(bwd_blocks[l], (d[l] + 15) / 16);
    }
    REQUIRE(o <= n_params, "ampc_mlpfit_create: a model's parameters end past the parameter buffer");
    spans.emplace_back(param_offsets[k], o);
    deepest = std::max(deepest, L);
    mlpfit_pack_model(host.data() + (size_t)k * mlpfit_model_bytes(), L, activations[k], d, lrs[k], w, b, a, g);
  }
  std::sort(spans.begin(), spans.end());
  for (size_t i = 1; i < spans.size(); ++i)
    REQUIRE(spans[i].first >= spans[i - 1].second, "ampc_mlpfit_create: two models' parameters overlap");
  HIP_OK(hipSetDevice(device));
  if (int rc = on_device(feed_dev, device, "ampc_mlpfit_create: feed")) return rc;
  if (int rc = on_device(target_dev, device, "ampc_mlpfit_create: target")) return rc;
  if (int rc = on_device(params_dev, device, "ampc_mlpfit_create: params")) return rc;

  ampc_mlpfit_plan* p = new ampc_mlpfit_plan;
  p->device = device; p->stream = (hipStream_t)stream;
  p->n_models = n_models; p->n_rows = n_rows; p->n_batch = n_batch; p->n_layers = deepest;
  p->fwd_cols = fwd_cols; p->bwd_blocks = bwd_blocks;
  p->feed = feed_dev; p->target = target_dev; p->params = params_dev;
  hipError_t e = p->models.reserve(host.size());
  if (e == hipSuccess) e = p->m.reserve((size_t)n_params * 8);
  if (e == hipSuccess) e = p->v.reserve((size_t)n_params * 8);
  if (e == hipSuccess) e = p->abuf.reserve((size_t)std::max(a_total, 1LL) * 8);
  if (e == hipSuccess) e = p->gbuf.reserve((size_t)g_total * 8);
  if (e == hipSuccess) e = hipMemcpyAsync(p->models.p, host.data(), host.size(), hipMemcpyHostToDevice, p->stream);
  if (e == hipSuccess) e = hipMemsetAsync(p->m.p, 0, (size_t)n_params * 8, p->stream);
  if (e == hipSuccess) e = hipMemsetAsync(p->v.p, 0, (size_t)n_params * 8, p->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(p->stream);       // `host` goes out of scope
  if (e != hipSuccess) {
    mlpfit_free(p);
    return fail(std::string("ampc_mlpfit_create: ") + hipGetErrorString(e));
  }
  *out = p;
  return 0;
}

extern "C" int ampc_mlpfit_run_epoch(ampc_mlpfit_plan* p, const int* idx_dev) {
  REQUIRE(p != nullptr && idx_dev != nullptr, "ampc_mlpfit_run_epoch: NULL argument");
  HIP_OK(hipSetDevice(p->device));
  if (int rc = on_device(idx_dev, p->device, "ampc_mlpfit_run_epoch: idx")) return rc;
  for (int row0 = 0; row0 < p->n_rows; row0 += p->n_batch) {
    const int nb = std::min(p->n_batch, p->n_rows - row0);
    const long long t = p->t + 1;
    const double bc1 = 1.0 - std::pow(0.9, (double)t), bc2 = 1.0 - std::pow(0.999, (double)t);
    if (int rc = mlpfit_launch_step(p->stream, p->n_models, p->n_layers, p->fwd_cols.data(), p->bwd_blocks.data(),
                                    p->models.p, p->feed, p->target, idx_dev, p->params, (double*)p->m.p,
                                    (double*)p->v.p, (double*)p->abuf.p, (double*)p->gbuf.p, p->n_rows, row0, nb, bc1,
                                    std::sqrt(bc2)))
      return rc;
    p->t = t;
  }
  return 0;
}

extern "C" int ampc_mlpfit_steps(const ampc_mlpfit_plan* p, long long* steps) {
  REQUIRE(p != nullptr && steps != nullptr, "ampc_mlpfit_steps: NULL argument");
  *steps = p->t;
  return 0;
}

extern "C" int ampc_mlpfit_destroy(ampc_mlpfit_plan* p) {
  if (p == nullptr) return 0;
  (void)hipSetDevice(p->device);
  (void)hipStreamSynchronize(p->stream);
  mlpfit_free(p);
  return 0;
}
