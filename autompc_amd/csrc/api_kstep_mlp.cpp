// api_kstep_mlp.cpp -- ampc_kstep_errors_mlp: k-step prediction error sums of MLP models of any mix of depth, widths
// and activation in ONE launch (kstep_mlp_kernels.hpp, launch_kstep_mlp.cpp).  This unit is host code only: the
// argument checks, the packing of host-resident parameters into one upload (kstep_mlp_prepare: no device call, so a
// stand-alone host program can run it) and the model table.  No handle is involved: device-resident parameters are read
// where they are.  f64 only.
#include "host_common.hpp"

#include "kstep_mlp_host.hpp"

size_t kstep_mlp_model_bytes();
void kstep_mlp_limits(int out[5]);
void kstep_mlp_pack_model(void* dst, int n_layers, int act, const int* dims, const double* const* w,
                          const double* const* b, const double* const* norm);
int kstep_mlp_launch(hipStream_t st, int n_models, const void* d_models, int nx, int nu, int n_traj,
                     const int* traj_len, const double* obs, const double* ctrls, int kmax, const double* inv_std,
                     double* sq_err, double* sq_delta_err);

int kstep_mlp_prepare(int n_models, const int* n_hidden, const int* dims, const int* activations,
                      const double* const* weights, const double* const* biases, const double* const* norms,
                      const int* on_device, int nx, int nu, int obs_dim, KstepMlpPrep* out) {
  REQUIRE(out != nullptr, "ampc_kstep_errors_mlp: internal: NULL prep");
  REQUIRE(n_models >= 1, "ampc_kstep_errors_mlp: no models");
  REQUIRE(n_hidden && dims && activations && weights && biases && norms && on_device,
          "ampc_kstep_errors_mlp: NULL model argument");
  int lim[5];
  kstep_mlp_limits(lim);
  const int max_hidden = lim[0], max_width = lim[1], max_in = lim[2], max_out = lim[3], max_ctrl = lim[4];
  REQUIRE(nx >= 1 && nx <= max_out, "ampc_kstep_errors_mlp: the state dim (nx) must be in 1..64");
  REQUIRE(nu >= 1 && nu <= max_ctrl, "ampc_kstep_errors_mlp: ctrl_dim (nu) must be in 1..16");
  REQUIRE(nx + nu <= max_in, "ampc_kstep_errors_mlp: inputs (nx + nu) must be at most 80");
  REQUIRE(obs_dim == nx, "ampc_kstep_errors_mlp: obs_dim must be the models' state dim (the state is the observation)");
  const int ML = max_hidden + 1, stride = ML + 1;
  out->n_models = n_models;
  out->max_layers = ML;
  out->stage.clear();
  out->w_off.assign((size_t)n_models * ML, -1);
  out->b_off.assign((size_t)n_models * ML, -1);
  out->n_off.assign((size_t)n_models * 4, -1);
  for (int k = 0; k < n_models; ++k) {
    const int nh = n_hidden[k], L = nh + 1;
    const int* d = dims + (size_t)k * stride;
    REQUIRE(nh >= 1 && nh <= max_hidden, "ampc_kstep_errors_mlp: a model must have 1..4 hidden layers");
    REQUIRE(activations[k] >= 0 && activations[k] <= 3,
            "ampc_kstep_errors_mlp: activation must be relu, tanh, sigmoid or selu");
    REQUIRE(d[0] == nx + nu && d[L] == nx,
            "ampc_kstep_errors_mlp: every model of a call takes nx + nu inputs and gives nx outputs");
    for (int l = 1; l < L; ++l)
      REQUIRE(d[l] >= 1 && d[l] <= max_width, "ampc_kstep_errors_mlp: hidden widths must be in 1..256");
    for (int l = 0; l < L; ++l)
      REQUIRE(weights[(size_t)k * ML + l] && biases[(size_t)k * ML + l],
              "ampc_kstep_errors_mlp: NULL weight or bias pointer");
    for (int i = 0; i < 4; ++i) REQUIRE(norms[(size_t)k * 4 + i], "ampc_kstep_errors_mlp: NULL normaliser pointer");
    if (on_device[k]) continue;
    // host-resident: layer after layer the weight [out][in] and the bias [out], then the four normalisers
    for (int l = 0; l < L; ++l) {
      const size_t nw = (size_t)d[l + 1] * d[l], nb = (size_t)d[l + 1];
      const double* w = weights[(size_t)k * ML + l];
      const double* b = biases[(size_t)k * ML + l];
      out->w_off[(size_t)k * ML + l] = (long long)out->stage.size();
      out->stage.insert(out->stage.end(), w, w + nw);
      out->b_off[(size_t)k * ML + l] = (long long)out->stage.size();
      out->stage.insert(out->stage.end(), b, b + nb);
    }
    for (int i = 0; i < 4; ++i) {
      const double* v = norms[(size_t)k * 4 + i];
      out->n_off[(size_t)k * 4 + i] = (long long)out->stage.size();
      out->stage.insert(out->stage.end(), v, v + (i < 2 ? nx + nu : nx));
    }
  }
  return 0;
}

static int km_on_device(const void* p, int device) {
  hipPointerAttribute_t attr;
  const hipError_t e = hipPointerGetAttributes(&attr, p);
  if (e != hipSuccess) (void)hipGetLastError();       // (a host address is an error of the query: not left behind)
  REQUIRE(e == hipSuccess && attr.type == hipMemoryTypeDevice && attr.device == device,
          "ampc_kstep_errors_mlp: a model flagged as device-resident has a parameter that is not device memory of "
          "`device`");
  return 0;
}

extern "C" int ampc_kstep_errors_mlp(int device, int n_models, const int* n_hidden, const int* dims,
                                     const int* activations, const double* const* weights,
                                     const double* const* biases, const double* const* norms, const int* on_device,
                                     int nx, int nu, int n_traj, const int* traj_len, int obs_dim, const double* obs,
                                     const double* ctrls, int kmax, const double* inv_std, double* sq_err,
                                     double* sq_delta_err) {
  REQUIRE(n_traj >= 0 && (n_traj == 0 || traj_len), "ampc_kstep_errors_mlp: NULL trajectory lengths");
  REQUIRE(kmax >= 1, "ampc_kstep_errors_mlp: kmax must be >= 1");
  REQUIRE(sq_err, "ampc_kstep_errors_mlp: NULL sq_err");
  REQUIRE(!sq_delta_err || inv_std, "ampc_kstep_errors_mlp: sq_delta_err needs inv_std");
  long long total = 0;
  for (int i = 0; i < n_traj; ++i) {
    REQUIRE(traj_len[i] >= 0, "ampc_kstep_errors_mlp: negative trajectory length");
    total += traj_len[i];
  }
  REQUIRE(total == 0 || (obs && ctrls), "ampc_kstep_errors_mlp: NULL obs / ctrls");
  KstepMlpPrep prep;
  if (int rc = kstep_mlp_prepare(n_models, n_hidden, dims, activations, weights, biases, norms, on_device, nx, nu,
                                 obs_dim, &prep))
    return rc;
  int n_dev = 0;
  REQUIRE(hipGetDeviceCount(&n_dev) == hipSuccess && n_dev > 0, "ampc_kstep_errors_mlp: no HIP device visible");
  REQUIRE(device >= 0 && device < n_dev, "ampc_kstep_errors_mlp: no such device");
  HIP_OK(hipSetDevice(device));
  const int ML = prep.max_layers;
  for (int k = 0; k < n_models; ++k) {
    if (!on_device[k]) continue;
    for (int l = 0; l <= n_hidden[k]; ++l) {
      if (int rc = km_on_device(weights[(size_t)k * ML + l], device)) return rc;
      if (int rc = km_on_device(biases[(size_t)k * ML + l], device)) return rc;
    }
    for (int i = 0; i < 4; ++i)
      if (int rc = km_on_device(norms[(size_t)k * 4 + i], device)) return rc;
  }
  hipStream_t st = nullptr;
  ScopedBuf d_stage, d_models;
  if (!prep.stage.empty()) {
    HIP_OK(d_stage.reserve(prep.stage.size() * 8));
    HIP_OK(hipMemcpyAsync(d_stage.p, prep.stage.data(), prep.stage.size() * 8, hipMemcpyHostToDevice, st));
  }
  const size_t mb = kstep_mlp_model_bytes();
  std::vector<char> table((size_t)n_models * mb);
  const double* sb = (const double*)d_stage.p;
  for (int k = 0; k < n_models; ++k) {
    const double* w[8] = {nullptr};
    const double* b[8] = {nullptr};
    const double* nm[4];
    for (int l = 0; l <= n_hidden[k]; ++l) {
      const size_t e = (size_t)k * ML + l;
      w[l] = on_device[k] ? weights[e] : sb + prep.w_off[e];
      b[l] = on_device[k] ? biases[e] : sb + prep.b_off[e];
    }
    for (int i = 0; i < 4; ++i) nm[i] = on_device[k] ? norms[(size_t)k * 4 + i] : sb + prep.n_off[(size_t)k * 4 + i];
    kstep_mlp_pack_model(table.data() + (size_t)k * mb, n_hidden[k] + 1, activations[k], dims + (size_t)k * (ML + 1),
                         w, b, nm);
  }
  HIP_OK(d_models.reserve(table.size()));
  HIP_OK(hipMemcpyAsync(d_models.p, table.data(), table.size(), hipMemcpyHostToDevice, st));
  HIP_OK(hipStreamSynchronize(st));            // `table` and `prep` may go out of scope on any path from here
  return kstep_mlp_launch(st, n_models, d_models.p, nx, nu, n_traj, traj_len, obs, ctrls, kmax, inv_std, sq_err,
                          sq_delta_err);
}
