// kstep_mlp_host.hpp -- the host half of ampc_kstep_errors_mlp that makes no device call (api_kstep_mlp.cpp): the
// checks of the model arguments and the packing of host-resident parameters into one upload.
#pragma once
#include <vector>

struct KstepMlpPrep {
  int n_models = 0, max_layers = 0;
  // every host-resident model's parameters: layer after layer the weight [out][in] and the bias [out], then xu_mean,
  // xu_std, dy_mean, dy_std
  std::vector<double> stage;
  // offsets into `stage` in doubles, -1 for a device-resident model: [n_models][max_layers] / [n_models][4]
  std::vector<long long> w_off, b_off, n_off;
};

// Arguments as ampc_kstep_errors_mlp takes them (include/autompc_hip.h).  Returns 0, or -1 with the message set.
int kstep_mlp_prepare(int n_models, const int* n_hidden, const int* dims, const int* activations,
                      const double* const* weights, const double* const* biases, const double* const* norms,
                      const int* on_device, int nx, int nu, int obs_dim, KstepMlpPrep* out);
