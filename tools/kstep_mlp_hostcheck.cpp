// kstep_mlp_hostcheck.cpp -- the host half of ampc_kstep_errors_mlp (csrc/api_kstep_mlp.cpp: argument checks and the
// packing of host-resident parameters) as a stand-alone program for the host sanitizers.  It links that ONE translation
// unit, supplies the pieces the unit takes from the rest of the library (the error slot, the kernel unit's limits and
// table packer, a launcher that must never be reached) and makes no device call past validation: every refusal below
// returns before the first HIP call, and the packing is run through kstep_mlp_prepare, which has none.
//
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -I include -I autompc_amd/csrc \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         tools/kstep_mlp_hostcheck.cpp autompc_amd/csrc/api_kstep_mlp.cpp -fsanitize=address,undefined -o hostcheck
//   ./hostcheck            (prints "kstep_mlp_hostcheck: N checks passed"; any sanitizer report fails it)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "autompc_hip.h"
#include "kstep_mlp_host.hpp"

thread_local std::string g_err;
extern "C" const char* ampc_last_error(void) { return g_err.c_str(); }

// -- what launch_kstep_mlp.cpp provides in the library -------------------------------------------------------------
struct HostModel {              // KstepMlpModel's layout (kstep_mlp_kernels.hpp), host side
  int n_layers, act, dims[6];
  const double* w[5];
  const double* b[5];
  const double* norm[4];
};
size_t kstep_mlp_model_bytes() { return sizeof(HostModel); }
void kstep_mlp_limits(int out[5]) { out[0] = 4; out[1] = 256; out[2] = 80; out[3] = 64; out[4] = 16; }
void kstep_mlp_pack_model(void* dst, int n_layers, int act, const int* dims, const double* const* w,
                          const double* const* b, const double* const* norm) {
  HostModel m{};
  m.n_layers = n_layers; m.act = act;
  for (int l = 0; l <= n_layers; ++l) m.dims[l] = dims[l];
  for (int l = 0; l < n_layers; ++l) { m.w[l] = w[l]; m.b[l] = b[l]; }
  for (int i = 0; i < 4; ++i) m.norm[i] = norm[i];
  std::memcpy(dst, &m, sizeof m);
}
struct ihipStream_t;
int kstep_mlp_launch(ihipStream_t*, int, const void*, int, int, int, const int*, const double*, const double*, int,
                     const double*, double*, double*) {
  std::fprintf(stderr, "kstep_mlp_hostcheck: the launcher was reached\n");
  std::abort();
}

static int n_checks = 0;
#define CHECK(cond)                                                                        \
  do {                                                                                     \
    if (!(cond)) { std::fprintf(stderr, "FAILED line %d: %s (last error: %s)\n", __LINE__, #cond, g_err.c_str()); return 1; } \
    ++n_checks;                                                                            \
  } while (0)

struct Batch {                  // exactly-sized heap arrays: an over-read by the packer is a sanitizer report
  int nx, nu;
  std::vector<int> n_hidden, dims, acts, on_device;
  std::vector<std::vector<double>> store;
  std::vector<const double*> w, b, norm;
  void add(std::vector<int> hidden, int act, int resident = 0) {
    const int k = (int)n_hidden.size();
    n_hidden.push_back((int)hidden.size()); acts.push_back(act); on_device.push_back(resident);
    std::vector<int> d{nx + nu};
    d.insert(d.end(), hidden.begin(), hidden.end());
    d.push_back(nx);
    dims.resize((size_t)(k + 1) * 6, 0); w.resize((size_t)(k + 1) * 5, nullptr); b.resize((size_t)(k + 1) * 5, nullptr);
    for (size_t i = 0; i < d.size(); ++i) dims[(size_t)k * 6 + i] = d[i];
    auto fill = [&](size_t n, double seed) {
      store.emplace_back(n);
      for (size_t i = 0; i < n; ++i) store.back()[i] = seed + 1e-3 * (double)i;
      return store.back().data();
    };
    for (size_t l = 0; l + 1 < d.size(); ++l) {
      w[(size_t)k * 5 + l] = fill((size_t)d[l + 1] * d[l], 100.0 * k + 10.0 * (double)l);
      b[(size_t)k * 5 + l] = fill((size_t)d[l + 1], 100.0 * k + 10.0 * (double)l + 5.0);
    }
    for (int i = 0; i < 4; ++i) norm.push_back(fill(i < 2 ? nx + nu : nx, 1000.0 * k + i));
  }
  int prepare(KstepMlpPrep* p, int obs_dim) const {
    return kstep_mlp_prepare((int)n_hidden.size(), n_hidden.data(), dims.data(), acts.data(), w.data(), b.data(),
                             norm.data(), on_device.data(), nx, nu, obs_dim, p);
  }
  int entry(int obs_dim, int kmax, double* S, const int* lens = nullptr, int n_traj = 0) const {
    return ampc_kstep_errors_mlp(0, (int)n_hidden.size(), n_hidden.data(), dims.data(), acts.data(), w.data(), b.data(),
                                 norm.data(), on_device.data(), nx, nu, n_traj, lens, obs_dim, nullptr, nullptr, kmax,
                                 nullptr, S, nullptr);
  }
};

static bool refused(int rc, const char* what) { return rc != 0 && g_err.find(what) != std::string::npos; }

int main() {
  // the packing of host-resident models, re-read against the sources; a device-resident model is skipped
  Batch ok{17, 6};
  ok.add({37, 16, 200, 256}, 3);
  ok.add({256}, 0, /*resident=*/1);        // (its addresses are never dereferenced on the host)
  ok.add({1, 255}, 2);
  KstepMlpPrep p;
  CHECK(ok.prepare(&p, 17) == 0);
  CHECK(p.n_models == 3 && p.max_layers == 5 && p.w_off.size() == 15 && p.n_off.size() == 12);
  size_t expect = 0;
  for (int k : {0, 2}) {
    const int L = ok.n_hidden[k] + 1;
    const int* d = &ok.dims[(size_t)k * 6];
    for (int l = 0; l < L; ++l) {
      const size_t nw = (size_t)d[l + 1] * d[l], nb = (size_t)d[l + 1];
      CHECK(p.w_off[k * 5 + l] == (long long)expect);
      CHECK(std::memcmp(&p.stage[expect], ok.w[k * 5 + l], nw * 8) == 0);
      expect += nw;
      CHECK(p.b_off[k * 5 + l] == (long long)expect);
      CHECK(std::memcmp(&p.stage[expect], ok.b[k * 5 + l], nb * 8) == 0);
      expect += nb;
    }
    for (int l = L; l < 5; ++l) CHECK(p.w_off[k * 5 + l] == -1 && p.b_off[k * 5 + l] == -1);
    for (int i = 0; i < 4; ++i) {
      const size_t n = i < 2 ? 23 : 17;
      CHECK(p.n_off[k * 4 + i] == (long long)expect);
      CHECK(std::memcmp(&p.stage[expect], ok.norm[k * 4 + i], n * 8) == 0);
      expect += n;
    }
  }
  CHECK(p.stage.size() == expect);
  for (int l = 0; l < 5; ++l) CHECK(p.w_off[5 + l] == -1 && p.b_off[5 + l] == -1);
  for (int i = 0; i < 4; ++i) CHECK(p.n_off[4 + i] == -1);
  // the limits themselves are accepted
  Batch edge{64, 16};
  edge.add({256, 256, 256, 256}, 1);
  edge.add({1}, 0);
  CHECK(edge.prepare(&p, 64) == 0);
  CHECK(p.stage.size() == (size_t)(256 * 80 + 256 + 3 * (256 * 256 + 256) + 64 * 256 + 64 + 2 * 80 + 2 * 64) +
                              (size_t)(80 + 1 + 64 + 64 + 2 * 80 + 2 * 64));

  // refusals of the entry, every one before the first device call
  double S[64];
  CHECK(refused(ok.entry(17, 0, S), "kmax must be >= 1"));
  CHECK(refused(ok.entry(17, 3, nullptr), "NULL sq_err"));
  CHECK(refused(ok.entry(17, 3, S, nullptr, 2), "NULL trajectory lengths"));
  const int neg[2] = {5, -1};
  CHECK(refused(ok.entry(17, 3, S, neg, 2), "negative trajectory length"));
  const int lens[2] = {5, 3};
  CHECK(refused(ok.entry(17, 3, S, lens, 2), "NULL obs / ctrls"));
  CHECK(refused(ok.entry(16, 3, S), "obs_dim must be the models' state dim"));
  CHECK(refused(ampc_kstep_errors_mlp(0, 0, ok.n_hidden.data(), ok.dims.data(), ok.acts.data(), ok.w.data(),
                                      ok.b.data(), ok.norm.data(), ok.on_device.data(), 17, 6, 0, nullptr, 17, nullptr,
                                      nullptr, 3, nullptr, S, nullptr), "no models"));
  CHECK(refused(ampc_kstep_errors_mlp(0, 3, ok.n_hidden.data(), nullptr, ok.acts.data(), ok.w.data(), ok.b.data(),
                                      ok.norm.data(), ok.on_device.data(), 17, 6, 0, nullptr, 17, nullptr, nullptr, 3,
                                      nullptr, S, nullptr), "NULL model argument"));
  { Batch x{17, 6}; x.add({16, 16, 16, 16}, 0); x.n_hidden[0] = 5; CHECK(refused(x.entry(17, 3, S), "1..4 hidden layers")); }
  { Batch x{17, 6}; x.add({16}, 0); x.n_hidden[0] = 0; CHECK(refused(x.entry(17, 3, S), "1..4 hidden layers")); }
  { Batch x{17, 6}; x.add({16, 257}, 0); CHECK(refused(x.entry(17, 3, S), "hidden widths must be in 1..256")); }
  { Batch x{17, 6}; x.add({16}, 0); x.dims[1] = 0; CHECK(refused(x.entry(17, 3, S), "hidden widths must be in 1..256")); }
  { Batch x{17, 6}; x.add({16}, 4); CHECK(refused(x.entry(17, 3, S), "activation must be")); }
  { Batch x{17, 6}; x.add({16}, 0); x.dims[0] = 22; CHECK(refused(x.entry(17, 3, S), "nx + nu inputs and gives nx outputs")); }
  { Batch x{17, 6}; x.add({16}, 0); x.dims[2] = 16; CHECK(refused(x.entry(17, 3, S), "nx + nu inputs and gives nx outputs")); }
  { Batch x{17, 6}; x.add({16}, 0); x.add({16, 16}, 1); x.b[5 + 2] = nullptr; CHECK(refused(x.entry(17, 3, S), "NULL weight or bias")); }
  { Batch x{17, 6}; x.add({16}, 0); x.norm[3] = nullptr; CHECK(refused(x.entry(17, 3, S), "NULL normaliser")); }
  { Batch x{65, 2}; x.add({16}, 0); CHECK(refused(x.entry(65, 3, S), "state dim (nx) must be in 1..64")); }
  { Batch x{8, 17}; x.add({16}, 0); CHECK(refused(x.entry(8, 3, S), "ctrl_dim (nu) must be in 1..16")); }
  { Batch x{8, 0}; x.add({16}, 0); CHECK(refused(x.entry(8, 3, S), "ctrl_dim (nu) must be in 1..16")); }
  std::printf("kstep_mlp_hostcheck: %d checks passed\n", n_checks);
  return 0;
}
