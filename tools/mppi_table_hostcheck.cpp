// mppi_table_hostcheck.cpp -- the host half of ampc_mppi_plan_set_model_table (csrc/mppi_table_host.hpp: the checks of
// the plan and of the model arguments, the LDS size of the table kernel's map; csrc/api_kstep_mlp.cpp: the packing of
// host-resident parameters) as a stand-alone program for the host sanitizers, in the manner of kstep_mlp_hostcheck.cpp.
// It links api_kstep_mlp.cpp alone, supplies what that unit takes from the rest of the library, and makes no device
// call: mppi_table_check has none, and the k-step launcher must never be reached.
//
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -I include -I autompc_amd/csrc \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         tools/mppi_table_hostcheck.cpp autompc_amd/csrc/api_kstep_mlp.cpp -fsanitize=address,undefined -o hostcheck
//   ./hostcheck            (prints "mppi_table_hostcheck: N checks passed"; any sanitizer report fails it)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "autompc_hip.h"
#include "mppi_table_host.hpp"

thread_local std::string g_err;
extern "C" const char* ampc_last_error(void) { return g_err.c_str(); }

// -- what launch_kstep_mlp.cpp provides in the library -------------------------------------------------------------
size_t kstep_mlp_model_bytes() { return 8 + 6 * 4 + 14 * 8; }
void kstep_mlp_limits(int out[5]) { out[0] = 4; out[1] = 256; out[2] = 80; out[3] = 64; out[4] = 16; }
void kstep_mlp_pack_model(void*, int, int, const int*, const double* const*, const double* const*, const double* const*) {
  std::fprintf(stderr, "mppi_table_hostcheck: the table packer was reached\n");
  std::abort();
}
struct ihipStream_t;
int kstep_mlp_launch(ihipStream_t*, int, const void*, int, int, int, const int*, const double*, const double*, int,
                     const double*, double*, double*) {
  std::fprintf(stderr, "mppi_table_hostcheck: the k-step launcher was reached\n");
  std::abort();
}

static int n_checks = 0;
#define CHECK(cond)                                                                        \
  do {                                                                                     \
    if (!(cond)) { std::fprintf(stderr, "FAILED line %d: %s (last error: %s)\n", __LINE__, #cond, g_err.c_str()); return 1; } \
    ++n_checks;                                                                            \
  } while (0)

constexpr int kBase = 9808;                  // mppi_table_lds_base(): act[2][16][257] + xu[16][81] + norm[288], in doubles
constexpr size_t kLimit = 160 * 1024;

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
  int check(const MppiTablePlanView& v, const std::vector<int>& index, KstepMlpPrep* p) const {
    return mppi_table_check(v, (int)n_hidden.size(), n_hidden.data(), dims.data(), acts.data(), w.data(), b.data(),
                            norm.data(), on_device.data(), index.empty() ? nullptr : index.data(), kBase, kLimit, p);
  }
};

static MppiTablePlanView view(int nx, int nu, int B, int max_h) {
  MppiTablePlanView v{};
  v.f64 = 1; v.has_mlp = 1; v.nx = nx; v.nu = nu; v.obs_dim = nx; v.B = B; v.max_h = max_h;
  v.cost_stride = (2 * nx * nx + nu * nu + 3 * nx + 2 + 3) / 4 * 4;
  return v;
}

static bool refused(int rc, const char* what, int code = -1) {
  return rc == code && g_err.find("ampc_mppi_plan_set_model_table: ") == 0 && g_err.find(what) != std::string::npos;
}

int main() {
  KstepMlpPrep p;
  // an accepted table: the packing of the host-resident models, re-read against the sources
  Batch ok{17, 6};
  ok.add({64, 16, 48, 128}, 3);
  ok.add({256, 256}, 0, /*resident=*/1);     // (its addresses are never dereferenced on the host)
  ok.add({1, 40}, 2);
  const MppiTablePlanView v = view(17, 6, 4, 30);
  CHECK(ok.check(v, {2, 0, 1, 1}, &p) == 0);
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
    for (int i = 0; i < 4; ++i) {
      const size_t n = i < 2 ? 23 : 17;
      CHECK(p.n_off[k * 4 + i] == (long long)expect);
      CHECK(std::memcmp(&p.stage[expect], ok.norm[k * 4 + i], n * 8) == 0);
      expect += n;
    }
  }
  CHECK(p.stage.size() == expect);
  for (int l = 0; l < 5; ++l) CHECK(p.w_off[5 + l] == -1 && p.b_off[5 + l] == -1);
  // the limits themselves are accepted
  Batch edge{64, 16};
  edge.add({256, 256, 256, 256}, 1);
  edge.add({1}, 0);
  CHECK(edge.check(view(64, 16, 2, 30), {1, 0}, &p) == 0);

  // the LDS map: 17 / 6 at horizon 30 fused, 8 / 16 at horizon caps 30 and 40, 64 / 16 with a dense block
  CHECK(mppi_table_lds_bytes(kBase, v.cost_stride, 6, 30, true) == (size_t)(10676 + 2880 + 32) * 8);
  CHECK(mppi_table_lds_bytes(kBase, v.cost_stride, 6, 30, false) == (size_t)10676 * 8);
  CHECK(mppi_table_lds_bytes(kBase, view(8, 16, 1, 30).cost_stride, 16, 30, true) == 147680);
  CHECK(mppi_table_lds_bytes(kBase, view(8, 16, 1, 40).cost_stride, 16, 40, true) == 169440);
  CHECK(mppi_table_lds_bytes(kBase, view(8, 16, 1, 40).cost_stride, 16, 40, false) <= kLimit);
  CHECK(mppi_table_lds_bytes(kBase, view(64, 16, 1, 5).cost_stride, 16, 5, false) == 148640);
  CHECK(mppi_table_lds_bytes(kBase, view(64, 16, 1, 30).cost_stride, 16, 30, true) > kLimit);

  // refusals of the plan
  { MppiTablePlanView x = v; x.f64 = 0; CHECK(refused(ok.check(x, {0, 0, 0, 0}, &p), "f64 only")); }
  { MppiTablePlanView x = v; x.has_mlp = 0; CHECK(refused(ok.check(x, {0, 0, 0, 0}, &p), "not an MLP")); }
  { MppiTablePlanView x = v; x.n_ind = 1; CHECK(refused(ok.check(x, {0, 0, 0, 0}, &p), "indicator cost terms")); }
  { MppiTablePlanView x = v; x.lift_n = 2; CHECK(refused(ok.check(x, {0, 0, 0, 0}, &p), "state lift")); }
  { MppiTablePlanView x = v; x.n_shape_models = 3; CHECK(refused(ok.check(x, {0, 0, 0, 0}, &p), "ampc_mppi_plan_set_models")); }
  { MppiTablePlanView x = view(64, 16, 1, 200); CHECK(refused(edge.check(x, {0}, &p), "more than 160 KB", kMppiTableNoFit)); }
  { MppiTablePlanView x = view(64, 16, 1, 130); CHECK(refused(edge.check(x, {0}, &p), "more than 160 KB", kMppiTableNoFit)); }
  { MppiTablePlanView x = view(64, 16, 1, 120); CHECK(edge.check(x, {0}, &p) == 0); }
  // ... of the model index
  CHECK(refused(ok.check(v, {}, &p), "NULL argument"));
  CHECK(refused(ok.check(v, {0, 1, 2, 3}, &p), "model_index out of range"));
  CHECK(refused(ok.check(v, {0, -1, 2, 1}, &p), "model_index out of range"));
  { Batch none{17, 6}; CHECK(refused(none.check(v, {0, 0, 0, 0}, &p), "NULL argument")); }
  // ... of the models: other dimensions than the handle's, obs_dim != nx, the limits of the table kernel
  { Batch x{16, 6}; x.add({16}, 0); CHECK(refused(x.check(v, {0, 0, 0, 0}, &p), "nx + nu inputs and gives nx outputs")); }
  { Batch x{17, 5}; x.add({16}, 0); CHECK(refused(x.check(v, {0, 0, 0, 0}, &p), "nx + nu inputs and gives nx outputs")); }
  { MppiTablePlanView x = v; x.obs_dim = 16; CHECK(refused(ok.check(x, {0, 0, 0, 0}, &p), "obs_dim must be the models' state dim")); }
  { Batch x{17, 6}; x.add({16, 16, 16, 16}, 0); x.n_hidden[0] = 5; CHECK(refused(x.check(v, {0, 0, 0, 0}, &p), "1..4 hidden layers")); }
  { Batch x{17, 6}; x.add({16}, 0); x.n_hidden[0] = 0; CHECK(refused(x.check(v, {0, 0, 0, 0}, &p), "1..4 hidden layers")); }
  { Batch x{17, 6}; x.add({16, 257}, 0); CHECK(refused(x.check(v, {0, 0, 0, 0}, &p), "hidden widths must be in 1..256")); }
  { Batch x{17, 6}; x.add({16}, 4); CHECK(refused(x.check(v, {0, 0, 0, 0}, &p), "activation must be")); }
  { Batch x{17, 6}; x.add({16}, 0); x.add({16, 16}, 1); x.b[5 + 2] = nullptr; CHECK(refused(x.check(v, {0, 1, 0, 0}, &p), "NULL weight or bias")); }
  { Batch x{17, 6}; x.add({16}, 0); x.norm[3] = nullptr; CHECK(refused(x.check(v, {0, 0, 0, 0}, &p), "NULL normaliser")); }
  { Batch x{65, 2}; x.add({16}, 0); CHECK(refused(x.check(view(65, 2, 1, 30), {0}, &p), "state dim (nx) must be in 1..64")); }
  { Batch x{8, 17}; x.add({16}, 0); CHECK(refused(x.check(view(8, 17, 1, 30), {0}, &p), "ctrl_dim (nu) must be in 1..16")); }
  { Batch x{64, 16}; x.add({16}, 0); MppiTablePlanView y = view(64, 16, 1, 30); y.nu = 17; y.nx = 64;
    CHECK(refused(x.check(y, {0}, &p), "ctrl_dim (nu) must be in 1..16")); }
  std::printf("mppi_table_hostcheck: %d checks passed\n", n_checks);
  return 0;
}
