// ilqr_table_hostcheck.cpp -- the host half of ampc_ilqr_plan_set_model_table (csrc/ilqr_table_host.hpp: the checks of
// the plan and of the model arguments, the LDS map of the table iteration kernel, the extent of the stored derivatives;
// csrc/api_kstep_mlp.cpp: the packing of host-resident parameters) as a stand-alone program for the host sanitizers, in
// the manner of mppi_table_hostcheck.cpp.  It links api_kstep_mlp.cpp alone, supplies what that unit takes from the rest
// of the library, and makes no device call: ilqr_table_check has none, and the k-step launcher must never be reached.
//
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -I include -I autompc_amd/csrc \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         tools/ilqr_table_hostcheck.cpp autompc_amd/csrc/api_kstep_mlp.cpp -fsanitize=address,undefined -o hostcheck
//   ./hostcheck            (prints "ilqr_table_hostcheck: N checks passed"; any sanitizer report fails it)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "autompc_hip.h"
#include "ilqr_table_host.hpp"

thread_local std::string g_err;
extern "C" const char* ampc_last_error(void) { return g_err.c_str(); }

// -- what launch_kstep_mlp.cpp provides in the library -------------------------------------------------------------
size_t kstep_mlp_model_bytes() { return 8 + 6 * 4 + 14 * 8; }
void kstep_mlp_limits(int out[5]) { out[0] = 4; out[1] = 256; out[2] = 80; out[3] = 64; out[4] = 16; }
void kstep_mlp_pack_model(void*, int, int, const int*, const double* const*, const double* const*, const double* const*) {
  std::fprintf(stderr, "ilqr_table_hostcheck: the table packer was reached\n");
  std::abort();
}
struct ihipStream_t;
int kstep_mlp_launch(ihipStream_t*, int, const void*, int, int, int, const int*, const double*, const double*, int,
                     const double*, double*, double*) {
  std::fprintf(stderr, "ilqr_table_hostcheck: the k-step launcher was reached\n");
  std::abort();
}

static int n_checks = 0;
#define CHECK(cond)                                                                        \
  do {                                                                                     \
    if (!(cond)) { std::fprintf(stderr, "FAILED line %d: %s (last error: %s)\n", __LINE__, #cond, g_err.c_str()); return 1; } \
    ++n_checks;                                                                            \
  } while (0)

constexpr int kBase = 9808;                  // ilqr_table_lds_base(): act[2][16][257] + xu[16][81] + norm[288], in doubles
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
  int check(const IlqrTablePlanView& v, KstepMlpPrep* p) const {
    return ilqr_table_check(v, (int)n_hidden.size(), n_hidden.data(), dims.data(), acts.data(), w.data(), b.data(),
                            norm.data(), on_device.data(), kBase, kLimit, p);
  }
};

static IlqrTablePlanView view(int nx, int nu) {
  IlqrTablePlanView v{};
  v.f64 = 1; v.has_mlp = 1; v.nx = nx; v.nu = nu; v.obs_dim = nx;
  v.cost_stride = (2 * nx * nx + nu * nu + 3 * nx + 2 + 3) / 4 * 4;
  return v;
}

static bool refused(int rc, const char* what, int code = -1) {
  return rc == code && g_err.find("ampc_ilqr_plan_set_model_table: ") == 0 && g_err.find(what) != std::string::npos;
}

int main() {
  KstepMlpPrep p;
  // an accepted table: the packing of the host-resident models, re-read against the sources
  Batch ok{17, 6};
  ok.add({64, 16, 48, 128}, 3);
  ok.add({256, 256}, 0, /*resident=*/1);     // (its addresses are never dereferenced on the host)
  ok.add({1, 40}, 2);
  const IlqrTablePlanView v = view(17, 6);
  CHECK(ok.check(v, &p) == 0);
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
  // the extent of the stored derivatives: the widest hidden layer rounded up to 16, the most hidden layers
  int wmax = 0, hmax = 0;
  ilqr_table_extent(3, ok.n_hidden.data(), ok.dims.data(), 5, &wmax, &hmax);
  CHECK(wmax == 256 && hmax == 4);
  { Batch x{17, 6}; x.add({17, 33}, 1); x.add({1}, 0);
    ilqr_table_extent(2, x.n_hidden.data(), x.dims.data(), 5, &wmax, &hmax); CHECK(wmax == 48 && hmax == 2); }
  { Batch x{17, 6}; x.add({1}, 0);
    ilqr_table_extent(1, x.n_hidden.data(), x.dims.data(), 5, &wmax, &hmax); CHECK(wmax == 16 && hmax == 1); }
  // the limits themselves are accepted: the widest, deepest networks at the sweep's 63 inputs
  Batch edge{47, 16};
  edge.add({256, 256, 256, 256}, 1);
  edge.add({1}, 0);
  CHECK(edge.check(view(47, 16), &p) == 0);
  { Batch x{62, 1}; x.add({16}, 0); CHECK(x.check(view(62, 1), &p) == 0); }

  // the work region and the LDS map: 17 / 6, and the largest map inside the entry's limits (62 states, one control)
  const IlqrTableWork wk = make_ilqr_table_work(17, 6, v.cost_stride);
  CHECK(wk.K == 0 && wk.k == 102 && wk.ubar == 108 && wk.xbar == 114 && wk.cpar == 131 && wk.lo == 131 + v.cost_stride);
  CHECK(wk.total == 102 + 6 + 6 + 17 + v.cost_stride + 6 + 6 + 16 + 16 + 8);
  CHECK(ilqr_table_lds_bytes(kBase, 17, 6, v.cost_stride) == (size_t)(kBase + wk.total) * 8);
  CHECK(ilqr_table_lds_bytes(kBase, 62, 1, view(62, 1).cost_stride) == 142848);
  CHECK(ilqr_table_lds_bytes(kBase, 47, 16, view(47, 16).cost_stride) <= kLimit);

  // refusals of the plan
  { IlqrTablePlanView x = v; x.f64 = 0; CHECK(refused(ok.check(x, &p), "f64 only")); }
  { IlqrTablePlanView x = v; x.has_mlp = 0; CHECK(refused(ok.check(x, &p), "not an MLP")); }
  { IlqrTablePlanView x = v; x.n_shape_models = 3; CHECK(refused(ok.check(x, &p), "ampc_ilqr_plan_set_models")); }
  { Batch x{48, 16}; x.add({16}, 0); CHECK(refused(x.check(view(48, 16), &p), "must be <= 63")); }
  // the LDS refusal carries its own code.  Inside the other limits no cost block is large enough (above), so the
  // views below state a cost stride no handle of these dimensions has: the code path, not a reachable plan.
  { IlqrTablePlanView x = v; x.cost_stride = 10560; CHECK(refused(ok.check(x, &p), "more than 160 KB", kIlqrTableNoFit)); }
  { IlqrTablePlanView x = v; x.cost_stride = 10490; CHECK(refused(ok.check(x, &p), "more than 160 KB", kIlqrTableNoFit)); }
  { IlqrTablePlanView x = v; x.cost_stride = 10489; CHECK(ok.check(x, &p) == 0); }
  // ... of the arguments
  { Batch none{17, 6}; CHECK(refused(none.check(v, &p), "NULL argument")); }
  CHECK(refused(ilqr_table_check(v, 1, nullptr, ok.dims.data(), ok.acts.data(), ok.w.data(), ok.b.data(), ok.norm.data(),
                                 ok.on_device.data(), kBase, kLimit, &p), "NULL model argument"));
  // ... of the models: other dimensions than the handle's, obs_dim != nx, the limits of the table kernels
  { Batch x{16, 6}; x.add({16}, 0); CHECK(refused(x.check(v, &p), "nx + nu inputs and gives nx outputs")); }
  { Batch x{17, 5}; x.add({16}, 0); CHECK(refused(x.check(v, &p), "nx + nu inputs and gives nx outputs")); }
  { IlqrTablePlanView x = v; x.obs_dim = 16; CHECK(refused(ok.check(x, &p), "obs_dim must be the models' state dim")); }
  { Batch x{17, 6}; x.add({16, 16, 16, 16}, 0); x.n_hidden[0] = 5; CHECK(refused(x.check(v, &p), "1..4 hidden layers")); }
  { Batch x{17, 6}; x.add({16}, 0); x.n_hidden[0] = 0; CHECK(refused(x.check(v, &p), "1..4 hidden layers")); }
  { Batch x{17, 6}; x.add({16, 257}, 0); CHECK(refused(x.check(v, &p), "hidden widths must be in 1..256")); }
  { Batch x{17, 6}; x.add({16}, 4); CHECK(refused(x.check(v, &p), "activation must be")); }
  { Batch x{17, 6}; x.add({16}, 0); x.add({16, 16}, 1); x.b[5 + 2] = nullptr; CHECK(refused(x.check(v, &p), "NULL weight or bias")); }
  { Batch x{17, 6}; x.add({16}, 0); x.norm[3] = nullptr; CHECK(refused(x.check(v, &p), "NULL normaliser")); }
  { Batch x{8, 17}; x.add({16}, 0); CHECK(refused(x.check(view(8, 17), &p), "ctrl_dim (nu) must be in 1..16")); }
  std::printf("ilqr_table_hostcheck: %d checks passed\n", n_checks);
  return 0;
}
