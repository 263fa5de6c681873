// ilqr_sindy_table_hostcheck.cpp -- the host half of ampc_ilqr_plan_set_sindy_models (csrc/ilqr_sindy_table_host.hpp:
// the checks of the plan and of the model handles, the selection rule between the two bodies of the iteration kernel,
// the LDS maps of both kernels) as a stand-alone program for the host sanitizers, in the manner of
// ilqr_table_hostcheck.cpp.  It makes no device call: the header has none.
//
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -I include -I autompc_amd/csrc \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         tools/ilqr_sindy_table_hostcheck.cpp -fsanitize=address,undefined -o hostcheck
//   ./hostcheck            (prints "ilqr_sindy_table_hostcheck: N checks passed"; any sanitizer report fails it)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ilqr_sindy_table_host.hpp"

thread_local std::string g_err;

static int n_checks = 0;
#define CHECK(cond)                                                                        \
  do {                                                                                     \
    if (!(cond)) { std::fprintf(stderr, "FAILED line %d: %s (last error: %s)\n", __LINE__, #cond, g_err.c_str()); return 1; } \
    ++n_checks;                                                                            \
  } while (0)

constexpr size_t kLimit = 160 * 1024;

// a handle's view as ampc_set_sindy would leave it: the product table unless it exceeds 160 entries, staging up to 48 KB
static IlqrSindyView view(int nx, int nu, int n_feat, int n_trig, int n_pow, int n_mon, int n_pool) {
  IlqrSindyView v;
  std::memset(&v, 0, sizeof(v));
  v.f64 = 1; v.has_sindy = 1; v.device = 0; v.nx = nx; v.nu = nu; v.obs_dim = nx;
  v.n_feat = n_feat; v.n_pool = n_pool;
  const int n_tab = 2 * n_trig + n_pow + n_mon + 1;
  if (n_tab <= 160) { v.n_trig = n_trig; v.n_pow = n_pow; v.n_mon = n_mon; v.n_tab = n_tab; }
  if (v.n_tab > 0) {
    const size_t elems = ilqr_sindy_prog_elems(nx, n_feat, v.n_trig, v.n_pow, v.n_mon, n_pool) - 2;
    v.stage = elems * 8 <= 48 * 1024 ? 1 : 0;
  }
  return v;
}

static bool refused(int rc, const char* text, int code = -1) {
  return rc == code && g_err.find("ampc_ilqr_plan_set_sindy_models: ") == 0 && g_err.find(text) != std::string::npos;
}

static int check(const IlqrSindyView& plan, int cost_stride, std::vector<IlqrSindyView> ms, size_t* need = nullptr,
                 int n_shape = 0, int n_table = 0, size_t limit = kLimit) {
  std::vector<const IlqrSindyView*> p;
  for (const IlqrSindyView& m : ms) p.push_back(&m);
  return ilqr_sindy_table_check(plan, cost_stride, n_shape, n_table, (int)p.size(), p.data(), limit, need);
}

int main() {
  // ---- the models of the tests' sets (tests/mppi_sindy_table_cases.py), as ampc_set_sindy lays them out
  const IlqrSindyView poly3trig2 = view(3, 2, 35, 10, 10, 0, 0);       // 5 variables: id, 2 x (sin, cos), powers 2, 3
  const IlqrSindyView cross3 = view(3, 2, 45, 0, 10, 30, 70);          // few monomials: a table
  const IlqrSindyView cross5 = view(3, 2, 251, 0, 20, 226, 700);       // 247 entries: direct evaluation
  const IlqrSindyView c1 = view(4, 1, 55, 5, 0, 0, 0);                 // CartPole library with interaction terms
  const IlqrSindyView hc = view(17, 6, 69, 23, 0, 0, 0);               // more than eight states
  const IlqrSindyView hcx = view(17, 6, 1081, 23, 0, 0, 0);            // 1081 features: a 147 KB program, not staged
  CHECK(ilqr_sindy_table_spread(poly3trig2.n_tab, 3, poly3trig2.stage));
  CHECK(ilqr_sindy_table_spread(cross3.n_tab, 3, cross3.stage));
  CHECK(cross5.n_tab == 0 && cross5.stage == 0 && !ilqr_sindy_table_spread(cross5.n_tab, 3, cross5.stage));
  CHECK(c1.n_tab == 11 && c1.stage == 1 && ilqr_sindy_table_spread(c1.n_tab, 4, c1.stage));
  CHECK(hc.stage == 1 && !ilqr_sindy_table_spread(hc.n_tab, 17, hc.stage));
  CHECK(hcx.n_tab == 47 && hcx.stage == 0 && !ilqr_sindy_table_spread(hcx.n_tab, 17, hcx.stage));
  CHECK(ilqr_sindy_table_spread(11, 8, 1) && !ilqr_sindy_table_spread(11, 9, 1) && !ilqr_sindy_table_spread(0, 4, 1) &&
        !ilqr_sindy_table_spread(11, 4, 0));

  // ---- the LDS maps: offsets follow the plan's constants and the entry's n_tab only
  {
    const int cs = 3 * 3 * 2 + 2 * 2 + 3 * 3 + 4;                      // a cost block of a 3 / 2 plan (any value does)
    const IlqrSindyLds a = make_ilqr_sindy_lds(3, 2, cs, 21, 0), b = make_ilqr_sindy_lds(3, 2, cs, 21, 1000);
    CHECK(a.work == 0 && a.xu == b.xu && a.xn == b.xn && a.tab == b.tab && a.prog == b.prog);
    CHECK(b.total == a.total + 1000 && a.total == (size_t)a.prog);
    CHECK(a.xs == 6 && a.xn >= a.xu + 16 * 6 && a.tab >= a.xn + 16 * 3 && a.prog >= a.tab + 16 * 21);
    CHECK(a.xu >= make_ilqr_table_work(3, 2, cs).total && a.xu % 4 == 0 && a.prog % 2 == 0);
    const IlqrSindyLds c = make_ilqr_sindy_lds(3, 2, cs, 0, 0);
    CHECK(c.xu == a.xu && c.xn == a.xn && c.tab == a.tab && c.prog == c.tab);
    const IlqrSindyJacLds j = make_ilqr_sindy_jac_lds(17, 6);
    CHECK(j.v == 0 && j.g == 64 && j.gvar == 64 + 640 && j.cnt == j.gvar + 320 && j.J == j.cnt + 32);
    CHECK(j.total == (size_t)j.J + 17 * 23);
    CHECK(make_ilqr_sindy_jac_lds(62, 1).total * 8 <= kLimit);
  }
  // the staged program's size is sindy_prog_elems' (sindy_kernels.hpp) + 2 for T = double
  CHECK(ilqr_sindy_prog_elems(4, 55, 5, 0, 0, 0) == (size_t)(55 * 4 + 5) + (2 * 55 + 5 + 1) / 2 + 4);

  // ---- accepted batches and their reservation: the largest entry's need
  const IlqrSindyView plan3 = poly3trig2, plan17 = hc;
  size_t need = 0;
  CHECK(check(plan3, 35, {poly3trig2, cross3, cross5}, &need) == 0);
  CHECK(need == ilqr_sindy_table_lds_bytes(plan3, 35, cross3) && need > ilqr_sindy_table_lds_bytes(plan3, 35, cross5));
  CHECK(check(plan17, 700, {hc, hcx}, &need) == 0 && need == ilqr_sindy_table_lds_bytes(plan17, 700, hc));
  CHECK(need <= kLimit);

  // ---- refusals
  CHECK(refused(ilqr_sindy_table_check(plan3, 35, 0, 0, 0, nullptr, kLimit, nullptr), "NULL argument"));
  CHECK(refused(ilqr_sindy_table_check(plan3, 35, 0, 0, 2, nullptr, kLimit, nullptr), "NULL argument"));
  { const IlqrSindyView* two[2] = {&cross3, nullptr};
    CHECK(refused(ilqr_sindy_table_check(plan3, 35, 0, 0, 2, two, kLimit, nullptr), "NULL model handle")); }
  { IlqrSindyView p = plan3; p.f64 = 0; CHECK(refused(check(p, 35, {cross3}), "f64 only")); }
  { IlqrSindyView p = plan3; p.has_sindy = 0; CHECK(refused(check(p, 35, {cross3}), "plan handle's model is not a SINDy model")); }
  { IlqrSindyView p = plan3; p.obs_dim = 2; CHECK(refused(check(p, 35, {cross3}), "observation dimension must be the state dimension")); }
  CHECK(refused(check(plan3, 35, {cross3}, nullptr, 1, 0), "ampc_ilqr_plan_set_models"));
  CHECK(refused(check(plan3, 35, {cross3}, nullptr, 0, 2), "ampc_ilqr_plan_set_model_table"));
  { IlqrSindyView m = cross3; m.has_sindy = 0; CHECK(refused(check(plan3, 35, {poly3trig2, m}), "holds no SINDy model")); }
  { IlqrSindyView m = cross3; m.f64 = 0; CHECK(refused(check(plan3, 35, {m}), "device and precision")); }
  { IlqrSindyView m = cross3; m.device = 1; CHECK(refused(check(plan3, 35, {m}), "device and precision")); }
  CHECK(refused(check(plan3, 35, {cross3, c1}), "state and control dimensions"));
  { IlqrSindyView p = view(60, 4, 64, 0, 0, 0, 0); CHECK(refused(check(p, 100, {p}), "<= 63")); }
  // -3: the need against a smaller limit (inside the entry's limits no plan reaches 160 KB), and a plan that does
  need = 7;
  CHECK(refused(check(plan3, 35, {cross3}, &need, 0, 0, 4096), "more than 160 KB", kIlqrTableNoFit) && need == 7);
  CHECK(check(plan3, 35, {cross3}, &need, 0, 0, ilqr_sindy_table_lds_bytes(plan3, 35, cross3)) == 0);
  CHECK(refused(check(plan3, 35, {cross3}, &need, 0, 0, ilqr_sindy_table_lds_bytes(plan3, 35, cross3) - 8), "more than 160 KB",
                kIlqrTableNoFit));
  { const IlqrSindyView p = view(8, 2, 600, 70, 0, 0, 0);       // 141 table entries x 16 rows, a 43 KB program
    CHECK(p.stage == 1 && check(p, 20000, {p}, &need) == -3 && refused(-3, "more than 160 KB", kIlqrTableNoFit)); }

  std::printf("ilqr_sindy_table_hostcheck: %d checks passed\n", n_checks);
  return 0;
}
