// ilqr_sindy_table_host.hpp -- the host half of ampc_ilqr_plan_set_sindy_models that makes no device call
// (api_ilqr.cpp): the checks of the plan and of the model handles, the selection rule between the two bodies of
// ilqr_iter_sindy_table_kernel and the LDS maps of both kernels of ilqr_sindy_table_kernels.hpp, which take them from
// here.  A stand-alone host program can run it (tools/ilqr_sindy_table_hostcheck.cpp).
#pragma once
#include <cstddef>
#include <string>

#include "ilqr_table_host.hpp"       // make_ilqr_table_work: the work region fixed by (nx, nu, cost stride)

// What the checks, the selection rule and the maps read of a handle that holds a SINDy model.
struct IlqrSindyView {
  int f64;               // the handle's precision is f64
  int has_sindy;         // it holds a SINDy model (ampc_set_sindy)
  int device;
  int nx, nu, obs_dim;
  int n_feat, n_trig, n_pow, n_mon, n_pool, n_tab;
  int stage;             // the kernels copy the program to LDS (SindyDev::stage: a product table, <= 48 KB)
};

constexpr int kIsRows = 16;                  // line-search rows of a workgroup
constexpr int kIsLanes = 16;                 // lanes per row
constexpr int kIsJacThreads = 64;            // the Jacobian kernel: one wave per (slot, t) row
constexpr int kIsJacPairs = 10;              // partial derivatives a feature can have (ampc_set_sindy: <= 10 pairs)

// Doubles of the staged program of an entry (sindy_kernels.hpp: sindy_prog_elems for T = double, + 2 of slack).
AMPC_IT_HD inline size_t ilqr_sindy_prog_elems(int nx, int n_feat, int n_trig, int n_pow, int n_mon, int n_pool) {
  const size_t flt = (size_t)n_feat * nx + n_trig + n_pow;
  const size_t ints = (size_t)2 * n_feat + n_trig + n_pow + 2 * (size_t)n_mon + 2 * (size_t)n_pool;
  return flt + (ints * sizeof(int) + 7) / 8 + 2 + 2;
}

// The selection rule: a function of the entry alone (the plan's constants do not enter: both bodies use one map).
AMPC_IT_HD inline bool ilqr_sindy_table_spread(int n_tab, int nx, int stage) { return n_tab > 0 && nx <= 8 && stage != 0; }

// LDS map of ilqr_iter_sindy_table_kernel, offsets in doubles.  work / xu follow the plan's constants, xn / tab / prog
// the workgroup's own entry (n_tab); nothing follows another entry of the table.
struct IlqrSindyLds {
  int work, xu, xs, xn, tab, prog;
  size_t total;          // doubles, the staged program included when the entry is staged
};
AMPC_IT_HD inline IlqrSindyLds make_ilqr_sindy_lds(int nx, int nu, int cost_stride, int n_tab, size_t prog_elems) {
  IlqrSindyLds L;
  int o = 0;
  L.work = o; o += (make_ilqr_table_work(nx, nu, cost_stride).total + 3) / 4 * 4;
  L.xs = nx + nu + 1;
  L.xu = o; o += (kIsRows * L.xs + 3) / 4 * 4;
  L.xn = o; o += (kIsRows * nx + 3) / 4 * 4;
  L.tab = o; o += (kIsRows * n_tab + 3) / 4 * 4;
  L.prog = o;
  L.total = (size_t)o + prog_elems;
  return L;
}
inline size_t ilqr_sindy_table_lds_bytes(const IlqrSindyView& plan, int cost_stride, const IlqrSindyView& m) {
  const size_t prog = m.stage ? ilqr_sindy_prog_elems(m.nx, m.n_feat, m.n_trig, m.n_pow, m.n_mon, m.n_pool) : 0;
  return make_ilqr_sindy_lds(plan.nx, plan.nu, cost_stride, m.n_tab, prog).total * 8;
}

// LDS map of ilqr_jac_sindy_table_kernel (doubles), fixed by the plan's nx / nu:
//   v [64] | partials [64][10] | their variables [64][10] ints | counts [64] ints | J [nx][nx + nu]
struct IlqrSindyJacLds {
  int v, g, gvar, cnt, J;
  size_t total;
};
AMPC_IT_HD inline IlqrSindyJacLds make_ilqr_sindy_jac_lds(int nx, int nu) {
  IlqrSindyJacLds L;
  int o = 0;
  L.v = o; o += 64;
  L.g = o; o += kIsJacThreads * kIsJacPairs;
  L.gvar = o; o += kIsJacThreads * kIsJacPairs / 2;
  L.cnt = o; o += kIsJacThreads / 2;
  L.J = o;
  L.total = (size_t)o + (size_t)nx * (nx + nu);
  return L;
}

inline int ilqr_sindy_table_fail(const std::string& msg, int rc = -1) {
  g_err = "ampc_ilqr_plan_set_sindy_models: " + msg;
  return rc;
}

// 0, or a refusal with the message set.  n_shape_models / n_table: what the plan holds through
// ampc_ilqr_plan_set_models / ampc_ilqr_plan_set_model_table.  *lds_bytes: the largest entry's need (the launch's
// reservation).
inline int ilqr_sindy_table_check(const IlqrSindyView& plan, int cost_stride, int n_shape_models, int n_table, int n_models,
                                  const IlqrSindyView* const* models, size_t lds_limit, size_t* lds_bytes) {
  if (n_models < 1 || !models) return ilqr_sindy_table_fail("NULL argument");
  if (!plan.f64) return ilqr_sindy_table_fail("the table kernels are f64 only; this plan's handle is f32");
  if (!plan.has_sindy) return ilqr_sindy_table_fail("the plan handle's model is not a SINDy model (ampc_set_sindy)");
  if (plan.obs_dim != plan.nx)
    return ilqr_sindy_table_fail("the observation dimension must be the state dimension (a SINDy model's state is the "
                                 "observation)");
  if (n_shape_models > 0)
    return ilqr_sindy_table_fail("the plan holds per-slot models of one shape (ampc_ilqr_plan_set_models); remove them first");
  if (n_table > 0)
    return ilqr_sindy_table_fail("the plan holds a table of MLP models (ampc_ilqr_plan_set_model_table); remove it first");
  if (plan.nx + plan.nu > 63) return ilqr_sindy_table_fail("state dim + ctrl dim must be <= 63 (the iLQR sweep's limit)");
  size_t need = 0;
  for (int i = 0; i < n_models; ++i) {
    const IlqrSindyView* m = models[i];
    if (!m) return ilqr_sindy_table_fail("NULL model handle");
    if (!m->has_sindy) return ilqr_sindy_table_fail("a model handle holds no SINDy model (ampc_set_sindy)");
    if (m->device != plan.device || m->f64 != plan.f64)
      return ilqr_sindy_table_fail("models must share the plan's device and precision");
    if (m->nx != plan.nx || m->nu != plan.nu)
      return ilqr_sindy_table_fail("models must have the plan handle's state and control dimensions");
    const size_t b = ilqr_sindy_table_lds_bytes(plan, cost_stride, *m);
    if (b > need) need = b;
  }
  if (need > lds_limit || make_ilqr_sindy_jac_lds(plan.nx, plan.nu).total * 8 > lds_limit)
    return ilqr_sindy_table_fail("a model's table columns (16 rows), the plan's states / controls / cost block and the "
                                 "staged program need more than 160 KB of LDS", kIlqrTableNoFit);
  if (lds_bytes) *lds_bytes = need;
  return 0;
}
