// ilqr_table_host.hpp -- the host half of ampc_ilqr_plan_set_model_table that makes no device call (api_ilqr.cpp):
// the checks of the plan and of the model arguments, the packing of host-resident parameters (kstep_mlp_prepare) and
// the LDS map of the table iteration kernel (ilqr_table_kernels.hpp, which takes the map from here).  A stand-alone
// host program can run it (tools/ilqr_table_hostcheck.cpp).
#pragma once
#include <cstddef>
#include <string>

#include "kstep_mlp_host.hpp"

#ifdef __HIPCC__
#define AMPC_IT_HD __host__ __device__
#else
#define AMPC_IT_HD
#endif

extern thread_local std::string g_err;

// return codes of ampc_ilqr_plan_set_model_table besides 0 and -1 (callers decide by the code, not by the text)
constexpr int kIlqrTableNoFit = -3;        // the plan's LDS map for the table iteration kernel exceeds 160 KB

// The work region of ilqr_iter_table_kernel behind act / xu / norm, offsets in doubles: fixed by (nx, nu, cost
// stride), never by the models.
struct IlqrTableWork {
  int K, k, ubar, xbar, cpar, lo, hi, lsobj, scal, piv, total;
};
AMPC_IT_HD inline IlqrTableWork make_ilqr_table_work(int nx, int nu, int cost_stride) {
  IlqrTableWork w;
  int o = 0;
  w.K = o; o += nu * nx;
  w.k = o; o += nu;
  w.ubar = o; o += nu;
  w.xbar = o; o += nx;
  w.cpar = o; o += cost_stride;
  w.lo = o; o += nu;
  w.hi = o; o += nu;
  w.lsobj = o; o += 16;
  w.scal = o; o += 16;
  w.piv = o; o += 8;          // ints: selected row, failure, success
  w.total = o;
  return w;
}

// Bytes of the iteration kernel's LDS map: `base` doubles (act, xu, norm: ilqr_table_lds_base()) + the work region.
inline size_t ilqr_table_lds_bytes(int base, int nx, int nu, int cost_stride) {
  return ((size_t)base + (size_t)make_ilqr_table_work(nx, nu, cost_stride).total) * 8;
}

// What the checks read of a plan and its handle.
struct IlqrTablePlanView {
  int f64;              // the handle's precision is f64
  int has_mlp;          // the handle's model is an MLP (not SINDy, not a linear model)
  int nx, nu, obs_dim;  // the handle's dimensions
  int n_shape_models;   // handles held through ampc_ilqr_plan_set_models
  int cost_stride;
};

inline int ilqr_table_fail(const std::string& msg, int rc = -1) {
  g_err = "ampc_ilqr_plan_set_model_table: " + msg;
  return rc;
}

// 0, or a refusal with the message set.  lds_base: ilqr_table_lds_base(); lds_limit: bytes of LDS a workgroup may use.
inline int ilqr_table_check(const IlqrTablePlanView& v, int n_models, const int* n_hidden, const int* dims,
                            const int* activations, const double* const* weights, const double* const* biases,
                            const double* const* norms, const int* on_device, int lds_base, size_t lds_limit,
                            KstepMlpPrep* prep) {
  if (!v.f64) return ilqr_table_fail("the table kernels are f64 only; this plan's handle is f32");
  if (!v.has_mlp) return ilqr_table_fail("the plan handle's model is not an MLP");
  if (v.n_shape_models > 0)
    return ilqr_table_fail("the plan holds per-slot models of one shape (ampc_ilqr_plan_set_models); remove them first");
  if (n_models < 1) return ilqr_table_fail("NULL argument");
  if (v.nx + v.nu > 63) return ilqr_table_fail("state dim + ctrl dim must be <= 63 (the iLQR sweep's limit)");
  if (int rc = kstep_mlp_prepare(n_models, n_hidden, dims, activations, weights, biases, norms, on_device, v.nx, v.nu,
                                 v.obs_dim, prep)) {
    g_err = "ampc_ilqr_plan_set_model_table: the models must have the plan handle's state and control dimensions, "
            "within the limits of ampc_kstep_errors_mlp -- " + g_err;
    return rc;
  }
  if (ilqr_table_lds_bytes(lds_base, v.nx, v.nu, v.cost_stride) > lds_limit)
    return ilqr_table_fail("states / controls / cost block of this plan need more than 160 KB of LDS in the table "
                           "iteration kernel", kIlqrTableNoFit);
  return 0;
}

// Widest hidden layer (rounded up to the 16-column tile) and most hidden layers of the table: the size of the stored
// activation derivatives [hidden layers][slots * padded horizon][width].
inline void ilqr_table_extent(int n_models, const int* n_hidden, const int* dims, int max_layers, int* width, int* hidden) {
  int wmax = 16, hmax = 1;
  for (int k = 0; k < n_models; ++k) {
    if (n_hidden[k] > hmax) hmax = n_hidden[k];
    for (int l = 1; l <= n_hidden[k]; ++l) {
      const int d = dims[(size_t)k * (max_layers + 1) + l];
      if ((d + 15) / 16 * 16 > wmax) wmax = (d + 15) / 16 * 16;
    }
  }
  *width = wmax;
  *hidden = hmax;
}
