// mppi_table_host.hpp -- the host half of ampc_mppi_plan_set_model_table that makes no device call (api_mppi.cpp):
// the checks of the plan and of the model arguments, the packing of host-resident parameters (kstep_mlp_prepare) and
// the size of the table kernel's LDS map.  A stand-alone host program can run it (tools/mppi_table_hostcheck.cpp).
#pragma once
#include <cstddef>
#include <string>

#include "kstep_mlp_host.hpp"

extern thread_local std::string g_err;

// return codes of ampc_mppi_plan_set_model_table besides 0 and -1 (callers decide by the code, not by the text)
constexpr int kMppiTableNoFit = -3;        // the plan's LDS map for the table kernel exceeds 160 KB

// What the checks read of a plan and its handle.
struct MppiTablePlanView {
  int f64;              // the handle's precision is f64
  int has_mlp;          // the handle's model is an MLP
  int nx, nu, obs_dim;  // the handle's dimensions
  int n_ind;            // indicator cost terms on the handle
  int lift_n;           // basis functions of a state lift on the plan
  int n_shape_models;   // handles held through ampc_mppi_plan_set_models
  int B, max_h, cost_stride;
};

// Bytes of the table kernel's LDS map: `base` doubles (act, xu, norm), cost block + bounds, the shifted sequence and
// -- fused -- the tile's clipped noise [max_h][16][nu] with 32 reduction slots.
inline size_t mppi_table_lds_bytes(int base, int cost_stride, int nu, int max_h, bool fused) {
  const size_t aseq = ((size_t)base + cost_stride + 3 * nu + 3) / 4 * 4;
  if (!fused) return (aseq + (size_t)max_h * nu) * 8;
  const size_t e0 = (aseq + (size_t)max_h * nu + 3) / 4 * 4;
  return (e0 + (size_t)max_h * 16 * nu + 32) * 8;
}

inline int mppi_table_fail(const std::string& msg, int rc = -1) {
  g_err = "ampc_mppi_plan_set_model_table: " + msg;
  return rc;
}

// 0, or a refusal with the message set.  lds_base: mppi_table_lds_base(); lds_limit: bytes of LDS a workgroup may use.
inline int mppi_table_check(const MppiTablePlanView& v, int n_models, const int* n_hidden, const int* dims,
                            const int* activations, const double* const* weights, const double* const* biases,
                            const double* const* norms, const int* on_device, const int* model_index, int lds_base,
                            size_t lds_limit, KstepMlpPrep* prep) {
  if (!v.f64) return mppi_table_fail("the table kernel is f64 only; this plan's handle is f32");
  if (!v.has_mlp) return mppi_table_fail("the plan handle's model is not an MLP");
  if (v.n_ind > 0) return mppi_table_fail("the plan's handle has indicator cost terms; the table kernel takes quadratic cost blocks only");
  if (v.lift_n > 0) return mppi_table_fail("the plan has a state lift; the table kernel rolls out on the observation");
  if (v.n_shape_models > 0)
    return mppi_table_fail("the plan holds per-problem models of one shape (ampc_mppi_plan_set_models); remove them first");
  if (n_models < 1 || !model_index) return mppi_table_fail("NULL argument");
  if (int rc = kstep_mlp_prepare(n_models, n_hidden, dims, activations, weights, biases, norms, on_device, v.nx, v.nu,
                                 v.obs_dim, prep)) {
    g_err = "ampc_mppi_plan_set_model_table: the models must have the plan handle's state and control dimensions, "
            "within the limits of ampc_kstep_errors_mlp -- " + g_err;
    return rc;
  }
  for (int b = 0; b < v.B; ++b)
    if (model_index[b] < 0 || model_index[b] >= n_models) return mppi_table_fail("model_index out of range");
  if (mppi_table_lds_bytes(lds_base, v.cost_stride, v.nu, v.max_h, false) > lds_limit)
    return mppi_table_fail("states / controls / horizon cap / cost block of this plan need more than 160 KB of LDS in "
                           "the table kernel", kMppiTableNoFit);
  return 0;
}
