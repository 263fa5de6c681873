// launch_mppi_table.cpp -- launcher of mppi_rollout_table_kernel (mppi_table_kernels.hpp): the rollout of an MPPI plan
// that holds a table of MLP models of mixed shapes (ampc_mppi_plan_set_model_table).  f64 only: compiled once, and
// not part of a shape plugin.  The entry, its checks and the table are in api_mppi.cpp / mppi_table_host.hpp.
#include "host_common.hpp"
#include "mppi_table_kernels.hpp"

// doubles of LDS in front of the plan's own regions (cost block, shifted sequence, clipped noise)
int mppi_table_lds_base() { return kMtOffExtra; }

// `args`: the solve's MppiArgs<double> (make_args).  Enqueues on the plan's stream.
int mppi_table_launch(ampc_mppi_plan* p, const void* args) {
  const MppiArgs<double>& a = *static_cast<const MppiArgs<double>*>(args);
  REQUIRE(p->table_n > 0 && p->table_models.p, "internal: table rollout without a model table");
  REQUIRE(p->tile_m == kMtRows && p->lds_bytes <= kLdsLimit && (int)(p->lds_bytes / 8) >= a.lds_aseq + p->max_h * p->h->nu &&
              a.lds_cost == kMtOffExtra,
          "internal: the plan's geometry is not the table kernel's");
  HIP_OK(allow_lds(mppi_rollout_table_kernel, p->lds_bytes));
  hipLaunchKernelGGL(mppi_rollout_table_kernel, dim3(p->n_tiles), dim3(kMtThreads), p->lds_bytes, p->h->stream,
                     (const KstepMlpModel*)p->table_models.p, a);
  return 0;
}
