// launch_ilqr_table.cpp -- launchers of the three kernels of ilqr_table_kernels.hpp: the line search / rollout, the
// forward pass and the Jacobian chain of an iLQR plan that holds a table of MLP models of mixed shapes
// (ampc_ilqr_plan_set_model_table).  f64 only: compiled once, and not part of a shape plugin.  The entry, its checks
// and the table are in api_ilqr.cpp / ilqr_table_host.hpp; the sweep stays launch_ilqr.cpp's.
#include "host_common.hpp"
#include "ilqr_table_kernels.hpp"

// doubles of LDS in front of the iteration kernel's work region (act, xu, norm)
int ilqr_table_lds_base() { return kItOffWork; }

// `args`: the iteration's IlqrArgs<double> (make_ilqr_args).  Enqueues on the plan's stream.
int ilqr_table_launch_iter(ampc_ilqr_plan* p, const void* args) {
  const IlqrArgs<double>& a = *static_cast<const IlqrArgs<double>*>(args);
  ampc_handle* h = p->h;
  REQUIRE(p->table_n > 0 && p->table_models.p, "internal: table iteration without a model table");
  const size_t lb = ilqr_table_lds_bytes(kItOffWork, h->nx, h->nu, h->cost_stride);
  REQUIRE(lb <= kLdsLimit && h->nx + h->nu <= 63 && h->nx <= kKmMaxOut && h->nu <= kKmMaxCtrl && a.ls_n <= kItRows,
          "internal: the plan's geometry is not the table kernel's");
  HIP_OK(allow_lds(ilqr_iter_table_kernel, lb));
  hipLaunchKernelGGL(ilqr_iter_table_kernel, dim3(ilqr_grid_slots(p)), dim3(kItThreads), lb, h->stream,
                     (const KstepMlpModel*)p->table_models.p, a);
  HIP_OK(hipGetLastError());
  return 0;
}

// Jacobians of every (slot, t) row of the nominal trajectories whose slot asked for it: forward pass, then the chain.
int ilqr_table_refresh(ampc_ilqr_plan* p) {
  ampc_handle* h = p->h;
  REQUIRE(p->table_n > 0 && p->table_models.p, "internal: table refresh without a model table");
  const int Bg = ilqr_grid_slots(p);
  IlqrTableRows r;
  std::memset(&r, 0, sizeof(r));
  r.states = (const double*)p->states.p; r.ctrls = (const double*)p->ctrls.p;
  r.dz = (double*)p->table_dz.p; r.jx = (double*)p->jx.p; r.ju = (double*)p->ju.p;
  r.refresh = (const int*)p->flags.p + 4 * p->B;
  r.slot_h = (p->queue_on && p->var_h) ? (const int*)p->slot_h.p : nullptr;
  r.slot_model = (p->queue_on && p->var_model) ? (const int*)p->slot_model.p : nullptr;
  r.slot_of = (p->queue_on && p->compact_on) ? (const int*)p->slot_of.p : nullptr;
  r.B = p->B; r.H = p->H; r.gpad = round_up(p->H, kItRows); r.nx = h->nx; r.nu = h->nu; r.wmax = p->table_wmax;
  REQUIRE((size_t)p->table_hidden * p->B * r.gpad * r.wmax * 8 <= p->table_dz.bytes,
          "internal: the stored derivatives do not fit the plan's buffer");
  HIP_OK(allow_lds(ilqr_fwd_table_kernel, kItRowsLdsBytes));
  HIP_OK(allow_lds(ilqr_jac_table_kernel, kItRowsLdsBytes));
  r.tiles = r.gpad / kItRows;
  hipLaunchKernelGGL(ilqr_fwd_table_kernel, dim3(Bg * r.tiles), dim3(kItThreads), kItRowsLdsBytes, h->stream,
                     (const KstepMlpModel*)p->table_models.p, r);
  HIP_OK(hipGetLastError());
  if (p->ev_cur) HIP_OK(hipEventRecord(p->ev_cur[3], h->stream));
  r.tiles = (p->H * (h->nx + h->nu) + kItRows - 1) / kItRows;
  hipLaunchKernelGGL(ilqr_jac_table_kernel, dim3(Bg * r.tiles), dim3(kItThreads), kItRowsLdsBytes, h->stream,
                     (const KstepMlpModel*)p->table_models.p, r);
  HIP_OK(hipGetLastError());
  if (p->ev_cur) HIP_OK(hipEventRecord(p->ev_cur[4], h->stream));
  return 0;
}
