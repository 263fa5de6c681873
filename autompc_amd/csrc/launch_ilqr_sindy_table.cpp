// launch_ilqr_sindy_table.cpp -- launchers of the two kernels of ilqr_sindy_table_kernels.hpp: the line search / rollout
// and the Jacobians of an iLQR plan that holds a table of SINDy models (ampc_ilqr_plan_set_sindy_models).  f64 only:
// compiled once, and not part of a shape plugin.  The entry, its checks and the table are in api_ilqr.cpp /
// ilqr_sindy_table_host.hpp; the sweep stays launch_ilqr.cpp's.
#include "host_common.hpp"
#include "ilqr_sindy_table_kernels.hpp"

// `args`: the iteration's IlqrArgs<double> (make_ilqr_args).  Enqueues on the plan's stream.
int ilqr_sindy_table_launch_iter(ampc_ilqr_plan* p, const void* args) {
  const IlqrArgs<double>& a = *static_cast<const IlqrArgs<double>*>(args);
  ampc_handle* h = p->h;
  REQUIRE(p->sindy_n > 0 && p->sindy_tab.p && p->sindy_lds > 0, "internal: table iteration without a table of SINDy models");
  REQUIRE(p->sindy_lds <= kLdsLimit && h->has_sindy && h->nx + h->nu <= 63 && a.ls_n <= kIsRows,
          "internal: the plan's geometry is not the SINDy table kernel's");
  HIP_OK(allow_lds(ilqr_iter_sindy_table_kernel, p->sindy_lds));
  hipLaunchKernelGGL(ilqr_iter_sindy_table_kernel, dim3(ilqr_grid_slots(p)), dim3(kIsRows * kIsLanes), p->sindy_lds,
                     h->stream, (const SindyDev<double>*)p->sindy_tab.p, a);
  HIP_OK(hipGetLastError());
  return 0;
}

// Jacobians of every (slot, t) row of the nominal trajectories whose slot asked for it: one wave per row.
int ilqr_sindy_table_refresh(ampc_ilqr_plan* p) {
  ampc_handle* h = p->h;
  REQUIRE(p->sindy_n > 0 && p->sindy_tab.p, "internal: table refresh without a table of SINDy models");
  IlqrSindyRows r;
  std::memset(&r, 0, sizeof(r));
  r.states = (const double*)p->states.p; r.ctrls = (const double*)p->ctrls.p;
  r.jx = (double*)p->jx.p; r.ju = (double*)p->ju.p;
  r.refresh = (const int*)p->flags.p + 4 * p->B;
  r.slot_h = (p->queue_on && p->var_h) ? (const int*)p->slot_h.p : nullptr;
  r.slot_model = (p->queue_on && p->var_model) ? (const int*)p->slot_model.p : nullptr;
  r.slot_of = (p->queue_on && p->compact_on) ? (const int*)p->slot_of.p : nullptr;
  r.B = p->B; r.H = p->H; r.nx = h->nx; r.nu = h->nu;
  const size_t lb = make_ilqr_sindy_jac_lds(h->nx, h->nu).total * 8;
  REQUIRE(lb <= kLdsLimit && h->nx + h->nu <= 63, "internal: the plan's geometry is not the SINDy table kernel's");
  HIP_OK(allow_lds(ilqr_jac_sindy_table_kernel, lb));
  hipLaunchKernelGGL(ilqr_jac_sindy_table_kernel, dim3(ilqr_grid_slots(p) * p->H), dim3(kIsJacThreads), lb, h->stream,
                     (const SindyDev<double>*)p->sindy_tab.p, r);
  HIP_OK(hipGetLastError());
  if (p->ev_cur) { HIP_OK(hipEventRecord(p->ev_cur[3], h->stream)); HIP_OK(hipEventRecord(p->ev_cur[4], h->stream)); }
  return 0;
}
