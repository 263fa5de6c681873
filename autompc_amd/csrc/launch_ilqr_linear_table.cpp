// launch_ilqr_linear_table.cpp -- launchers of the kernels of ilqr_linear_table_kernels.hpp: the sweep and the line
// search / rollout of an iLQR plan that holds a table of linear models of mixed state dimension
// (ampc_ilqr_plan_set_linear_models), its queue refill and the three launches around the surrogate step of its closed
// loop.  f64 only: compiled once, and not part of a shape plugin.  The entry, its checks and the table are in
// api_ilqr.cpp.
#include "host_common.hpp"
#include "ilqr_linear_table_kernels.hpp"

static IlqrLinTab lin_tab_of(const ampc_ilqr_plan* p) {
  IlqrLinTab t;
  t.table = (const LinDev<double>*)p->lqt_tab.p;
  t.slot_model = (const int*)p->slot_model.p;
  t.nx_w = p->lqt_nxw; t.nxp_w = round_up(p->lqt_nxw, 16); t.ldj_w = round_up(p->lqt_nxw + p->h->nu, 16);
  t.lds_xn = p->lqt_lds_xn; t.lds_work = p->lqt_lds_work;
  return t;
}

// `args`: the iteration's IlqrArgs<double> (make_ilqr_args).  Enqueues on the plan's stream; e: the iteration's timing
// events or nullptr.
int ilqr_linear_table_launch_iter(ampc_ilqr_plan* p, const void* args, int mode, hipEvent_t* e) {
  const IlqrArgs<double>& a = *static_cast<const IlqrArgs<double>*>(args);
  ampc_handle* h = p->h;
  REQUIRE(p->lqt_n > 0 && p->lqt_tab.p && p->slot_model.p && p->queue_on,
          "internal: table iteration without a table of linear models, or outside a queue");
  REQUIRE(p->lqt_sweep_bytes <= kLdsLimit && p->lqt_ls_bytes <= kLdsLimit && p->lqt_nxw <= kLinMaxIlqrNx && a.ls_n <= 16,
          "internal: the plan's geometry is not the linear table kernels'");
  const IlqrLinTab t = lin_tab_of(p);
  const int Bg = p->B;                      // (workgroup b = slot b: no compaction on this path)
  if (mode == 1) {
    const size_t wb = p->lqt_sweep_bytes;
#define AMPC_LT_NU(NUV)                                                                                \
    case NUV: { auto rk = ilqr_riccati_wide_table_kernel<NUV>; HIP_OK(allow_lds(rk, wb));                \
      hipLaunchKernelGGL(rk, dim3(Bg), dim3(kRicThreads), wb, h->stream, a, t); } break;
    switch (h->nu) {
      AMPC_LT_NU(1) AMPC_LT_NU(2) AMPC_LT_NU(3) AMPC_LT_NU(4) AMPC_LT_NU(6) AMPC_LT_NU(8)
      default: return fail("internal: control dimension of a linear table iLQR plan");
    }
#undef AMPC_LT_NU
    HIP_OK(hipGetLastError());
  }
  if (e) HIP_OK(hipEventRecord(e[1], h->stream));
  HIP_OK(allow_lds(ilqr_iter_linear_table_kernel, p->lqt_ls_bytes));
  hipLaunchKernelGGL(ilqr_iter_linear_table_kernel, dim3(Bg), dim3(64 * kIltW), p->lqt_ls_bytes, h->stream, a, t);
  HIP_OK(hipGetLastError());
  if (e) HIP_OK(hipEventRecord(e[2], h->stream));
  return 0;
}

int ilqr_linear_table_refill(ampc_ilqr_plan* p, const void* args, const void* queue, const int* x_off) {
  const IlqrArgs<double>& a = *static_cast<const IlqrArgs<double>*>(args);
  const IlqrQueue<double>& q = *static_cast<const IlqrQueue<double>*>(queue);
  REQUIRE(p->lqt_n > 0 && q.model && q.slot_model && x_off && q.nx == p->lqt_nxw, "internal: refill without a table of linear models");
  hipLaunchKernelGGL(ilqr_linear_table_refill_kernel, dim3(p->B), dim3(256), 0, p->h->stream, a, q, lin_tab_of(p), x_off);
  HIP_OK(hipGetLastError());
  return 0;
}

// controller states <- rule(state, u_prev, sim[:obs_dim]) for n descriptors (linear_ctrl_state_kernel, unchanged)
int ilqr_linear_table_ctrl_state(ampc_ilqr_plan* p, int n, const void* descs, double* states, const double* sim, int snx,
                                 const double* u_prev) {
  ampc_handle* h = p->h;
  hipLaunchKernelGGL(linear_ctrl_state_kernel<double>, dim3(n), dim3(kLinCtrlThreads), 0, h->stream,
                     (const LinCtrlDesc*)descs, (const LinDev<double>*)p->lqt_tab.p, states, sim, snx, h->obs_dim, h->nu,
                     u_prev, (const double*)p->lqt_prog.p);
  HIP_OK(hipGetLastError());
  return 0;
}

size_t ilqr_linear_table_desc_bytes() { return sizeof(LinCtrlDesc); }
void ilqr_linear_table_desc_fill(void* dst, int i, int n, int rule, int n_basis, int model, int x_off, int lift_off) {
  static_cast<LinCtrlDesc*>(dst)[i] = LinCtrlDesc{n, rule, n_basis, model, x_off, lift_off};
}

int ilqr_linear_table_chain_pre(ampc_ilqr_plan* p, const void* args, const IlqrLinChains* chains) {
  const IlqrArgs<double>& a = *static_cast<const IlqrArgs<double>*>(args);
  const IlqrLinChains& q = *chains;
  hipLaunchKernelGGL(ilqr_linear_chain_pre_kernel, dim3(p->B), dim3(64), 0, p->h->stream, a, q, lin_tab_of(p));
  HIP_OK(hipGetLastError());
  return 0;
}

int ilqr_linear_table_chain_post(ampc_ilqr_plan* p, const void* args, const IlqrLinChains* chains) {
  const IlqrArgs<double>& a = *static_cast<const IlqrArgs<double>*>(args);
  const IlqrLinChains& q = *chains;
  hipLaunchKernelGGL(ilqr_linear_chain_post_kernel, dim3(p->B), dim3(256), 0, p->h->stream, a, q, lin_tab_of(p));
  HIP_OK(hipGetLastError());
  return 0;
}
