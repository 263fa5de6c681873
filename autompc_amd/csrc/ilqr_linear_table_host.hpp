// ilqr_linear_table_host.hpp -- what the kernels of ilqr_linear_table_kernels.hpp and the host code of
// ampc_ilqr_plan_set_linear_models / ampc_ilqr_closed_loop_linear (api_ilqr.cpp) share: the second kernel argument, the
// closed loop's bookkeeping record, the LDS maps and the launchers' declarations (launch_ilqr_linear_table.cpp).
#pragma once
#include "ilqr_kernels.hpp"
#include "ilqr_wide.hpp"
#include "linear_kernels.hpp"

struct ampc_ilqr_plan;

namespace ampc {

struct LinCtrlDesc;              // mppi_linear_table_kernels.hpp

// The second argument of the table kernels (IlqrArgs keeps its layout: the shape plugins read it).
struct IlqrLinTab {
  const LinDev<double>* table;   // [n_models]
  const int* slot_model;         // [B] entry of each slot's problem
  int nx_w, nxp_w, ldj_w;        // the widest entry's nx, nxp, ldj: strides of the per-slot regions
  int lds_xn, lds_work;          // line search: next-state scratch and work map (elements)
};

// LDS of the sweep for an entry of nx states (make_wide_lds is monotone in nx: the widest entry's is the launch's)
inline size_t ilqr_linear_table_sweep_bytes(int nx, int nu, int no) { return (size_t)make_wide_lds(nx, nu, no).total * 8; }

// Line search: [x | u] [16][xs], next states [16][nx], the compact work map -- placed for the WIDEST entry (nx); an
// entry uses its own row stride and its own work map inside.
inline size_t ilqr_linear_table_ls_map(int nx, int nu, int cost_stride, int* lds_xn, int* lds_work) {
  const int xs = lin_xs((nx + nu + 3) / 4 * 4, 8);
  const int xn = (16 * xs + 3) / 4 * 4, wk = (xn + 16 * nx + 3) / 4 * 4;
  if (lds_xn) *lds_xn = xn;
  if (lds_work) *lds_work = wk;
  return ((size_t)wk + make_ilqr_work(nx, nu, cost_stride, true).total) * 8;
}

// Bookkeeping of the closed loop: ilqr_kernels.hpp's IlqrChains with a surrogate state per slot and the per-entry rules.
struct IlqrLinChains {
  int C, B, H, nxw, nu, snx, n_steps, max_iter;
  const int* horizon; int* slot_h;
  const int* model; int* slot_model;                          // [C], [B]
  const int* rule; const int* n_basis; const int* lift_off;   // per table entry
  int* ctl; int* slot_chain; int* need; int* chain_t; int* chain_fail;
  long long* chain_iters;
  const double* x0; const int* x_off;     // ragged initial controller states, [C] offsets
  const double* sim0;                     // [C][snx] initial surrogate states
  const int* cost; int* cost_idx;
  double* sim; double* stage_u; double* stage_next;           // [B][snx], [B][nu], [B][snx]
  LinCtrlDesc* desc;                      // [B]
  double* traj_obs; double* traj_ctrls;   // [C][n_steps+1][snx], [C][n_steps+1][nu]
};

}  // namespace ampc

// launch_ilqr_linear_table.cpp (f64 only, not part of a shape plugin); everything enqueues on the plan's stream
int ilqr_linear_table_refill(ampc_ilqr_plan* p, const void* args, const void* queue, const int* x_off);
int ilqr_linear_table_ctrl_state(ampc_ilqr_plan* p, int n, const void* descs, double* states, const double* sim, int snx,
                                 const double* u_prev);
size_t ilqr_linear_table_desc_bytes();
void ilqr_linear_table_desc_fill(void* dst, int i, int n, int rule, int n_basis, int model, int x_off, int lift_off);
int ilqr_linear_table_chain_pre(ampc_ilqr_plan* p, const void* args, const ampc::IlqrLinChains* chains);
int ilqr_linear_table_chain_post(ampc_ilqr_plan* p, const void* args, const ampc::IlqrLinChains* chains);
