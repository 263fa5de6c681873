// mppi_program_kernels.hpp -- MPPI rollout on an analytic dynamics program (program_kernels.hpp): the controller that
// plans on the true dynamics.  A handle is such a controller model once ampc_set_program_jvp has staged the program's
// JVP beside it (api_program.cpp); the rollout itself runs the program, not the JVP.
//
// One sample per lane, one wave per workgroup, the plan's 64-sample tiles -- the layout and the semantics of
// mppi_rollout_sindy_kernel (sindy_kernels.hpp; mppi.py:120-152): the same MppiArgs, cost block, bounds, clipping,
// eps_out, lam_over_sigma, term_mode and term_last, and mppi_update_kernel finishes the solve.  The cost arithmetic is
// written as that kernel writes it; contraction is off inside the interpreter only (program_run).
//
// LDS: [n_slots][64] value slots, [nx][64] hand-over rows, then the shared cost block and the bounds.
//
// What differs from the SINDy kernel: the slot allocator reuses the input slots, so [x | u] are dead after
// program_run -- a step's stage cost and control cost are formed BEFORE the step, the controls are stored again every
// step, and the outputs pass through the hand-over rows before they become the next inputs (an output may be an input
// slot, or the outputs a permutation of the inputs).  The ProgDev arrives by value and every index into code, consts
// and out_slot is wave-uniform: the instruction stream keeps arriving through scalar loads and the opcode switch stays
// a scalar branch.  IND: the handle's cost has indicator terms (a separate instantiation, as the lane-spread SINDy
// kernel's).
#pragma once
#include <hip/hip_runtime.h>

#include "mppi_kernels.hpp"
#include "program_kernels.hpp"

namespace ampc {

template <typename T, bool IND>
__global__ __launch_bounds__(kProgLanes) void mppi_rollout_program_kernel(const MppiArgs<T> args, const ProgDev<T> pg) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* lds = reinterpret_cast<T*>(smem_raw);
  constexpr int BS = kProgLanes;
  const int lane = threadIdx.x, nx = pg.nx, nu = pg.nu, no = args.obs_dim;
  const int p = args.tile_prob[blockIdx.x];
  const MppiProblem<T> pr = args.probs[p];
  const int n = (blockIdx.x - pr.tile0) * BS + lane;
  const int H = pr.H, N = pr.N;
  const bool valid = n < N;
  T* v = lds + lane;                                   // [n_slots][BS]  x | u | the program's values
  T* hand = lds + (size_t)pg.n_slots * BS + lane;      // [nx][BS]       a step's outputs on their way to the inputs
  T* cpar = lds + (size_t)(pg.n_slots + nx) * BS;      // Q R F goal | lo hi scale (shared)
  for (int i = lane; i < args.cost_stride; i += BS)
    cpar[i] = args.costs_par[(size_t)pr.cost_idx * args.cost_stride + i];
  for (int i = lane; i < 3 * nu; i += BS) cpar[args.cost_stride + i] = args.bounds[i];
  __syncthreads();
  const T* Qm = cpar; const T* Rm = Qm + no * no; const T* Fm = Rm + nu * nu;
  const T* goal = Fm + no * no;
  const T* lin = goal + no; const T* lint = lin + no;       // affine part (all zero for one QuadCost)
  const T* blo = cpar + args.cost_stride; const T* bhi = blo + nu; const T* bsc = bhi + nu;
  for (int i = 0; i < nx; ++i) v[i * BS] = args.x0[p * nx + i];
  const T* eps_row = args.eps + pr.eps_off + (size_t)(valid ? n : 0) * H * nu;
  T* epso = args.eps_out + pr.epso_off;
  T c = T(0), ca = T(0);
  for (int t = 0; t < H; ++t) {
    const int ts = (t + 1 < H) ? t + 1 : H - 1;               // a[:-1] = a[1:]; a[-1] = a[-2]
    for (int j = 0; j < nu; ++j) {
      const T a = args.act_in[pr.a_off + ts * nu + j];
      T A = (valid ? eps_row[t * nu + j] : T(0)) + a;
      A = A < blo[j] ? blo[j] : A;
      A = A > bhi[j] ? bhi[j] : A;
      const T ec = A - a;
      if (valid) epso[((size_t)t * N + n) * nu + j] = ec;
      ca += A * ec;
      v[(nx + j) * BS] = A * bsc[j];
    }
    for (int i = 0; i < no; ++i) {
      T s = T(0);
      for (int j = 0; j < no; ++j) s += Qm[i * no + j] * (v[j * BS] - goal[j]);
      c += (v[i * BS] - goal[i]) * (s + lin[i]);
    }
    c += lint[no];
    if constexpr (IND) c += indicator_all<T>(args.ind_tab, args.n_ind, v, BS, no);
    for (int i = 0; i < nu; ++i) {
      T s = T(0);
      for (int j = 0; j < nu; ++j) s += Rm[i * nu + j] * v[(nx + j) * BS];
      c += v[(nx + i) * BS] * s;
    }
    program_run<T>(pg, v);                                    // (x | u are dead from here on)
    for (int i = 0; i < nx; ++i) hand[i * BS] = v[pg.out_slot[i] * BS];
    for (int i = 0; i < nx; ++i) v[i * BS] = hand[i * BS];
  }
  T term = T(0);
  for (int i = 0; i < no; ++i) {
    T s = T(0);
    for (int j = 0; j < no; ++j) s += Fm[i * no + j] * (v[j * BS] - goal[j]);
    term += (v[i * BS] - goal[i]) * (s + lint[i]);
  }
  term += lint[no + 1];
  c += pr.lam_over_sigma * ca;
  if (args.term_mode == 1) c += term;
  if (valid) {
    args.costs[pr.cost_off + n] = c;
    if (n == N - 1) args.term_last[p] = term;
  }
}

}  // namespace ampc
