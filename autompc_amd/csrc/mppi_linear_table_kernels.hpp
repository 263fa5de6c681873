// mppi_linear_table_kernels.hpp -- the MPPI rollout of a plan whose problems run on DIFFERENT linear models
// x' = A x + B u of mixed state dimension (ARX histories, Koopman lifts) in ONE launch
// (ampc_mppi_plan_set_linear_models), and the per-problem controller-state rules of its closed loop
// (ampc_mppi_closed_loop_linear).
//
// linear_rollout_kernel (linear_kernels.hpp) receives its model as a by-value LinDev<T> kernel argument and reads the
// initial state at x0[p * nx].  Here a workgroup (16 samples x kLinW waves) finds its problem through args.tile_prob,
// the problem's MppiProblem::model names an entry of a device array of LinDev<T>, and the initial state sits at
// x_off[p] of a ragged x0 (problem b owns nx[model of b] values, in plan order).  x_off is a parallel array: the
// problem record and the argument block keep the layout the shape-specialised kernels read.
//
// LDS map (elements of T): the [x | u] ping-pong [2][16][xs] starts at 0 with the workgroup's OWN entry's row stride
// xs = lin_xs(kp); the plan-level regions (args.lds_cost, lds_aseq, lds_eps, lds_red) lie behind
// lin_lds_base(widest kp of the table).  No arithmetic depends on an offset, and everything else restates
// linear_rollout_kernel's statements in their order -- clipping, the TPS = 32 cost partials, lin_tile's k-order, the
// fused softmin tile part -- so a problem's results are the same bits alone, in any plan of the same horizon cap and
// update mode, at any position, and the bits of a single-model plan on linear_rollout_kernel
// (tests/test_gpu_mppi_linear_table.py compares bit for bit).
#pragma once
#include "linear_kernels.hpp"

namespace ampc {

template <typename T>
__global__ __launch_bounds__(64 * kLinW) void linear_table_rollout_kernel(const MppiArgs<T> args,
                                                                          const LinDev<T>* __restrict__ table,
                                                                          const int* __restrict__ x_off) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* lds = reinterpret_cast<T*>(smem_raw);
  constexpr int M = 16, NTHR = 64 * kLinW, TPS = NTHR / M;      // 32 threads per sample, one wave half each
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int tile = blockIdx.x;                                  // (the plan's longest-horizon-first order)
  const int p = args.tile_prob[tile];
  const MppiProblem<T> pr = args.probs[p];
  const LinDev<T> m = table[pr.model];
  const int nx = m.nx, nu = m.nu, no = args.obs_dim, xs = lin_xs(m.kp, (int)sizeof(T));
  const bool diag = args.cost_diag != 0, affine = args.cost_affine != 0;
  const int cost_stride = args.cost_stride;
  const int first = (tile - pr.tile0) * M;
  const int H = pr.H, N = pr.N;
  T* xb[2] = {lds, lds + 16 * xs};
  T* aseq = lds + args.lds_aseq;
  T* cpar = lds + args.lds_cost;
  const T* Qm = cpar; const T* Rm = Qm + no * no; const T* Fm = Rm + nu * nu; const T* goal = Fm + no * no;
  const T* lin = goal + no; const T* lint = lin + no;
  const T* blo = cpar + cost_stride; const T* bhi = blo + nu; const T* bsc = bhi + nu;

  for (int i = tid; i < 2 * 16 * xs; i += NTHR) lds[i] = T(0);
  for (int i = tid; i < cost_stride; i += NTHR) cpar[i] = args.costs_par[(size_t)pr.cost_idx * cost_stride + i];
  for (int i = tid; i < 3 * nu; i += NTHR) cpar[cost_stride + i] = args.bounds[i];
  for (int i = tid; i < H * nu; i += NTHR) {
    const int t = i / nu, j = i - t * nu;
    const int ts = (t + 1 < H) ? t + 1 : H - 1;                 // a[:-1] = a[1:]; a[-1] = a[-2]
    aseq[i] = args.act_in[pr.a_off + ts * nu + j];
  }
  const int ms = tid / TPS, r = tid % TPS;                      // sample in tile, helper index
  const int n = first + ms;
  const bool valid = n < N;
  const T* eps_row = args.eps + pr.eps_off + (size_t)(valid ? n : 0) * H * nu;
  T* epso = args.eps_out + pr.epso_off;
  const T* x0p = args.x0 + x_off[p];
  __syncthreads();
  for (int i = tid; i < M * nx; i += NTHR) {
    const int row = i / nx, col = i - row * nx;
    xb[0][row * xs + col] = x0p[col];
  }
  T c_part = T(0), ca_part = T(0);
  // actions of step t into buffer `dst`: A = clip(eps + a), eps <- A - a, u = A * scale (mppi.py:134-139)
  auto actions = [&](int t, T* dst) {
    if (r < nu) {
      const int j = r;
      const T a = aseq[t * nu + j];
      T A = (valid ? eps_row[t * nu + j] : T(0)) + a;
      A = A < blo[j] ? blo[j] : A;              // by comparison: a NaN poisons the sample as in the reference
      A = A > bhi[j] ? bhi[j] : A;
      const T ec = A - a;
      if (valid && args.write_eps_out) epso[((size_t)t * N + n) * nu + j] = ec;
      if (args.lds_eps >= 0) lds[args.lds_eps + (t * M + ms) * nu + j] = ec;
      ca_part += A * ec;
      const T u = A * bsc[j];
      dst[ms * xs + nx + j] = u;
      if (diag) c_part += Rm[j * nu + j] * u * u;
    }
  };
  actions(0, xb[0]);
  __syncthreads();
  if (affine && r == 0) c_part += T(H) * lint[no];
  for (int t = 0; t < H; ++t) {
    T* cur = xb[t & 1];
    T* nxt = xb[(t + 1) & 1];
    // ---- stage cost of (x_t, u_t): TPS partials per sample, reduced once after the loop
    c_part += quad_rows<T>(Qm, cur + ms * xs, goal, no, r, TPS, diag);
    if (args.n_ind) c_part += indicator_rows<T>(args.ind_tab, args.n_ind, cur + ms * xs, 1, no, r, TPS);
    if (!diag) c_part += quad_rows<T>(Rm, cur + ms * xs + nx, nullptr, nu, r, TPS, false);
    if (affine) c_part += affine_rows<T>(lin, cur + ms * xs, goal, no, r, TPS, T(0));
    // ---- dynamics: x_{t+1} = M [x_t ; u_t] into the other buffer; the next step's actions beside it
    for (int nt = w; nt < m.ntile; nt += kLinW) {
      const typename Acc<T>::type acc = lin_tile<T>(m, cur, xs, nt, lane);
      const int col = 16 * nt + (lane & 15);
#pragma unroll
      for (int rr = 0; rr < 4; ++rr)
        if (col < nx) nxt[acc_row<T>(lane >> 4, rr) * xs + col] = acc[rr];
    }
    if (t + 1 < H) actions(t + 1, nxt);
    lds_barrier();
  }
  // ---- epilogue: terminal cost, reduce the TPS partials, write ---------------------------------
  const T* xe = xb[H & 1] + ms * xs;
  T term = quad_rows<T>(Fm, xe, goal, no, r, TPS, diag);
  if (affine) term += affine_rows<T>(lint, xe, goal, no, r, TPS, lint[no + 1]);
  T c = c_part + pr.lam_over_sigma * ca_part;
  if (args.term_mode == 1) c += term;
#pragma unroll
  for (int off = TPS / 2; off > 0; off >>= 1) {
    c += __shfl_xor(c, off);
    term += __shfl_xor(term, off);
  }
  if (r == 0 && valid) {
    args.costs[pr.cost_off + n] = c;
    if (n == N - 1) args.term_last[p] = term;
  }
  if (args.lds_eps < 0) return;
  // ---- fused softmin update, tile part (as linear_rollout_kernel; mppi_combine_kernel finishes)
  T* cred = lds + args.lds_red;
  T* sred = cred + M;
  if (r == 0) cred[ms] = valid ? c : T(INFINITY);
  __syncthreads();
  T mw = cred[0];
  for (int i = 1; i < M; ++i) mw = cred[i] < mw ? cred[i] : mw;
  const bool dead_tile = !(mw < T(INFINITY));
  if (tid < M)
    sred[tid] = (first + tid < N && !dead_tile) ? exp(pr.neg_inv_lambda * (cred[tid] - mw)) : T(0);
  __syncthreads();
  const T* el = lds + args.lds_eps;
  T* tp = args.tile_part + (size_t)tile * args.hnu_stride;
  for (int e = tid; e < H * nu; e += NTHR) {
    const int t = e / nu, j = e - t * nu;
    T s = T(0);
    for (int i = 0; i < M; ++i) s += sred[i] * el[(t * M + i) * nu + j];
    tp[e] = s;
  }
  if (tid == 0) {
    T ss = T(0);
    for (int i = 0; i < M; ++i) ss += sred[i];
    args.tile_stat[2 * tile] = mw;
    args.tile_stat[2 * tile + 1] = ss;
  }
}

// One problem of the closed loop's controller-state update.
struct LinCtrlDesc {
  int n, rule, n_basis, model;   // rule 0: state = observation; 1: ARX shift A s + B u_prev, then the observation slot
                                 // overwritten (arx.py:94-99); 2: lift of the observation (koopman.py:105-122, 166-168)
  int x_off, lift_off;           // into the ragged state; into the lift programs ((kind, parameter) pairs)
};

constexpr int kLinCtrlThreads = 256;     // >= the widest state (256): one entry per thread

// state_b <- rule_b(state_b, u_prev_b, sim_b[:no]) of every problem (one workgroup each), in the plan's precision:
// lqr_ctrl_kernel's three rules (lqr_kernels.hpp).  sim [B][snx]: the surrogate state, whose first `no` entries are the
// observation simulate() hands the controller; u_prev [B][nu].  Rule 1 reads the PLAIN [A | B] rows of the entry.
template <typename T>
__global__ __launch_bounds__(kLinCtrlThreads) void linear_ctrl_state_kernel(const LinCtrlDesc* __restrict__ descs,
                                                                            const LinDev<T>* __restrict__ table,
                                                                            T* __restrict__ states,
                                                                            const T* __restrict__ sim, int snx, int no,
                                                                            int nu, const T* __restrict__ u_prev,
                                                                            const T* __restrict__ lprog) {
  __shared__ T s_old[kLinCtrlThreads];
  const int b = blockIdx.x, t = threadIdx.x;
  const LinCtrlDesc d = descs[b];
  const int n = d.n;
  T* st = states + d.x_off;
  const T* obs = sim + (size_t)b * snx;
  if (d.rule == 0) {
    for (int i = t; i < n; i += kLinCtrlThreads) st[i] = obs[i];
  } else if (d.rule == 1) {
    const T* __restrict__ ab = table[d.model].plain;
    const T* ub = u_prev + (size_t)b * nu;
    const int m = n + nu;
    for (int i = t; i < n; i += kLinCtrlThreads) s_old[i] = st[i];
    __syncthreads();
    for (int i = t; i < n; i += kLinCtrlThreads) {
      if (i < no) {
        st[i] = obs[i];
        continue;
      }
      const T* row = ab + (size_t)i * m;
      T a = T(0), c = T(0);
      for (int j = 0; j < n; ++j) a = fma(row[j], s_old[j], a);
      for (int r = 0; r < nu; ++r) c = fma(row[n + r], ub[r], c);
      st[i] = a + c;
    }
  } else {
    const T* prog = lprog + d.lift_off;
    for (int e = t; e < n; e += kLinCtrlThreads) {
      const int f = e / no, j = e - f * no;
      const T o = obs[j];
      const int kind = (int)prog[2 * f];
      const T par = prog[2 * f + 1];
      T v = o;
      if (kind == 1) {                     // o ** p rounded once (state_lift_kernel, mppi_kernels.hpp)
        const int pw = (int)par;
        double hi = pw >= 1 ? (double)o : 1.0, lo = 0.0;
        for (int k = 1; k < pw; ++k) {
          const double ph = hi * (double)o;
          const double pe = fma(hi, (double)o, -ph) + lo * (double)o;
          hi = ph + pe;
          lo = pe - (hi - ph);
        }
        v = (T)hi;
      } else if (kind == 2) {
        v = sin(par * o);
      } else if (kind == 3) {
        v = cos(par * o);
      }
      st[e] = v;
    }
  }
}

}  // namespace ampc
