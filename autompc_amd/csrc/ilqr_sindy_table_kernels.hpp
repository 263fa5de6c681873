// ilqr_sindy_table_kernels.hpp -- the model-touching half of an iLQR iteration for a plan whose slots run on DIFFERENT
// SINDy models: any mix of feature libraries, coefficients and time modes (ampc_ilqr_plan_set_sindy_models; gfx950, f64
// only).  An iteration keeps its launches: sweep | line search | Jacobians.  The sweep is the plan's run-time-shape
// sweep (ilqr_kernels.hpp: it reads Jacobians from memory and depends on nx / nu only); the other two are here.  A
// slot's model is table[slot_model[slot]] (entry 0 without per-slot models), an entry of a device array of
// SindyDev<double> whose pointers lead into the models' own handles (as mppi_sindy_table_kernels.hpp reads them).
//
// ilqr_iter_sindy_table_kernel   one workgroup of 256 threads per slot; the contract of ilqr_iter_kernel<.., DYN = 1>
//     (ilqr_kernels.hpp) statement for statement: mode 0 rolls out the guess (one row; states, obj, active / refresh),
//     mode 1 the line search -- the ls_n <= 16 step sizes are the rows, thread (m = tid / 16, r = tid % 16) is lane r of
//     row m, u = alpha k_t + ubar_t + K_t (x - xbar_t) clipped when bounded, ls_states / ls_ctrls for rows < ls_n, the
//     objective dt (stage costs) + terminal cost through quad_rows / affine_rows -- then acceptance, the ||du|| test,
//     the swap and the flags.  slot_mode, slot_h (stride H), slot_of, the early returns of retired slots and of the
//     singular-sweep flag ric[3] as there; K_t, k_t, ubar_t, xbar_t reach LDS one step ahead through registers.
//     Only the dynamics step differs, in two bodies picked per ENTRY by ilqr_sindy_table_spread() -- a function of the
//     entry alone, never of the batch, shared with the host (ilqr_sindy_table_host.hpp):
//       lane-spread   entries with a product table, at most eight states and a program staged in LDS (sindy_stage<T,
//                     true>: every program pointer derives from LDS).  The sixteen lanes of row m fill the table
//                     entries j = r, r + 16, .., then form the features k = r, r + 16, .. and their nx coefficient
//                     products, and a DPP sum over the row (sindy_group_sum<16>) leaves the next state in every lane.
//       one-thread    everything else -- direct evaluation (n_tab == 0), more than eight states, programs over 48 KB
//                     read from global memory: sindy_step on lane r == 0 of the row, the program staged where the
//                     entry allows.
//     LDS (doubles; IlqrSindyLds): work region K, k, ubar, xbar, cost block, lo, hi, lsobj, scal, piv | xu [16][nx + nu
//     + 1] | next x [16][nx] | table [16][n_tab] | staged program.  Every offset follows the workgroup's OWN entry and
//     the plan's constants; only the reserved byte count follows the largest entry.
// ilqr_jac_sindy_table_kernel    Jacobians of the rows (slot, t < the slot's horizon) of the slots with refresh != 0
//     into the plan's jx / ju in the layout sindy_jacobian_kernel writes and the sweeps read ([slot * H + t][i][c]).
//     One wave per row -- a workgroup serves one row of one slot, hence one model (the per-slot grouping of RowMap with
//     a tile height of one row: no padding).  Features go through in chunks of 64, two phases per chunk:
//       one   lane f forms the partial derivatives of feature 64 chunk + f -- one or two (interaction terms), for a
//             monomial one per (variable, exponent) pair -- into LDS with the variable each belongs to;
//       two   lane e owns the entries J[i][c], i nx + c = e, e + 64, ..: it walks the chunk's features in ascending
//             order, a feature's first variable before its second, and adds xi[i][k] g for the partials of variable c
//             to the LDS-resident entry through a register.
//     That is sindy_jacobian_kernel's order per entry (its sums start from zero too), so the two kernels' Jacobians are
//     comparable entry by entry.  strict, monomials and continuous (I + dt J, dt Ju) as there.  Nothing accumulates in
//     global memory.
//
// No scratch, no atomics, and no index depends on a state value: a NaN poisons only its own slot.  A problem's results
// are the same bits alone, in any batch, in any slot, at any position of the table.  The lane-spread body forms a sum
// over the features in another order than sindy_step (sixteen partial sums, then the butterfly) and a sin / cos pair
// with one argument reduction: results agree with the single-model kernels to rounding, not bit for bit.
#pragma once
#include "ilqr_kernels.hpp"
#include "ilqr_sindy_table_host.hpp"

namespace ampc {

// The rows of the Jacobian kernel (the nominal trajectories of the plan's slots).
struct IlqrSindyRows {
  const double* states;       // [B][H + 1][nx]
  const double* ctrls;        // [B][H][nu]
  double* jx;                 // [B * H][nx][nx]
  double* ju;                 // [B * H][nx][nu]
  const int* refresh;         // [B]
  const int* slot_h;          // [B] or nullptr: H
  const int* slot_model;      // [B] or nullptr: entry 0
  const int* slot_of;         // row group -> slot (the slots with work first), or nullptr: identity
  int B, H, nx, nu;
};

// The rollouts, the objective and the acceptance of one slot on its (staged) entry `m`.
template <bool SPREAD>
__device__ __forceinline__ void is_run(const IlqrArgs<double>& args, const SindyDev<double>& m, double* lds,
                                       const IlqrSindyLds& L, const int p, const int mode) {
  using T = double;
  constexpr int M = kIsRows, NTHR = kIsRows * kIsLanes, TPS = kIsLanes, NR = 8;
  const int tid = threadIdx.x;
  const int nx = args.sindy.nx, nu = args.sindy.nu, no = args.obs_dim;
  const int HS = args.H, H = args.slot_h ? args.slot_h[p] : HS;      // array stride, this slot's horizon
  const int cost_stride = args.cost_stride, xs_ = L.xs, ntab = m.n_tab;
  const IlqrTableWork wk = make_ilqr_table_work(nx, nu, cost_stride);
  T* Wr = lds + L.work;
  T* Km = Wr + wk.K; T* kv = Wr + wk.k; T* ubar = Wr + wk.ubar; T* xbar = Wr + wk.xbar; T* cpar = Wr + wk.cpar;
  T* blo = Wr + wk.lo; T* bhi = Wr + wk.hi; T* lsobj = Wr + wk.lsobj; T* scal = Wr + wk.scal;
  int* piv = reinterpret_cast<int*>(Wr + wk.piv);
  const T* Qm = cpar; const T* Rm = Qm + no * no; const T* Fm = Rm + nu * nu;
  const T* goal = Fm + no * no;
  const T* clin = goal + no; const T* clint = clin + no;     // affine part of the stage / terminal cost
  T* xu = lds + L.xu;
  T* xnext = lds + L.xn;
  T* tab = lds + L.tab;

  T* st = args.states + (size_t)p * (HS + 1) * nx;
  T* ct = args.ctrls + (size_t)p * HS * nu;
  const T* Kg = args.Ks + (size_t)p * HS * nu * nx;
  const T* kg = args.ks + (size_t)p * HS * nu;

  // =========================== forward rollout(s) (ilqr.py:141-149, 196-205) ===================
  const int rows = mode == 0 ? 1 : args.ls_n;
  const int mr = tid / TPS, r = tid % TPS;        // row, lane of the row (same wave)
  T obj_part = T(0);
  const T alpha = args.alphas[mr];
  T* xrow = xu + mr * xs_;
  T* tr = tab + mr * ntab;
  for (int i = tid; i < M * nx; i += NTHR) {
    const int row = i / nx, col = i - row * nx;
    xu[row * xs_ + col] = st[col];
  }
  if (SPREAD && r == 0) tr[ntab - 1] = T(1);     // (the table's constant entry)
  __syncthreads();
  T* lss = args.ls_states + (size_t)p * args.ls_n * (HS + 1) * nx;
  T* lsc = args.ls_ctrls + (size_t)p * args.ls_n * HS * nu;
  // K_t, k_t, ubar_t, xbar_t reach LDS one step ahead, through registers: the global loads for step t + 1 are issued
  // at the top of step t and committed at its end; the barriers inside the loop are LDS-only
  constexpr int KR = (16 * 64 + NTHR - 1) / NTHR;
  T kreg[KR];
  T kvr = T(0), ubr = T(0), xbr = T(0);
  auto fetch_ls = [&](int t) {
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      const int idx = tid + k * NTHR;
      if (idx < nu * nx) kreg[k] = Kg[(size_t)t * nu * nx + idx];
    }
    if (tid < nu) { kvr = kg[(size_t)t * nu + tid]; ubr = ct[(size_t)t * nu + tid]; }
    if (tid < nx) xbr = st[(size_t)t * nx + tid];
  };
  auto commit_ls = [&]() {
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      const int idx = tid + k * NTHR;
      if (idx < nu * nx) Km[idx] = kreg[k];
    }
    if (tid < nu) { kv[tid] = kvr; ubar[tid] = ubr; }
    if (tid < nx) xbar[tid] = xbr;
  };
  if (mode == 1) {
    fetch_ls(0);
    commit_ls();
    __syncthreads();
  }
  const bool cdiag = args.cost_diag != 0, caff = args.cost_affine != 0;
  for (int t = 0; t < H; ++t) {
    if (mode == 1 && t + 1 < H) fetch_ls(t + 1);
    // controls for this step
    for (int a = r; a < nu; a += TPS) {
      T u;
      if (mode == 0) {
        u = ct[(size_t)t * nu + a];
      } else {
        // four partial sums over interleaved b (ilqr_iter_kernel)
        T f0 = T(0), f1 = T(0), f2 = T(0), f3 = T(0);
        int b = 0;
        for (; b + 4 <= nx; b += 4) {
          const T k0 = Km[a * nx + b], k1 = Km[a * nx + b + 1], k2 = Km[a * nx + b + 2], k3 = Km[a * nx + b + 3];
          const T d0 = xrow[b] - xbar[b], d1 = xrow[b + 1] - xbar[b + 1];
          const T d2 = xrow[b + 2] - xbar[b + 2], d3 = xrow[b + 3] - xbar[b + 3];
          f0 += k0 * d0; f1 += k1 * d1; f2 += k2 * d2; f3 += k3 * d3;
        }
        for (; b < nx; ++b) f0 += Km[a * nx + b] * (xrow[b] - xbar[b]);
        const T fb = (f0 + f1) + (f2 + f3);
        u = alpha * kv[a] + ubar[a] + fb;
        if (args.bounded) { u = u < blo[a] ? blo[a] : u; u = u > bhi[a] ? bhi[a] : u; }
        if (mr < rows) lsc[((size_t)mr * HS + t) * nu + a] = u;
      }
      xrow[nx + a] = u;
    }
    if (mode == 1 && mr < rows)
      for (int a = r; a < nx; a += TPS) lss[((size_t)mr * (HS + 1) + t) * nx + a] = xrow[a];
    lds_barrier();
    // objective: dt * (stage costs)
    obj_part += args.dt * (quad_rows<T>(Qm, xrow, goal, no, r, TPS, cdiag) +
                           quad_rows<T>(Rm, xrow + nx, nullptr, nu, r, TPS, cdiag));
    if (caff) obj_part += args.dt * affine_rows<T>(clin, xrow, goal, no, r, TPS, clint[no]);
    // dynamics
    if constexpr (SPREAD) {
      // (the row's lanes run in one wave: LDS accesses of a wave complete in order, no barrier between the phases)
      for (int j = r; j < m.n_trig; j += TPS) {
        const T arg = m.tpar[j] * xrow[m.tvar[j]];
        T sv, cv;
        sincos(arg, &sv, &cv);                   // (one argument reduction for the pair)
        tr[2 * j] = sv;
        tr[2 * j + 1] = cv;
      }
      for (int j = r; j < m.n_pow; j += TPS) tr[2 * m.n_trig + j] = pow(xrow[m.pvar[j]], m.ppar[j]);
      for (int j = r; j < m.n_mon; j += TPS)
        tr[2 * m.n_trig + m.n_pow + j] = sindy_monomial<T>(m.mpool, m.moff[j], m.mcnt[j], xrow, 1);
      T acc[NR];
#pragma unroll
      for (int i = 0; i < NR; ++i) acc[i] = T(0);
      const int last = nx - 1;
      for (int k = r; k < m.n_feat; k += TPS) {
        const int ix = m.fx[k], iy = m.fy[k];
        const T fa = xrow[ix >= 0 ? ix : 0], fb = tr[ix >= 0 ? 0 : -ix - 1], fc = tr[iy];
        const T f = (ix >= 0 ? fa : fb) * fc;
        // (coefficient rows past nx: the last row again, never stored)
#pragma unroll
        for (int i = 0; i < NR; ++i) acc[i] += m.xi[(i < last ? i : last) * m.n_feat + k] * f;
      }
      // (no branch per sum: side by side their DPP stages overlap)
      if (nx <= NR / 2) {
#pragma unroll
        for (int i = 0; i < NR / 2; ++i) acc[i] = sindy_group_sum<TPS>(acc[i]);
      } else {
#pragma unroll
        for (int i = 0; i < NR; ++i) acc[i] = sindy_group_sum<TPS>(acc[i]);
      }
      // next state: in every lane's registers; lane i of the row stores element i
#pragma unroll
      for (int i = 0; i < NR; ++i)
        if (i < nx) {
          const T xn = m.continuous ? xrow[i] + m.dt * acc[i] : acc[i];
          if (r == i) {
            xrow[i] = xn;
            if (mode == 0 && mr == 0) st[(size_t)(t + 1) * nx + i] = xn;
          }
        }
    } else {
      if (r == 0) sindy_step<T>(m, xrow, 1, xnext + mr * nx, 1, tr, 1);
      __syncthreads();
      for (int a = r; a < nx; a += TPS) {
        const T xn = xnext[mr * nx + a];
        xrow[a] = xn;
        if (mode == 0 && mr == 0) st[(size_t)(t + 1) * nx + a] = xn;
      }
    }
    // every thread passed the barrier above after its last read of K, k, ubar, xbar
    if (mode == 1 && t + 1 < H) commit_ls();
    lds_barrier();
  }
  if (mode == 1 && mr < rows)
    for (int a = r; a < nx; a += TPS) lss[((size_t)mr * (HS + 1) + H) * nx + a] = xrow[a];
  obj_part += quad_rows<T>(Fm, xrow, goal, no, r, TPS, cdiag);
  if (caff) obj_part += affine_rows<T>(clint, xrow, goal, no, r, TPS, clint[no + 1]);
#pragma unroll
  for (int off = TPS / 2; off > 0; off >>= 1) obj_part += __shfl_xor(obj_part, off);
  if (r == 0) lsobj[mr] = obj_part;
  __syncthreads();

  if (mode == 0) {
    if (tid == 0) {
      args.obj[p] = lsobj[0];
      args.active[p] = 1; args.converged[p] = 0; args.iters[p] = 0; args.status[p] = 0;
      args.refresh[p] = 1; args.ls_rows[p] = 0;
    }
    return;
  }

  // =========================== acceptance (ilqr.py:207-261) ====================================
  if (tid == 0) {
    const T obj = args.obj[p];
    const T lin_ = scal[0], quad_ = scal[1], ksn = scal[2];
    T best_obj = INFINITY;
    int best = -1, last = 0;
    for (int j = 0; j < rows; ++j) {
      last = j;
      const T a = args.alphas[j];
      const T new_obj = lsobj[j];
      const T expect = a * lin_ + a * a * quad_ / T(2);
      const T ratio = (obj - new_obj) / (-expect);
      if (ratio > args.ls_cost_threshold) { best_obj = new_obj; best = j; break; }
      if (new_obj < best_obj) { best_obj = new_obj; best = j; }
      if (ksn < args.u_threshold) break;
    }
    const bool success = (best_obj < obj) || (ksn < args.u_threshold);
    int sel = success ? best : last;
    int fail = 0;
    if (best < 0) { fail = 1; sel = 0; if (success) args.status[p] = 2; }
    const T new_obj = lsobj[sel];
    if (!success && new_obj > obj + T(1e-3)) fail = 1;
    piv[0] = sel; piv[1] = fail; piv[2] = success ? 1 : 0;
    scal[3] = new_obj;
    args.iters[p] += 1;
    args.ls_rows[p] += M;
  }
  __syncthreads();
  const int sel = piv[0], fail = piv[1], success = piv[2];
  if (fail) {
    if (tid == 0) { args.active[p] = 0; args.refresh[p] = 0; }
    return;
  }
  // ||new_ctrls - ctrls||, then swap in the selected candidate
  T du2 = T(0);
  for (int i = tid; i < H * nu; i += NTHR) {
    const T d = lsc[(size_t)sel * HS * nu + i] - ct[i];
    du2 += d * d;
  }
  du2 = block_sum_any(du2, lsobj, NTHR / 64);
  for (int i = tid; i < H * nu; i += NTHR) ct[i] = lsc[(size_t)sel * HS * nu + i];
  for (int i = tid; i < (H + 1) * nx; i += NTHR) st[i] = lss[(size_t)sel * (HS + 1) * nx + i];
  if (tid == 0) {
    const bool conv = sqrt(du2) < args.u_threshold;
    args.obj[p] = scal[3];
    args.refresh[p] = success;
    if (conv) { args.converged[p] = 1; args.active[p] = 0; }
    else if (args.max_iter > 0 && args.iters[p] >= args.max_iter) args.active[p] = 0;
    if (args.active[p] == 0) args.refresh[p] = 0;       // retired: nobody reads its Jacobians again
  }
}

__global__ __launch_bounds__(kIsRows * kIsLanes) void ilqr_iter_sindy_table_kernel(
    const SindyDev<double>* __restrict__ table, const IlqrArgs<double> args) {
  using T = double;
  constexpr int M = kIsRows, NTHR = kIsRows * kIsLanes;
  const int p = ilqr_slot(args);
  const int mode = args.slot_mode ? args.slot_mode[p] : args.mode;   // (queue: per slot)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* lds = reinterpret_cast<T*>(smem_raw);
  const int tid = threadIdx.x;
  const int nx = args.sindy.nx, nu = args.sindy.nu;
  if (mode == 1 && args.active[p] == 0) {
    if (tid == 0) args.refresh[p] = 0;
    return;
  }
  const SindyDev<T> mg = table[args.slot_model ? __builtin_amdgcn_readfirstlane(args.slot_model[p]) : 0];
  const IlqrSindyLds L = make_ilqr_sindy_lds(nx, nu, args.cost_stride, mg.n_tab, 0);
  const IlqrTableWork wk = make_ilqr_table_work(nx, nu, args.cost_stride);
  T* Wr = lds + L.work;
  T* cpar = Wr + wk.cpar; T* blo = Wr + wk.lo; T* bhi = Wr + wk.hi; T* scal = Wr + wk.scal;
  for (int i = tid; i < M * L.xs; i += NTHR) lds[L.xu + i] = T(0);
  for (int i = tid; i < args.cost_stride; i += NTHR)
    cpar[i] = args.costs_par[(size_t)args.cost_idx[p] * args.cost_stride + i];
  for (int i = tid; i < nu; i += NTHR) {
    blo[i] = args.bounded ? args.ubounds[i] : T(0);
    bhi[i] = args.bounded ? args.ubounds[nu + i] : T(0);
  }
  __syncthreads();
  // (backward Riccati sweep: launched just before this kernel)
  if (mode == 1) {
    const T* rin = args.ric + (size_t)p * kRicStride;
    if (rin[3] != T(0)) return;     // singular Quu: the sweep already retired this problem
    if (tid == 0) { scal[0] = rin[0]; scal[1] = rin[1]; scal[2] = rin[2]; }
    __syncthreads();
  }
  // (uniform over the workgroup: both branches stage with a barrier of their own)
  if (ilqr_sindy_table_spread(mg.n_tab, nx, mg.stage)) {
    const SindyDev<T> m = sindy_stage<T, true>(mg, lds + L.prog, tid, NTHR);
    is_run<true>(args, m, lds, L, p, mode);
  } else {
    const SindyDev<T> m = sindy_stage<T, false>(mg, lds + L.prog, tid, NTHR);
    is_run<false>(args, m, lds, L, p, mode);
  }
}

__global__ __launch_bounds__(kIsJacThreads) void ilqr_jac_sindy_table_kernel(const SindyDev<double>* __restrict__ table,
                                                                             const IlqrSindyRows a) {
  using T = double;
  constexpr int NT = kIsJacThreads, KP = kIsJacPairs;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* lds = reinterpret_cast<T*>(smem_raw);
  const int vg = blockIdx.x / a.H, t = blockIdx.x - vg * a.H;
  const int slot = a.slot_of ? __builtin_amdgcn_readfirstlane(a.slot_of[vg]) : vg;
  if (a.refresh[slot] == 0) return;
  if (t >= (a.slot_h ? a.slot_h[slot] : a.H)) return;
  const SindyDev<T> m = table[a.slot_model ? __builtin_amdgcn_readfirstlane(a.slot_model[slot]) : 0];
  const int lane = threadIdx.x, nx = a.nx, nu = a.nu, nv = nx + nu, nf = m.n_feat;
  const IlqrSindyJacLds L = make_ilqr_sindy_jac_lds(nx, nu);
  T* v = lds + L.v;
  T* G = lds + L.g;
  int* gvar = reinterpret_cast<int*>(lds + L.gvar);
  int* cnt = reinterpret_cast<int*>(lds + L.cnt);
  T* J = lds + L.J;
  const T* xs = a.states + ((size_t)slot * (a.H + 1) + t) * nx;
  const T* us = a.ctrls + ((size_t)slot * a.H + t) * nu;
  for (int c = lane; c < nv; c += NT) v[c] = c < nx ? xs[c] : us[c - nx];
  for (int e = lane; e < nx * nv; e += NT) J[e] = T(0);
  __syncthreads();
  const T twice = m.strict ? T(2) : T(1);
  for (int base = 0; base < nf; base += NT) {
    // ---- phase one: the partial derivatives of feature base + lane
    const int k = base + lane;
    int n = 0;
    if (k < nf) {
      const int kind = m.kind[k], c0 = m.a0[k], c1 = m.a1[k];
      if (kind == SF_MONO) {
        // d/dv_f of prod_j v_j ** e_j (basis_funcs.py:74-84), one per pair
        for (int f = 0; f < c1; ++f) {
          G[lane * KP + f] = sindy_monomial<T>(m.mpool, c0, c1, v, 1, f);
          gvar[lane * KP + f] = m.mpool[2 * (c0 + f)];
        }
        n = c1;
      } else {
        const T va = v[c0], vb = v[c1], par = m.par[k];
        T g0 = T(0), g1 = T(0);
        switch (kind) {
          case SF_ID: g0 = T(1); break;
          case SF_SIN: g0 = par * cos(par * va); break;
          case SF_COS: g0 = -par * sin(par * va); break;
          case SF_XSIN: g0 = twice * sin(par * vb); g1 = twice * va * par * cos(par * vb); break;
          case SF_XCOS: g0 = twice * cos(par * vb); g1 = -twice * va * par * sin(par * vb); break;
          default: g0 = (m.strict ? T(1) : par) * pow(va, par - T(1)); break;
        }
        G[lane * KP] = g0; gvar[lane * KP] = c0;
        n = 1;
        if (kind == SF_XSIN || kind == SF_XCOS) { G[lane * KP + 1] = g1; gvar[lane * KP + 1] = c1; n = 2; }
      }
    }
    cnt[lane] = n;
    __syncthreads();
    // ---- phase two: every entry adds its variable's partials, features ascending, first variable first
    const int nk = nf - base < NT ? nf - base : NT;
    for (int e = lane; e < nx * nv; e += NT) {
      const int i = e / nv, c = e - i * nv;
      T acc = J[e];
      for (int f = 0; f < nk; ++f) {
        const int nf_ = cnt[f];
        for (int s = 0; s < nf_; ++s)
          if (gvar[f * KP + s] == c) acc += m.xi[i * nf + base + f] * G[f * KP + s];
      }
      J[e] = acc;
    }
    __syncthreads();
  }
  T* Jx = a.jx + ((size_t)slot * a.H + t) * nx * nx;
  T* Ju = a.ju + ((size_t)slot * a.H + t) * nx * nu;
  for (int e = lane; e < nx * nv; e += NT) {
    const int i = e / nv, c = e - i * nv;
    T val = J[e];
    if (c < nx) {
      if (m.continuous) val = (i == c ? T(1) : T(0)) + m.dt * val;
      Jx[i * nx + c] = val;
    } else {
      if (m.continuous) val *= m.dt;
      Ju[i * nu + (c - nx)] = val;
    }
  }
}

}  // namespace ampc
