// mppi_sindy_table_kernels.hpp -- the MPPI rollout of a plan whose problems run on DIFFERENT SINDy models (any mix
// of feature libraries, coefficients and time modes) in ONE launch (ampc_mppi_plan_set_sindy_models).
//
// The single-model rollouts (sindy_kernels.hpp) receive their model as a by-value SindyDev<T> kernel argument.  Here a
// tile finds its problem through args.tile_prob, the problem's MppiProblem::model names an entry of a device array of
// SindyDev<T> (pointers into the models' handles, as kstep_sindy_kernels.hpp reads them), and the workgroup rolls its
// samples out on that entry.  Two bodies, picked per ENTRY by sindy_table_spread() -- a function of the entry and of
// plan constants (horizon cap, cost stride, AMPC_SINDY_FP as it stood when the table was set), never of the batch:
//
//   lane-spread   the arithmetic of mppi_rollout_sindy_fp_kernel<T, 16>: sixteen lanes share a sample.  Entries that
//                 are staged in LDS, have a product table and at most eight states, and whose LDS need fits.
//   one-thread    the arithmetic of mppi_rollout_sindy_kernel: one thread per sample.  Direct evaluation, programs
//                 read from global memory, more than eight states.
//
// Launch: n_tiles * 16 workgroups of 64 threads.  Workgroup b belongs to the plan's 64-sample tile b / 16; for a
// lane-spread entry it takes the four samples of sub-block b % 16, for a one-thread entry sub-block 0 takes the tile's
// 64 samples and the other fifteen return before any barrier (the decision is uniform over the workgroup).  The
// plan's tiling, offsets, output layout (costs / term_last / eps_out) and the update kernel are the single-model
// plan's.
//
// LDS map (elements of T; every offset follows the workgroup's OWN entry and the plan's hcap / cost_stride -- only the
// reserved byte count follows the plan's largest entry, so a problem's results are the same bits alone, in any plan,
// at any position, and the bits of the single-model kernels under AMPC_SINDY_G=16):
//   lane-spread   4 x { x|u [nx + nu], table [n_tab], noise row [hcap], shifted actions [hcap] } | cost block
//                 [cost_stride] | bounds [3 nu] | 1 | staged program
//   one-thread    x|u [nx + nu][64] | next x [nx][64] | table [n_tab][64] | cost block | bounds | 1 | staged program
//                 (when the entry is staged; else the program is read through flat pointers)
// The bodies restate the single-model kernels' statements in their order: same operations, same rounding
// (tests/test_gpu_mppi_sindy_table.py compares bit for bit).
#pragma once
#include <hip/hip_runtime.h>

#include "sindy_kernels.hpp"

namespace ampc {

constexpr int kSindyTabG = 16;            // lanes per sample of the lane-spread body
constexpr int kSindyTabSub = 16;          // workgroups per 64-sample tile

// bytes of the staged program of an entry (host_common.hpp: sindy_stage_bytes), from the entry alone
template <typename T> __host__ __device__ inline size_t sindy_table_stage_bytes(const SindyDev<T>& m) {
  if (!m.stage) return 0;
  return (sindy_prog_elems(m.nx, m.n_feat, m.n_trig, m.n_pow, m.n_mon, m.n_pool, sizeof(T)) + 2) * sizeof(T);
}
// LDS bytes of the two bodies for an entry (launch_mppi.cpp: lbf with G = 16, lb)
template <typename T>
__host__ __device__ inline size_t sindy_table_spread_bytes(const SindyDev<T>& m, int hcap, int cost_stride) {
  return ((size_t)(64 / kSindyTabG) * (m.nx + m.nu + m.n_tab + 2 * hcap) + cost_stride + 3 * m.nu + 2) * sizeof(T) +
         sindy_table_stage_bytes<T>(m);
}
template <typename T>
__host__ __device__ inline size_t sindy_table_thread_bytes(const SindyDev<T>& m, int cost_stride) {
  return ((size_t)(2 * m.nx + m.nu + m.n_tab) * 64 + cost_stride + 3 * m.nu + 2) * sizeof(T) +
         sindy_table_stage_bytes<T>(m);
}
// The selection rule (launch_mppi.cpp's for one model, G pinned to 16).
template <typename T>
__host__ __device__ inline bool sindy_table_spread(const SindyDev<T>& m, int hcap, int cost_stride, int fp_allowed,
                                                   size_t lds_limit) {
  return fp_allowed && m.stage && m.n_tab > 0 && m.nx <= 8 &&
         sindy_table_spread_bytes<T>(m, hcap, cost_stride) <= lds_limit;
}

// a * b + c in one rounding.  The single-model kernels' `c += lam_over_sigma * ca` is contracted to a fused multiply-add
// by the compiler; in this kernel, with two bodies in one function, the f32 build paired that addition with another one
// (a packed add) and left the product unfused -- one ulp on some costs.  Written out, the fusion does not depend on
// what surrounds it.
template <typename T> __device__ __forceinline__ T sindy_table_fma(T a, T b, T c) {
  if constexpr (sizeof(T) == 8) return __builtin_fma(a, b, c);
  else return __builtin_fmaf(a, b, c);
}

// ---- one thread per sample (mppi_rollout_sindy_kernel) ---------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void sindy_table_thread_body(const MppiArgs<T>& args, const SindyDev<T>& mg, T* lds,
                                                        const int tile, const int p, const MppiProblem<T>& pr) {
  constexpr int BS = 64;
  const SindyDev<T> m = sindy_stage<T>(
      mg, lds + (2 * mg.nx + mg.nu + mg.n_tab) * BS + args.cost_stride + 3 * mg.nu + 1, threadIdx.x, BS);
  const int lane = threadIdx.x, nx = m.nx, nu = m.nu, nv = nx + nu, no = args.obs_dim;
  const int n = (tile - pr.tile0) * BS + lane;
  const int H = pr.H, N = pr.N;
  const bool valid = n < N;
  T* v = lds + lane;                        // [nv][BS]  x | u
  T* o = lds + nv * BS + lane;              // [nx][BS]  next state
  T* tr = lds + (nv + nx) * BS + lane;      // [n_tab][BS]  per-thread table
  T* cpar = lds + (nv + nx + m.n_tab) * BS;   // Q R F goal | lo hi scale (shared)
  for (int i = lane; i < args.cost_stride; i += BS)
    cpar[i] = args.costs_par[(size_t)pr.cost_idx * args.cost_stride + i];
  for (int i = lane; i < 3 * nu; i += BS) cpar[args.cost_stride + i] = args.bounds[i];
  __syncthreads();
  const T* Qm = cpar; const T* Rm = Qm + no * no; const T* Fm = Rm + nu * nu;
  const T* goal = Fm + no * no;
  const T* lin = goal + no; const T* lint = lin + no;
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
    if (args.n_ind) c += indicator_all<T>(args.ind_tab, args.n_ind, v, BS, no);
    for (int i = 0; i < nu; ++i) {
      T s = T(0);
      for (int j = 0; j < nu; ++j) s += Rm[i * nu + j] * v[(nx + j) * BS];
      c += v[(nx + i) * BS] * s;
    }
    sindy_step<T>(m, v, BS, o, BS, tr, BS);
    for (int i = 0; i < nx; ++i) v[i * BS] = o[i * BS];
  }
  T term = T(0);
  for (int i = 0; i < no; ++i) {
    T s = T(0);
    for (int j = 0; j < no; ++j) s += Fm[i * no + j] * (v[j * BS] - goal[j]);
    term += (v[i * BS] - goal[i]) * (s + lint[i]);
  }
  term += lint[no + 1];
  c = sindy_table_fma<T>(pr.lam_over_sigma, ca, c);   // (c += lam_over_sigma * ca, fused: see sindy_table_fma)
  if (args.term_mode == 1) c += term;
  if (valid) {
    args.costs[pr.cost_off + n] = c;
    if (n == N - 1) args.term_last[p] = term;
  }
}

// ---- features spread over sixteen lanes per sample (mppi_rollout_sindy_fp_kernel<T, 16, IND>) -----------------------
template <typename T, bool IND>
__device__ __forceinline__ void sindy_table_spread_body(const MppiArgs<T>& args, const SindyDev<T>& mg, T* lds,
                                                        const int hcap, const int tile, const int sub, const int p,
                                                        const MppiProblem<T>& pr) {
  constexpr int G = kSindyTabG, BS = 64, SPB = BS / G, NR = 8;
  const int lane = threadIdx.x, nx = mg.nx, nu = mg.nu, nv = nx + nu, no = args.obs_dim, ntab = mg.n_tab;
  const int per_s = nv + ntab + 2 * hcap;
  T* cpar = lds + SPB * per_s;
  // (only staged entries come here: every pointer of `m` derives from the LDS array -- ds_read, not flat loads)
  const SindyDev<T> m = sindy_stage<T, true>(mg, cpar + args.cost_stride + 3 * nu + 1, lane, BS);
  const int sl = lane / G, g = lane - sl * G;               // sample of the block, lane of the group
  const int n = (tile - pr.tile0) * BS + sub * SPB + sl;
  const int H = pr.H, N = pr.N;
  const bool valid = n < N;
  T* v = lds + sl * per_s;                                   // this sample's x | u
  T* tr = v + nv;                                            // ... and its table
  T* er = tr + ntab;                                         // ... its noise row [H][nu]
  T* ar = er + hcap;                                         // ... and a[min(t + 1, H - 1)][nu]
  for (int i = lane; i < args.cost_stride; i += BS)
    cpar[i] = args.costs_par[(size_t)pr.cost_idx * args.cost_stride + i];
  for (int i = lane; i < 3 * nu; i += BS) cpar[args.cost_stride + i] = args.bounds[i];
  for (int i = g; i < nx; i += G) v[i] = args.x0[p * nx + i];
  if (g == 0) tr[ntab - 1] = T(1);
  {
    const T* eps_row = args.eps + pr.eps_off + (size_t)(n < pr.N ? n : 0) * pr.H * nu;
    for (int e = g; e < pr.H * nu; e += G) {
      const int t = e / nu, j = e - t * nu, ts = (t + 1 < pr.H) ? t + 1 : pr.H - 1;   // a[:-1] = a[1:]; a[-1] = a[-2]
      er[e] = n < pr.N ? eps_row[e] : T(0);
      ar[e] = args.act_in[pr.a_off + ts * nu + j];
    }
  }
  __syncthreads();
  const T* Qm = cpar; const T* Rm = Qm + no * no; const T* Fm = Rm + nu * nu;
  const T* goal = Fm + no * no;
  const T* lin = goal + no; const T* lint = lin + no;
  const T* blo = cpar + args.cost_stride; const T* bhi = blo + nu; const T* bsc = bhi + nu;
  T* epso = args.eps_out + pr.epso_off;
  const bool cdiag = args.cost_diag != 0;
  constexpr int KF = 2;
  T xreg[NR], qd[NR], gl[NR], ln[NR];
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    const int ix = i < no ? i : 0;
    xreg[i] = v[i < nx ? i : 0];
    qd[i] = Qm[ix * no + ix]; gl[i] = goal[ix]; ln[i] = lin[ix];
  }
  const T lc = lint[no];
  const bool t0 = g < m.n_trig;
  const int tv0 = t0 ? m.tvar[g] : 0;
  const T tp0 = t0 ? m.tpar[g] : T(0);
  int fxr[KF], fyr[KF];
  bool fk[KF];
  T xir[KF][NR];
#pragma unroll
  for (int q = 0; q < KF; ++q) {
    const int k = g + q * G;
    fk[q] = k < m.n_feat;
    const int kk = fk[q] ? k : 0;
    fxr[q] = m.fx[kk]; fyr[q] = m.fy[kk];
#pragma unroll
    for (int i = 0; i < NR; ++i) xir[q][i] = (fk[q] && i < nx) ? m.xi[(i < nx ? i : 0) * m.n_feat + kk] : T(0);
  }
  T c = T(0), ca = T(0);
  for (int t = 0; t < H; ++t) {
    for (int j = 0; j < nu; ++j) {
      const T a = ar[t * nu + j];
      T A = er[t * nu + j] + a;
      A = A < blo[j] ? blo[j] : A;
      A = A > bhi[j] ? bhi[j] : A;
      const T ec = A - a;
      if (valid && g == 0) epso[((size_t)t * N + n) * nu + j] = ec;
      ca += A * ec;
      const T uj = A * bsc[j];
      if (g == 0) v[nx + j] = uj;
      if (cdiag) c += uj * (Rm[j * nu + j] * uj);
    }
    // (the group's lanes run in one wave: LDS accesses of a wave complete in order, no barrier needed)
    if (cdiag) {
#pragma unroll
      for (int i = 0; i < NR; ++i)
        if (i < no) {
          const T d = xreg[i] - gl[i];
          c += d * (qd[i] * d + ln[i]);
        }
    } else {
      for (int i = 0; i < no; ++i) {
        T s = T(0);
        for (int j = 0; j < no; ++j) s += Qm[i * no + j] * (v[j] - goal[j]);
        c += (v[i] - goal[i]) * (s + lin[i]);
      }
      for (int i = 0; i < nu; ++i) {
        T s = T(0);
        for (int j = 0; j < nu; ++j) s += Rm[i * nu + j] * v[nx + j];
        c += v[nx + i] * s;
      }
    }
    c += lc;
    if constexpr (IND) {                   // indicator terms (threshold / box, mlp_tile.hpp), from the register copy
      for (int k = 0; k < args.n_ind; ++k) {
        const T* tk = args.ind_tab + (size_t)k * ind_stride(no);
        const int kind = (int)tk[0];
        bool viol = false, nan_in = false;
#pragma unroll
        for (int i = 0; i < NR; ++i)
          if (i < no) {
            viol = viol || ind_entry<T>(kind, xreg[i], tk[2 + i], tk[2 + no + i]);
            nan_in = nan_in || ind_void<T>(kind, xreg[i], tk[2 + no + i]);
          }
        if (viol && !nan_in) c += T(1);
      }
    }
    // ---- table entries of this lane (the first one from hoisted operands)
    if (t0) {
      const T arg = tp0 * v[tv0];
      T sv, cv;
      if constexpr (sizeof(T) == 8) sincos(arg, &sv, &cv);
      else sincosf(arg, &sv, &cv);
      tr[2 * g] = sv;
      tr[2 * g + 1] = cv;
    }
    for (int j = g + G; j < m.n_trig; j += G) {
      const T arg = m.tpar[j] * v[m.tvar[j]];
      T sv, cv;
      if constexpr (sizeof(T) == 8) sincos(arg, &sv, &cv);
      else sincosf(arg, &sv, &cv);
      tr[2 * j] = sv;
      tr[2 * j + 1] = cv;
    }
    for (int j = g; j < m.n_pow; j += G) tr[2 * m.n_trig + j] = pow(v[m.pvar[j]], m.ppar[j]);
    for (int j = g; j < m.n_mon; j += G)
      tr[2 * m.n_trig + m.n_pow + j] = sindy_monomial<T>(m.mpool, m.moff[j], m.mcnt[j], v, 1);
    // ---- features of this lane, times their coefficient column
    T acc[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) acc[i] = T(0);
#pragma unroll
    for (int q = 0; q < KF; ++q) {
      const int ix = fxr[q];
      const T fa = v[ix >= 0 ? ix : 0], fb = tr[ix >= 0 ? 0 : -ix - 1], fc = tr[fyr[q]];
      const T f = (ix >= 0 ? fa : fb) * fc;
#pragma unroll
      for (int i = 0; i < NR; ++i) acc[i] += xir[q][i] * f;
    }
    for (int k = g + KF * G; k < m.n_feat; k += G) {
      const int ix = m.fx[k], iy = m.fy[k];
      const T f = (ix >= 0 ? v[ix] : tr[-ix - 1]) * tr[iy];
#pragma unroll
      for (int i = 0; i < NR; ++i)
        if (i < nx) acc[i] += m.xi[i * m.n_feat + k] * f;
    }
    if (nx <= NR / 2) {
#pragma unroll
      for (int i = 0; i < NR / 2; ++i) acc[i] = sindy_group_sum<G>(acc[i]);
    } else {
#pragma unroll
      for (int i = 0; i < NR; ++i) acc[i] = sindy_group_sum<G>(acc[i]);
    }
    // ---- next state: in every lane's registers; lane i of the group refreshes the LDS copy
#pragma unroll
    for (int i = 0; i < NR; ++i)
      if (i < nx) {
        xreg[i] = m.continuous ? xreg[i] + m.dt * acc[i] : acc[i];
        if (g == i % G) v[i] = xreg[i];
      }
  }
  T term = T(0);
  for (int i = 0; i < no; ++i) {
    T s = T(0);
    for (int j = 0; j < no; ++j) s += Fm[i * no + j] * (v[j] - goal[j]);
    term += (v[i] - goal[i]) * (s + lint[i]);
  }
  term += lint[no + 1];
  c = sindy_table_fma<T>(pr.lam_over_sigma, ca, c);   // (c += lam_over_sigma * ca, fused: see sindy_table_fma)
  if (args.term_mode == 1) c += term;
  if (valid && g == 0) {
    args.costs[pr.cost_off + n] = c;
    if (n == N - 1) args.term_last[p] = term;
  }
}

// IND: the handle's cost has indicator terms (the lane-spread body's own instantiation, as in sindy_kernels.hpp).
// fp_allowed / lds_limit: plan constants of the selection rule.
template <typename T, bool IND>
__global__ __launch_bounds__(64) void mppi_rollout_sindy_table_kernel(const MppiArgs<T> args,
                                                                      const SindyDev<T>* __restrict__ table,
                                                                      const int hcap, const int fp_allowed,
                                                                      const unsigned lds_limit) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* lds = reinterpret_cast<T*>(smem_raw);
  const int tile = blockIdx.x / kSindyTabSub, sub = blockIdx.x - tile * kSindyTabSub;
  const int p = args.tile_prob[tile];
  const MppiProblem<T> pr = args.probs[p];
  const SindyDev<T> mg = table[pr.model];
  if (sindy_table_spread<T>(mg, hcap, args.cost_stride, fp_allowed, lds_limit)) {
    sindy_table_spread_body<T, IND>(args, mg, lds, hcap, tile, sub, p, pr);
  } else {
    if (sub != 0) return;                  // (uniform over the workgroup, before any barrier)
    sindy_table_thread_body<T>(args, mg, lds, tile, p, pr);
  }
}

}  // namespace ampc
