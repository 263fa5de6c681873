// ilqr_linear_table_kernels.hpp -- the iLQR iteration of a plan whose slots run on DIFFERENT linear models
// x' = A x + B u of mixed state dimension (ARX histories, Koopman lifts) (ampc_ilqr_plan_set_linear_models), the
// queue's refill and the bookkeeping of its closed loop (ampc_ilqr_closed_loop_linear).  f64 only.
//
// ilqr_riccati_wide_kernel (ilqr_wide.hpp) and ilqr_iter_kernel<double, 1, 8, 2> (ilqr_kernels.hpp) take their model
// from IlqrArgs::lin and index every per-slot array with the plan handle's nx.  Here a slot's model is an entry of a
// device array of LinDev<double>, named by slot_model[slot]; IlqrArgs keeps its layout (the shape plugins read it), so
// the table, the per-slot model array and the strides travel in a second kernel argument, IlqrLinTab.
//
// Layout rule: every per-slot and per-problem region keeps the stride of the plan's horizon H and of the WIDEST entry
// (nx_w, nxp_w, ldj_w); inside its region a slot's rows are packed at its OWN nx.  Kernel-internal indexing is the
// originals'; only the base pointers differ.  Nothing reads a region past what the slot's current model wrote, so a
// slot that held a wider model before leaves no trace.
//
// LDS: the sweep's WideLds is made from the entry's own nx (the launch reserves the widest entry's).  The line search
// keeps [x | u] [16][xs] at 0 with the entry's own row stride xs = lin_xs(kp), its next-state scratch [16][nx] behind
// the widest entry's rows (tab.lds_xn) and its compact work map behind the widest entry's scratch (tab.lds_work).
//
// Both kernels RESTATE the originals' statements in their order -- no floating-point statement changes its order or
// its operands -- so a problem's results are the bits of a single-model plan on the wide path, alone, in any batch,
// at any table position (tests/test_gpu_ilqr_linear_table.py compares bit for bit).
#pragma once
#include "ilqr_linear_table_host.hpp"
#include "mppi_linear_table_kernels.hpp"     // LinCtrlDesc, linear_ctrl_state_kernel: the closed loop's state rules

namespace ampc {

// ---- the backward sweep: ilqr_riccati_wide_kernel with the entry, its own WideLds and the strided base pointers -------
template <int NU>
__global__ __launch_bounds__(kRicThreads) void ilqr_riccati_wide_table_kernel(const IlqrArgs<double> args,
                                                                              const IlqrLinTab tab) {
  using T = double;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* Wr = reinterpret_cast<T*>(smem_raw);
  using acc_t = typename Acc<T>::type;
  constexpr int NTHR = kRicThreads, NW = NTHR / 64, nu = NU;
  const int tid = threadIdx.x, p = blockIdx.x, lane = tid & 63;
  const LinDev<T> lin = tab.table[tab.slot_model[p]];
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i16 = lane & 15, q = lane >> 4;
  const int ns = lin.nx, n = ns + nu, no = args.obs_dim, nsp = lin.nxp, ldJ = lin.ldj;
  const int HS = args.H, H = args.slot_h ? args.slot_h[p] : HS;      // array stride, this slot's horizon
  if (args.active[p] == 0) return;
  const WideLds L = make_wide_lds(ns, nu, no);
  T* V = Wr + L.V; T* vv = Wr + L.vv; T* qt = Wr + L.qt; T* Km = Wr + L.K; T* Zm = Wr + L.Z;
  T* Qux = Wr + L.Qux; T* Quu = Wr + L.Quu; T* goal = Wr + L.goal;
  T* xbar = Wr + L.xbar; T* ubar = Wr + L.ubar; T* scal = Wr + L.scal;
  const int ldV = L.ldV, ldB = L.ldB, nu4 = (nu + 3) / 4 * 4;
  const T* cpar = args.costs_par + (size_t)args.cost_idx[p] * args.cost_stride;      // Q R F goal lin lint
  const T* st = args.states + (size_t)p * (HS + 1) * tab.nx_w;
  const T* ct = args.ctrls + (size_t)p * HS * nu;
  T* Kg = args.Ks + (size_t)p * HS * nu * tab.nx_w;
  T* kg = args.ks + (size_t)p * HS * nu;
  T* vj = args.vj + (size_t)p * tab.nxp_w * tab.ldj_w;  // this slot's VJ scratch, [nsp][ldJ] inside
  const T* Jp = lin.jp;                               // [nsp][ldJ], zero padded
  const T dt = args.dt;
  for (int i = tid; i < L.total; i += NTHR) Wr[i] = T(0);
  __syncthreads();
  const T* Rp = cpar + no * no;
  auto CQ = [&](int a, int b) { return cpar[a * no + b] + cpar[b * no + a]; };
  auto CR = [&](int a, int b) { return Rp[a * nu + b] + Rp[b * nu + a]; };
  for (int i = tid; i < 3 * no; i += NTHR) goal[i] = cpar[2 * no * no + nu * nu + i];
  const T* clin = goal + no; const T* clint = clin + no;
  const T* Fp = cpar + no * no + nu * nu;
  for (int i = tid; i < no * no; i += NTHR) {         // V_H = F + F' on the observed block
    const int a = i / no, b = i - a * no;
    V[a * ldV + b] = Fp[a * no + b] + Fp[b * no + a];
  }
  __syncthreads();
  for (int a = tid; a < no; a += NTHR) {              // v_H (term_goal == 0: the reference's goal-less gradient)
    T s = T(0);
    for (int b = 0; b < no; ++b) s += V[a * ldV + b] * (st[(size_t)H * ns + b] - (args.term_goal ? goal[b] : T(0)));
    if (args.term_goal) s += clint[a];
    vv[a] = s;
  }
  for (int i = tid; i < ns; i += NTHR) xbar[i] = st[(size_t)(H - 1) * ns + i];
  for (int i = tid; i < nu; i += NTHR) ubar[i] = ct[(size_t)(H - 1) * nu + i];
  __syncthreads();
  const int ksn = nsp / 4, mts = nsp / 16, ntn = ldJ / 16;
  T lin_s = T(0), quad_s = T(0), ksn2 = T(0);         // meaningful in thread ns only
  int sing_any = 0;
  for (int t = H - 1; t >= 0; --t) {
    // ---- A: VJ = V J (to the global scratch);  qt = ct + J' v
    for (int tile = w; tile < mts * ntn; tile += NW) {
      const int mt = tile / ntn, nt = tile - mt * ntn;
      const T* a = V + (16 * mt + i16) * ldV + q;
      const T* b = Jp + (size_t)q * ldJ + 16 * nt + i16;
      acc_t acc = {0, 0, 0, 0};
      int ks = 0;
      for (; ks + 4 <= ksn; ks += 4) {                // four fragments in flight
        const T b0 = b[(size_t)(4 * ks) * ldJ], b1 = b[(size_t)(4 * ks + 4) * ldJ], b2 = b[(size_t)(4 * ks + 8) * ldJ],
                b3 = b[(size_t)(4 * ks + 12) * ldJ];
        const T a0 = a[4 * ks], a1 = a[4 * ks + 4], a2 = a[4 * ks + 8], a3 = a[4 * ks + 12];
        acc = mfma16(a0, b0, acc); acc = mfma16(a1, b1, acc); acc = mfma16(a2, b2, acc); acc = mfma16(a3, b3, acc);
      }
      for (; ks < ksn; ++ks) acc = mfma16(a[4 * ks], b[(size_t)(4 * ks) * ldJ], acc);
#pragma unroll
      for (int r = 0; r < 4; ++r) vj[(size_t)(16 * mt + acc_row<T>(q, r)) * ldJ + 16 * nt + i16] = acc[r];
    }
    for (int c = tid; c < n; c += NTHR) {
      T s = T(0);
      for (int a = 0; a < ns; ++a) s += Jp[(size_t)a * ldJ + c] * vv[a];
      T cc = T(0);
      if (c < no) {
        for (int b = 0; b < no; ++b) cc += CQ(c, b) * (xbar[b] - goal[b]);
        cc += clin[c];
      } else if (c >= ns) {
        for (int j = 0; j < nu; ++j) cc += CR(c - ns, j) * ubar[j];
      }
      qt[c] = cc * dt + s;
    }
    __syncthreads();                                  // (VJ: global stores visible to the workgroup)
    // ---- B: Qt = Ct + J' VJ, upper-triangular tiles; Qxx -> V, Qux, Quu
    for (int tile = w; tile < ntn * ntn; tile += NW) {
      const int mt = tile / ntn, nt = tile - mt * ntn;
      if (nt < mt || 16 * mt >= n || 16 * nt >= n) continue;
      const T* a = Jp + (size_t)q * ldJ + 16 * mt + i16;
      const T* b = vj + (size_t)q * ldJ + 16 * nt + i16;
      acc_t acc = {0, 0, 0, 0};
      int ks = 0;
      for (; ks + 4 <= ksn; ks += 4) {
        const size_t o0 = (size_t)(4 * ks) * ldJ, o1 = o0 + 4 * (size_t)ldJ, o2 = o1 + 4 * (size_t)ldJ, o3 = o2 + 4 * (size_t)ldJ;
        const T a0 = a[o0], a1 = a[o1], a2 = a[o2], a3 = a[o3];
        const T b0 = b[o0], b1 = b[o1], b2 = b[o2], b3 = b[o3];
        acc = mfma16(a0, b0, acc); acc = mfma16(a1, b1, acc); acc = mfma16(a2, b2, acc); acc = mfma16(a3, b3, acc);
      }
      for (; ks < ksn; ++ks) acc = mfma16(a[(size_t)(4 * ks) * ldJ], b[(size_t)(4 * ks) * ldJ], acc);
      const int s = 16 * nt + i16;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = 16 * mt + acc_row<T>(q, r);
        if (c >= n || s >= n || s < c) continue;      // (diagonal tiles: the upper half, mirrored below)
        T val = acc[r];
        if (c < no && s < no) val += CQ(c, s) * dt;
        else if (c >= ns && s >= ns) val += CR(c - ns, s - ns) * dt;
        if (s < ns) { V[c * ldV + s] = val; V[s * ldV + c] = val; }              // Qxx (c <= s < ns)
        else if (c < ns) Qux[(s - ns) * ldB + c] = val;                           // Qxu[c][s-ns] = Qux[s-ns][c]
        else { Quu[(c - ns) * nu4 + (s - ns)] = val; Quu[(s - ns) * nu4 + (c - ns)] = val; }
      }
    }
    __syncthreads();
    // ---- C: the nu x nu solves, one right-hand side per thread (columns 0..ns-1: Qux, column ns: qu)
    if (tid <= ns) {
      T A0[NU][NU], x[NU], x0[NU];
#pragma unroll
      for (int i = 0; i < NU; ++i) {
#pragma unroll
        for (int j = 0; j < NU; ++j) A0[i][j] = Quu[i * nu4 + j];
        x0[i] = tid < ns ? Qux[i * ldB + tid] : qt[ns + i];
        x[i] = x0[i];
      }
      int ok = ldl_solve_lane<T, NU>(A0, x);
      if (!ok) {                                       // (identical in every thread: Quu is shared)
#pragma unroll
        for (int i = 0; i < NU; ++i) x[i] = x0[i];
        sing_any |= lu_solve_lane<T, NU>(A0, x);
      }
      T l = T(0), qd = T(0), k2 = T(0);
#pragma unroll
      for (int i = 0; i < NU; ++i) x[i] = -x[i];
#pragma unroll
      for (int i = 0; i < NU; ++i) {
        T s = T(0);
#pragma unroll
        for (int j = 0; j < NU; ++j) s += A0[i][j] * x[j];
        l += x0[i] * x[i];
        qd += x[i] * s;
        k2 += x[i] * x[i];
        Km[i * ldB + tid] = x[i];                      // column ns: k
        Zm[i * ldB + tid] = x0[i] + s;                 // column ns: z = qu + Quu k
      }
      if (tid == ns) { lin_s += l; quad_s += qd; ksn2 += k2; }
    }
    __syncthreads();
    // ---- D: V = Qxx + Qxu K + K' Z (Z = Qux + Quu K);  v = qx + Qxu k + K' z;  store K_t, k_t
    for (int idx = tid; idx < ns * ns; idx += NTHR) {
      const int a = idx / ns, b = idx - a * ns;
      T s = V[a * ldV + b];
#pragma unroll
      for (int j = 0; j < NU; ++j) s += Qux[j * ldB + a] * Km[j * ldB + b] + Km[j * ldB + a] * Zm[j * ldB + b];
      V[a * ldV + b] = s;                              // (every thread reads and writes only its own entries of V)
    }
    for (int a = tid; a < ns; a += NTHR) {
      T s = qt[a];
#pragma unroll
      for (int j = 0; j < NU; ++j) s += Qux[j * ldB + a] * Km[j * ldB + ns] + Km[j * ldB + a] * Zm[j * ldB + ns];
      vv[a] = s;
    }
    for (int i = tid; i < nu * ns; i += NTHR) {
      const int j = i / ns, b = i - j * ns;
      Kg[(size_t)t * nu * ns + i] = Km[j * ldB + b];
    }
    if (tid < nu) kg[(size_t)t * nu + tid] = Km[tid * ldB + ns];
    if (t > 0) {
      for (int i = tid; i < ns; i += NTHR) xbar[i] = st[(size_t)(t - 1) * ns + i];
      for (int i = tid; i < nu; i += NTHR) ubar[i] = ct[(size_t)(t - 1) * nu + i];
    }
    __syncthreads();
  }
  if (sing_any) scal[0] = T(1);
  __syncthreads();
  if (tid == ns) {
    T* out = args.ric + (size_t)p * kRicStride;
    const T sg = scal[0];
    out[0] = lin_s; out[1] = quad_s; out[2] = sqrt(ksn2); out[3] = sg;
    if (sg != T(0)) {             // singular Quu: the reference raises LinAlgError here
      args.status[p] = 1; args.active[p] = 0; args.refresh[p] = 0;
    }
  }
}

// ---- the line search / rollout of the guess: ilqr_iter_kernel<double, 1, 8, 2> with the entry's nx, its own compact
//      work map and [x | u] stride, and the scratch behind the widest entry's ------------------------------------------
constexpr int kIltW = 8;                                        // waves per workgroup, as the wide path launches it

__global__ __launch_bounds__(64 * kIltW) void ilqr_iter_linear_table_kernel(const IlqrArgs<double> args,
                                                                            const IlqrLinTab tab) {
  using T = double;
  constexpr int W = kIltW;
  const int p = blockIdx.x;
  const int mode = args.slot_mode ? args.slot_mode[p] : args.mode;   // (queue: per slot)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* lds = reinterpret_cast<T*>(smem_raw);
  constexpr int M = 16, NTHR = 64 * W, TPS = NTHR / M;
  const int tid = threadIdx.x;
  const LinDev<T> lm = tab.table[tab.slot_model[p]];
  const int nx = lm.nx, nu = lm.nu, no = args.obs_dim;
  const int HS = args.H, H = args.slot_h ? args.slot_h[p] : HS;      // array stride, this slot's horizon
  const int xs_ = lin_xs(lm.kp, (int)sizeof(T));
  const int cost_stride = args.cost_stride;
  const IlqrWork wk = make_ilqr_work(nx, nu, cost_stride, true);
  T* Wr = lds + tab.lds_work;
  T* Km = Wr + wk.K; T* kv = Wr + wk.k;
  T* xbar = Wr + wk.xbar; T* ubar = Wr + wk.ubar; T* cpar = Wr + wk.cpar;
  T* blo = Wr + wk.lo; T* bhi = Wr + wk.hi; T* scal = Wr + wk.scal; T* lsobj = Wr + wk.lsobj;
  int* piv = reinterpret_cast<int*>(Wr + wk.piv);
  const T* Qm = cpar; const T* Rm = Qm + no * no; const T* Fm = Rm + nu * nu;
  const T* goal = Fm + no * no;
  const T* clin = goal + no; const T* clint = clin + no;     // affine part of the stage / terminal cost
  T* xu = lds;

  if (mode == 1 && args.active[p] == 0) {
    if (tid == 0) args.refresh[p] = 0;
    return;
  }

  for (int i = tid; i < M * xs_; i += NTHR) lds[i] = T(0);
  for (int i = tid; i < cost_stride; i += NTHR)
    cpar[i] = args.costs_par[(size_t)args.cost_idx[p] * cost_stride + i];
  for (int i = tid; i < nu; i += NTHR) {
    blo[i] = args.bounded ? args.ubounds[i] : T(0);
    bhi[i] = args.bounded ? args.ubounds[nu + i] : T(0);
  }
  __syncthreads();

  T* st = args.states + (size_t)p * (HS + 1) * tab.nx_w;
  T* ct = args.ctrls + (size_t)p * HS * nu;
  T* Kg = args.Ks + (size_t)p * HS * nu * tab.nx_w;
  T* kg = args.ks + (size_t)p * HS * nu;

  if (mode == 1) {
    const T* rin = args.ric + (size_t)p * kRicStride;
    if (rin[3] != T(0)) return;     // singular Quu: the sweep already retired this problem
    if (tid == 0) { scal[0] = rin[0]; scal[1] = rin[1]; scal[2] = rin[2]; }
    __syncthreads();
  }

  // =========================== forward rollout(s) (ilqr.py:141-149, 196-205) ===================
  const int rows = mode == 0 ? 1 : args.ls_n;
  const int m = tid / TPS, r = tid % TPS;        // row-in-tile, helper index (same wave)
  T obj_part = T(0);
  const T alpha = args.alphas[m];
  for (int i = tid; i < M * nx; i += NTHR) {
    const int row = i / nx, col = i - row * nx;
    xu[row * xs_ + col] = st[col];
  }
  __syncthreads();
  T* lss = args.ls_states + (size_t)p * args.ls_n * (HS + 1) * tab.nx_w;
  T* lsc = args.ls_ctrls + (size_t)p * args.ls_n * HS * nu;
  constexpr int KR = (16 * kLinMaxIlqrNx + NTHR - 1) / NTHR;
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
        T f0 = T(0), f1 = T(0), f2 = T(0), f3 = T(0);
        int b = 0;
        for (; b + 4 <= nx; b += 4) {
          const T k0 = Km[a * nx + b], k1 = Km[a * nx + b + 1], k2 = Km[a * nx + b + 2], k3 = Km[a * nx + b + 3];
          const T d0 = xu[m * xs_ + b] - xbar[b], d1 = xu[m * xs_ + b + 1] - xbar[b + 1];
          const T d2 = xu[m * xs_ + b + 2] - xbar[b + 2], d3 = xu[m * xs_ + b + 3] - xbar[b + 3];
          f0 += k0 * d0; f1 += k1 * d1; f2 += k2 * d2; f3 += k3 * d3;
        }
        for (; b < nx; ++b) f0 += Km[a * nx + b] * (xu[m * xs_ + b] - xbar[b]);
        const T fb = (f0 + f1) + (f2 + f3);
        u = alpha * kv[a] + ubar[a] + fb;
        if (args.bounded) { u = u < blo[a] ? blo[a] : u; u = u > bhi[a] ? bhi[a] : u; }
        if (m < rows) lsc[((size_t)m * HS + t) * nu + a] = u;
      }
      xu[m * xs_ + nx + a] = u;
    }
    if (mode == 1 && m < rows)
      for (int a = r; a < nx; a += TPS) lss[((size_t)m * (HS + 1) + t) * nx + a] = xu[m * xs_ + a];
    lds_barrier();
    // objective: dt * (stage costs)
    obj_part += args.dt * (quad_rows<T>(Qm, xu + m * xs_, goal, no, r, TPS, cdiag) +
                           quad_rows<T>(Rm, xu + m * xs_ + nx, nullptr, nu, r, TPS, cdiag));
    if (caff) obj_part += args.dt * affine_rows<T>(clin, xu + m * xs_, goal, no, r, TPS, clint[no]);
    {
      // x_{t+1} = M [x_t ; u_t] for the 16 rows: wave w takes output column tiles w, w + W, ...
      T* xnext = lds + tab.lds_xn;
      const int lane = tid & 63, wv = tid >> 6;
      for (int nt = wv; nt < lm.ntile; nt += W) {
        const typename Acc<T>::type acc = lin_tile<T>(lm, xu, xs_, nt, lane);
        const int col = 16 * nt + (lane & 15);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
          if (col < nx) xnext[acc_row<T>(lane >> 4, rr) * nx + col] = acc[rr];
      }
      __syncthreads();
      for (int a = r; a < nx; a += TPS) {
        const T xn = xnext[m * nx + a];
        xu[m * xs_ + a] = xn;
        if (mode == 0 && m == 0) st[(size_t)(t + 1) * nx + a] = xn;
      }
    }
    // every thread passed the barrier above after its last read of K, k, ubar, xbar
    if (mode == 1 && t + 1 < H) commit_ls();
    lds_barrier();
  }
  if (mode == 1 && m < rows)
    for (int a = r; a < nx; a += TPS) lss[((size_t)m * (HS + 1) + H) * nx + a] = xu[m * xs_ + a];
  obj_part += quad_rows<T>(Fm, xu + m * xs_, goal, no, r, TPS, cdiag);
  if (caff) obj_part += affine_rows<T>(clint, xu + m * xs_, goal, no, r, TPS, clint[no + 1]);
#pragma unroll
  for (int off = TPS / 2; off > 0; off >>= 1) obj_part += __shfl_xor(obj_part, off);
  if (r == 0) lsobj[m] = obj_part;
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
  du2 = block_sum_any(du2, lsobj, W);
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

// ---- continuous batching: ilqr_queue_refill_kernel with the region strides (q.nx = the widest entry's nx), the ragged
//      x0 and a harvest that zeroes what lies past the problem's own horizon and own nx ---------------------------------
__global__ __launch_bounds__(256) void ilqr_linear_table_refill_kernel(const IlqrArgs<double> args,
                                                                       const IlqrQueue<double> q, const IlqrLinTab tab,
                                                                       const int* __restrict__ x_off) {
  using T = double;
  __shared__ int next_s;
  const int p = blockIdx.x, tid = threadIdx.x;
  if (ilqr_slot_started(args, p, tid)) return;
  if (args.active[p] != 0 || args.slot_mode[p] == 0) return;      // running, or loaded and not yet started
  const int H = q.H, nxw = q.nx, nu = q.nu;
  T* st = args.states + (size_t)p * (H + 1) * nxw;
  T* ct = args.ctrls + (size_t)p * H * nu;
  const int j = q.slot_prob[p];
  if (j >= 0) {                                        // harvest, packed at the problem's own nx; the rest zero
    const int hj = q.horizon ? q.horizon[j] : H;
    const int nx = tab.table[q.model[j]].nx;
    for (int i = tid; i < (H + 1) * nxw; i += 256) q.out_states[(size_t)j * (H + 1) * nxw + i] = i < (hj + 1) * nx ? st[i] : T(0);
    for (int i = tid; i < H * nu; i += 256) q.out_ctrls[(size_t)j * H * nu + i] = i < hj * nu ? ct[i] : T(0);
    for (int i = tid; i < H * nu * nxw; i += 256)
      q.out_Ks[(size_t)j * H * nu * nxw + i] = i < hj * nu * nx ? args.Ks[(size_t)p * H * nu * nxw + i] : T(0);
    for (int i = tid; i < H * nu; i += 256) q.out_ks[(size_t)j * H * nu + i] = i < hj * nu ? args.ks[(size_t)p * H * nu + i] : T(0);
    if (tid == 0) {
      q.out_obj[j] = args.obj[p];
      q.out_flags[4 * j] = args.converged[p]; q.out_flags[4 * j + 1] = args.iters[p];
      q.out_flags[4 * j + 2] = args.status[p]; q.out_flags[4 * j + 3] = args.ls_rows[p];
    }
  }
  if (tid == 0) {
    int n = q.ctl[0] < q.P ? atomicAdd(&q.ctl[0], 1) : q.P;
    if (n >= q.P) n = -1;
    next_s = n;
    q.slot_prob[p] = n;
    if (n >= 0) {
      q.cost_idx[p] = q.cost[n]; args.slot_mode[p] = 0; args.refresh[p] = 0;
      if (q.horizon) q.slot_h[p] = q.horizon[n];
      q.slot_model[p] = q.model[n];
    }
    if (j >= 0) { __threadfence(); atomicAdd(&q.ctl[1], 1); }
  }
  __syncthreads();
  const int n = next_s;
  if (n < 0) return;
  const int nx = tab.table[q.model[n]].nx;
  for (int i = tid; i < nx; i += 256) st[i] = q.x0[x_off[n] + i];
  for (int i = tid; i < H * nu; i += 256) ct[i] = q.uguess[(size_t)n * H * nu + i];
}

// ---- device-resident closed loops (ampc_ilqr_closed_loop_linear) ---------------------------------------------------------
// As ilqr_chain_pre_kernel / ilqr_chain_post_kernel, with a slot carrying its chain's SURROGATE state (snx wide, sim
// [B][snx]) beside the controller state (row 0 of the slot's nominal trajectory).  Per iteration of the plan:
//   pre   stages u_0 and writes the slot's LinCtrlDesc (n = 0 for a slot that does not step)
//   surrogate step   next = surrogate.pred(sim, u_0) over the B rows
//   linear_ctrl_state_kernel (unchanged)   controller state <- rule(old state, u_0 as u_prev, next[:obs_dim])
//   post  records, keeps `next` as the slot's surrogate state, or hands the slot its next chain (whose initial
//         controller state has been through its rule once, with u_prev = 0, before the loop -- simulate()'s first run()).
__global__ __launch_bounds__(64) void ilqr_linear_chain_pre_kernel(const IlqrArgs<double> args, const IlqrLinChains q,
                                                                   const IlqrLinTab tab) {
  const int p = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) {
    q.need[p] = 0;
    q.desc[p] = LinCtrlDesc{0, 0, 0, 0, 0, 0};
  }
  if (ilqr_slot_started(args, p, tid)) return;
  if (args.active[p] != 0 || args.slot_mode[p] == 0) return;        // solving, or loaded and not yet started
  const int c = q.slot_chain[p];
  if (c < 0) { if (tid == 0) q.need[p] = 3; return; }
  if (tid == 0) q.chain_iters[c] += args.iters[p];
  if (args.status[p] == 1) {                    // singular Quu -- the reference's LinAlgError: the episode ends
    if (tid == 0) { q.chain_fail[c] = 1; q.need[p] = 2; }
    return;
  }
  const double* ct = args.ctrls + (size_t)p * q.H * q.nu;
  for (int i = tid; i < q.nu; i += 64) q.stage_u[(size_t)p * q.nu + i] = ct[i];
  if (tid == 0) {
    const int mi = q.slot_model[p];
    q.desc[p] = LinCtrlDesc{tab.table[mi].nx, q.rule[mi], q.n_basis[mi], mi, p * (q.H + 1) * q.nxw, q.lift_off[mi]};
    q.need[p] = 1;
  }
}

__global__ __launch_bounds__(256) void ilqr_linear_chain_post_kernel(const IlqrArgs<double> args, const IlqrLinChains q,
                                                                     const IlqrLinTab tab) {
  __shared__ int next_s;
  const int p = blockIdx.x, tid = threadIdx.x;
  const int need = q.need[p];
  if (need == 0) return;
  const int H = q.H, nxw = q.nxw, nu = q.nu, snx = q.snx, T1 = q.n_steps + 1;
  double* st = args.states + (size_t)p * (H + 1) * nxw;
  double* ct = args.ctrls + (size_t)p * H * nu;
  int c = q.slot_chain[p];
  bool finished = need == 2;
  if (need == 1) {
    const int t = q.chain_t[c];
    for (int i = tid; i < nu; i += 256) q.traj_ctrls[((size_t)c * T1 + t) * nu + i] = q.stage_u[(size_t)p * nu + i];
    for (int i = tid; i < snx; i += 256) {
      const double v = q.stage_next[(size_t)p * snx + i];
      q.traj_obs[((size_t)c * T1 + t + 1) * snx + i] = v;
      q.sim[(size_t)p * snx + i] = v;             // (the controller state: linear_ctrl_state_kernel, just before)
    }
    __syncthreads();
    if (tid == 0) q.chain_t[c] = t + 1;
    if (t + 1 < q.n_steps) {                      // the next solve starts from a zero guess (ilqr.py:280-281)
      for (int i = tid; i < H * nu; i += 256) ct[i] = 0.0;
      if (tid == 0) { args.slot_mode[p] = 0; args.refresh[p] = 0; }
      return;
    }
    finished = true;
  }
  if (tid == 0) {
    if (finished) { __threadfence(); atomicAdd(&q.ctl[1], 1); }
    int n = q.ctl[0] < q.C ? atomicAdd(&q.ctl[0], 1) : q.C;
    if (n >= q.C) n = -1;
    next_s = n;
    q.slot_chain[p] = n;
    if (n >= 0) {
      q.cost_idx[p] = q.cost[n]; args.slot_mode[p] = 0; args.refresh[p] = 0; q.chain_t[n] = 0;
      if (q.horizon) q.slot_h[p] = q.horizon[n];
      q.slot_model[p] = q.model[n];
    }
  }
  __syncthreads();
  const int n = next_s;
  if (n < 0) return;
  const int nx = tab.table[q.model[n]].nx;
  for (int i = tid; i < nx; i += 256) st[i] = q.x0[q.x_off[n] + i];
  for (int i = tid; i < snx; i += 256) {
    const double v = q.sim0[(size_t)n * snx + i];
    q.sim[(size_t)p * snx + i] = v;
    q.traj_obs[(size_t)n * T1 * snx + i] = v;
  }
  for (int i = tid; i < H * nu; i += 256) ct[i] = 0.0;
}

}  // namespace ampc
