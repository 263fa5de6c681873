// ilqr_table_kernels.hpp -- the model-touching half of an iLQR iteration for a plan whose slots run on MLP models of any
// mix of depth, widths and activation (ampc_ilqr_plan_set_model_table; gfx950, f64 only).  An iteration keeps its four
// launches: sweep | line search | forward | Jacobian chain.  The sweep is the plan's run-time-shape sweep
// (ilqr_kernels.hpp: it reads Jacobians from memory and depends on nx / nu only); the other three are here, on the
// model step of kstep_mlp_kernels.hpp, which reads plain nn.Linear parameters through a device table.
//
// Geometry, the same for every model: 256 threads = four waves, 16-row tiles.  A workgroup's model is
// models[slot_model[slot]] (entry 0 without per-slot models), read field by field through the pointer (wave-uniform
// loads; no by-value copy of the entry: kstep_mlp_kernels.hpp).  The layers are km_fetch_group / km_mma_group of that
// file (v_mfma_f64_16x16x4_f64 over 16-column output tiles, wave w takes the tiles w, w + 4, ..., weights from global
// memory / L2) with its padding rules: reduction indices >= in are selected to exact zeros on both operands, weight
// rows >= out land in columns that are stored as 0 or not at all.
//
// ilqr_iter_table_kernel   one workgroup per slot; the contract of ilqr_iter_kernel<.., DYN = 0> (ilqr_kernels.hpp),
//     statement for statement: mode 0 rolls out the guess (one row; states, obj, active / refresh), mode 1 the line
//     search -- the ls_n <= 16 step sizes are the rows of the tile, u = alpha k_t + ubar_t + K_t (x - xbar_t) clipped
//     when bounded, ls_states / ls_ctrls for rows < ls_n, objective dt (stage costs) + terminal cost through quad_rows
//     / affine_rows with the same per-row reduction -- then acceptance, the ||du|| test, the swap and the flags.
//     slot_mode, slot_h (stride H), slot_of, the early returns of retired slots and the singular-sweep flag ric[3] as
//     there.  Step: in = ([x, u] - xu_mean) / xu_std; a_{l+1} = act(a_l W_l' + b_l); x += z dy_std + dy_mean.  K_t, k_t,
//     ubar_t, xbar_t reach LDS one step ahead through registers.
//     LDS (doubles), fixed per plan by (nx, nu, cost stride) -- never by the models:
//       act[2][16][257]   the two activation buffers; the normalised input goes into act[1]
//       xu[16][81]        the raw [x | u] rows (odd stride)
//       norm[288]         xu_mean[80] xu_std[80] dy_mean[64] dy_std[64]                -- kItOffWork = 9808 doubles
//       K [nu][nx], k, ubar, xbar, cost block, lo, hi, lsobj[16], scal[16], piv        (ilqr_table_host.hpp)
// ilqr_fwd_table_kernel    one forward pass over the rows (slot, t < the slot's horizon) of the slots with refresh != 0,
//     grouped per slot and padded to 16 so that a tile has one model (the RowMap / gpad scheme of per-slot models,
//     mlp_kernels.hpp); stores act'(z_l) of every hidden layer to dz [hidden layer][slot * gpad + t][wmax], wmax the
//     table's widest hidden layer rounded up to 16.  LDS: act[2][16][257].
// ilqr_jac_table_kernel    jx = I + diag(dy_std) J_net diag(1 / xu_std)[:, :nx], ju = ..[:, nx:] into the plan's jx / ju
//     in the layout mlp_jacobian_kernel writes and the sweeps read ([slot * H + t][i][c]).  Forward mode over tangent
//     rows: the rows (t, c), c < nx + nu, of one slot are flattened into 16-row tiles;
//       T_1[(t, c)][j] = d_1[t][j] W_1[j][c] / xu_std[c]                 (no sum)
//       T_l = (T_{l-1} W_l') * d_l[t]                                    (a layer without bias; the stored derivative
//                                                                         of the row's t instead of the activation)
//       J[(t, c)][i] = (T_L W_out')[i] dy_std[i] + [i == c]               (the output layer's epilogue stores it)
//     LDS: act[2][16][257].
//
// Sums.  An output element of a layer -- forward or tangent -- accumulates over k in blocks of 16 in order, inside a
// block as the MFMA does (t = 0..3 in order, each the sum over q = 0..3 of the products at k = 16 kb + 4 q + t): a
// function of the layer's own `in`.  A Jacobian entry is therefore the sum over the LAST hidden layer's units in that
// order of products that were themselves summed the same way layer by layer from the input side (forward mode:
// W_out (D_L W_L (.. (D_1 W_1)))), where mlp_jacobian_kernel sums from the output side.  A candidate's objective: each
// of its row's 16 threads adds its terms in step order, the 16 partials meet in a butterfly of shuffles.  ||du||^2:
// block_sum_any over four waves.  No atomics; no index depends on a state value, so a NaN poisons only its own slot.  A
// problem's results are the same bits alone, in any batch, in any slot, at any position of the table, from run to run.
#pragma once
#include "ilqr_kernels.hpp"
#include "ilqr_table_host.hpp"
#define AMPC_KM_LAYERS_ONLY          // the layer routines and the table entry, not the k-step kernel
#include "kstep_mlp_kernels.hpp"

namespace ampc {

constexpr int kItRows = kKmRows;              // rows per tile: the line search's step sizes
constexpr int kItThreads = kKmThreads;
constexpr int kItTps = kItThreads / kItRows;  // threads per row: 16, a quarter wave
constexpr int kItXuStride = kKmMaxIn + 1;
static_assert(kItRows == kIlqrMaxLs && kItTps == 16 && kMaxNu <= kItTps, "thread (m, j) owns control j of step size m");
// LDS map, in doubles
constexpr int kItOffAct = 0;
constexpr int kItOffXu = 2 * kItRows * kKmActStride;
constexpr int kItOffNorm = kItOffXu + kItRows * kItXuStride;
constexpr int kItOffWork = (kItOffNorm + 2 * kKmMaxIn + 2 * kKmMaxOut + 3) / 4 * 4;
constexpr size_t kItRowsLdsBytes = (size_t)2 * kItRows * kKmActStride * 8;       // the forward / Jacobian kernels
constexpr int kItMaxGain = 16 * 63;           // nu nx <= 16 * 63 gains, staged through registers
constexpr int kItKr = (kItMaxGain + kItThreads - 1) / kItThreads;

// The rows of the refresh kernels (the nominal trajectories of the plan's slots).
struct IlqrTableRows {
  const double* states;       // [B][H + 1][nx]
  const double* ctrls;        // [B][H][nu]
  double* dz;                 // [hidden layer][B * gpad][wmax]
  double* jx;                 // [B * H][nx][nx]
  double* ju;                 // [B * H][nx][nu]
  const int* refresh;         // [B]
  const int* slot_h;          // [B] or nullptr: H
  const int* slot_model;      // [B] or nullptr: entry 0
  const int* slot_of;         // row group -> slot (the slots with work first), or nullptr: identity
  int B, H, gpad, nx, nu, wmax;
  int tiles;                  // 16-row tiles per slot: gpad / 16 (forward), ceil(H (nx + nu) / 16) (Jacobians)
};

// acc[t] = bin W_t' over the whole reduction, for the NT tiles w, w + 4, ... of wave w (km_layer's loop).
template <int NT>
__device__ __forceinline__ void it_mma(d4 (&acc)[NT], const double* __restrict__ W, int in, int out, const double* bin,
                                       int w, int lane) {
  const int i = lane & 15, q = lane >> 4;
  int roff[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int col = 16 * (w + kKmWaves * t) + i;
    roff[t] = (col < out ? col : out - 1) * in;
    acc[t] = d4{0.0, 0.0, 0.0, 0.0};
  }
  const double* ap = bin + i * kKmActStride;
  const int ng = (in + 16 * kKmGroup - 1) / (16 * kKmGroup);
  double b0[NT][4 * kKmGroup], b1[NT][4 * kKmGroup];
  km_fetch_group<NT>(b0, W, roff, 0, q, in);
#pragma unroll 1
  for (int g = 0; g < ng; g += 2) {
    if (g + 1 < ng) km_fetch_group<NT>(b1, W, roff, g + 1, q, in);
    km_mma_group<NT>(acc, b0, ap, g, q, in);
    if (g + 2 < ng) km_fetch_group<NT>(b0, W, roff, g + 2, q, in);
    if (g + 1 < ng) km_mma_group<NT>(acc, b1, ap, g + 1, q, in);
  }
}

// A hidden layer: bout = act(bin W' + b); DERIV: act'(z) to dzl [16][wmax] as well (columns >= out: 0).
// accumulator register r of lane (i, q): row q + 4 r, column 16 (w + 4 t) + i
template <int NT, bool DERIV>
__device__ __forceinline__ void it_hidden(const double* __restrict__ W, const double* __restrict__ B, int in, int out,
                                          int act, const double* bin, double* bout, int w, int lane, double* dzl, int wmax) {
  const int i = lane & 15, q = lane >> 4;
  d4 acc[NT];
  it_mma<NT>(acc, W, in, out, bin, w, lane);
  // (z first, the activation in place one column tile at a time: kstep_mlp_kernels.hpp, km_layer)
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int c = 16 * (w + kKmWaves * t) + i;
    const double bias = B[c < out ? c : out - 1];
#pragma unroll
    for (int r = 0; r < 4; ++r) bout[(q + 4 * r) * kKmActStride + c] = acc[t][r] + bias;
  }
#pragma unroll 1
  for (int t = 0; t < NT; ++t) {
    const int c = 16 * (w + kKmWaves * t) + i;
    double* p = bout + q * kKmActStride + c;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double z = p[4 * r * kKmActStride];
      const double v = act_apply<double>(act, z);
      p[4 * r * kKmActStride] = c < out ? v : 0.0;
      if constexpr (DERIV) {
        const double d = act_deriv<double>(act, z);
        dzl[(size_t)(q + 4 * r) * wmax + c] = c < out ? d : 0.0;
      }
    }
  }
}

// The output layer of a step (one tile per wave): xu[:, c] += z dy_std + dy_mean.
__device__ __forceinline__ void it_output(const double* __restrict__ W, const double* __restrict__ B, int in, int out,
                                          const double* bin, int w, int lane, double* xu, const double* norm) {
  const int i = lane & 15, q = lane >> 4;
  d4 acc[1];
  it_mma<1>(acc, W, in, out, bin, w, lane);
  const int c = 16 * w + i;
  if (c >= out) return;
  const double bias = B[c];
  const double dm = norm[2 * kKmMaxIn + c], ds = norm[2 * kKmMaxIn + kKmMaxOut + c];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    double* x = xu + (q + 4 * r) * kItXuStride + c;
    *x = *x + ((acc[0][r] + bias) * ds + dm);
  }
}

// The layers of one model step on the tile: act[1] holds the normalised input, xu the raw rows.
__device__ __forceinline__ void it_step(const KstepMlpModel* md, int nl, int act, double* buf0, double* buf1, double* xu,
                                        const double* norm, int w, int lane) {
  for (int l = 0; l < nl; ++l) {
    const int in = md->dims[l], out = md->dims[l + 1];
    const double* W = md->w[l];
    const double* B = md->b[l];
    const double* bin = ((l + 1) & 1) ? buf1 : buf0;
    double* bout = (l & 1) ? buf1 : buf0;
    const int ct = (out + 15) / 16;
    const int ntw = w < ct ? (ct - w + kKmWaves - 1) / kKmWaves : 0;     // this wave's tiles (wave-uniform)
    static_assert(kKmMaxTiles == 4, "one case per tile count");
    if (l == nl - 1) {
      if (ntw == 1) it_output(W, B, in, out, bin, w, lane, xu, norm);
    } else {
      switch (ntw) {
        case 1: it_hidden<1, false>(W, B, in, out, act, bin, bout, w, lane, nullptr, 0); break;
        case 2: it_hidden<2, false>(W, B, in, out, act, bin, bout, w, lane, nullptr, 0); break;
        case 3: it_hidden<3, false>(W, B, in, out, act, bin, bout, w, lane, nullptr, 0); break;
        case 4: it_hidden<4, false>(W, B, in, out, act, bin, bout, w, lane, nullptr, 0); break;
        default: break;
      }
    }
    lds_barrier();
  }
}

__global__ __launch_bounds__(kItThreads) void ilqr_iter_table_kernel(const KstepMlpModel* __restrict__ models,
                                                                     const IlqrArgs<double> args) {
  using T = double;
  const int p = ilqr_slot(args);
  const int mode = args.slot_mode ? args.slot_mode[p] : args.mode;   // (queue: per slot)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* lds = reinterpret_cast<T*>(smem_raw);
  constexpr int M = kItRows, NTHR = kItThreads, TPS = kItTps;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const KstepMlpModel* md = models + (args.slot_model ? __builtin_amdgcn_readfirstlane(args.slot_model[p]) : 0);
  const int nl = md->n_layers, act = md->act;
  const int nx = args.mlp.nx, nu = args.mlp.nu, kin = nx + nu, no = args.obs_dim;     // (no == nx: checked by the host)
  const int HS = args.H, H = args.slot_h ? args.slot_h[p] : HS;      // array stride, this slot's horizon
  const int cost_stride = args.cost_stride;
  const IlqrTableWork wk = make_ilqr_table_work(nx, nu, cost_stride);
  T* buf0 = lds + kItOffAct;
  T* buf1 = buf0 + M * kKmActStride;
  T* xu = lds + kItOffXu;
  T* norm = lds + kItOffNorm;
  T* Wr = lds + kItOffWork;
  T* Km = Wr + wk.K; T* kv = Wr + wk.k; T* ubar = Wr + wk.ubar; T* xbar = Wr + wk.xbar; T* cpar = Wr + wk.cpar;
  T* blo = Wr + wk.lo; T* bhi = Wr + wk.hi; T* lsobj = Wr + wk.lsobj; T* scal = Wr + wk.scal;
  int* piv = reinterpret_cast<int*>(Wr + wk.piv);
  const T* Qm = cpar; const T* Rm = Qm + no * no; const T* Fm = Rm + nu * nu;
  const T* goal = Fm + no * no;
  const T* clin = goal + no; const T* clint = clin + no;     // affine part of the stage / terminal cost

  if (mode == 1 && args.active[p] == 0) {
    if (tid == 0) args.refresh[p] = 0;
    return;
  }

  for (int i = tid; i < kin; i += NTHR) {
    norm[i] = md->norm[0][i];
    norm[kKmMaxIn + i] = md->norm[1][i];
  }
  for (int i = tid; i < nx; i += NTHR) {
    norm[2 * kKmMaxIn + i] = md->norm[2][i];
    norm[2 * kKmMaxIn + kKmMaxOut + i] = md->norm[3][i];
  }
  for (int i = tid; i < cost_stride; i += NTHR)
    cpar[i] = args.costs_par[(size_t)args.cost_idx[p] * cost_stride + i];
  for (int i = tid; i < nu; i += NTHR) {
    blo[i] = args.bounded ? args.ubounds[i] : T(0);
    bhi[i] = args.bounded ? args.ubounds[nu + i] : T(0);
  }
  __syncthreads();

  T* st = args.states + (size_t)p * (HS + 1) * nx;
  T* ct = args.ctrls + (size_t)p * HS * nu;
  const T* Kg = args.Ks + (size_t)p * HS * nu * nx;
  const T* kg = args.ks + (size_t)p * HS * nu;

  // (backward Riccati sweep: launched just before this kernel)
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
  T* xrow = xu + m * kItXuStride;
  for (int a = r; a < nx; a += TPS) xrow[a] = st[a];
  __syncthreads();
  T* lss = args.ls_states + (size_t)p * args.ls_n * (HS + 1) * nx;
  T* lsc = args.ls_ctrls + (size_t)p * args.ls_n * HS * nu;
  // K_t, k_t, ubar_t, xbar_t reach LDS one step ahead, through registers: the global loads for step t + 1 are issued
  // at the top of step t and committed at its end; the barriers inside the loop are LDS-only
  T kreg[kItKr];
  T kvr = T(0), ubr = T(0), xbr = T(0);
  auto fetch_ls = [&](int t) {
#pragma unroll
    for (int k = 0; k < kItKr; ++k) {
      const int idx = tid + k * NTHR;
      if (idx < nu * nx) kreg[k] = Kg[(size_t)t * nu * nx + idx];
    }
    if (tid < nu) { kvr = kg[(size_t)t * nu + tid]; ubr = ct[(size_t)t * nu + tid]; }
    if (tid < nx) xbr = st[(size_t)t * nx + tid];
  };
  auto commit_ls = [&]() {
#pragma unroll
    for (int k = 0; k < kItKr; ++k) {
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
    // controls for this step: thread (m, a = r)
    if (r < nu) {
      const int a = r;
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
        if (m < rows) lsc[((size_t)m * HS + t) * nu + a] = u;
      }
      xrow[nx + a] = u;
    }
    if (mode == 1 && m < rows)
      for (int a = r; a < nx; a += TPS) lss[((size_t)m * (HS + 1) + t) * nx + a] = xrow[a];
    lds_barrier();
    // objective: dt * (stage costs)
    obj_part += args.dt * (quad_rows<T>(Qm, xrow, goal, no, r, TPS, cdiag) +
                           quad_rows<T>(Rm, xrow + nx, nullptr, nu, r, TPS, cdiag));
    if (caff) obj_part += args.dt * affine_rows<T>(clin, xrow, goal, no, r, TPS, clint[no]);
    // dynamics
    for (int c = r; c < kin; c += TPS) buf1[m * kKmActStride + c] = (xrow[c] - norm[c]) / norm[kKmMaxIn + c];
    lds_barrier();
    it_step(md, nl, act, buf0, buf1, xu, norm, w, lane);
    if (mode == 0 && m == 0)
      for (int a = r; a < nx; a += TPS) st[(size_t)(t + 1) * nx + a] = xrow[a];
    // every thread passed a barrier above after its last read of K, k, ubar, xbar
    if (mode == 1 && t + 1 < H) commit_ls();
    lds_barrier();
  }
  if (mode == 1 && m < rows)
    for (int a = r; a < nx; a += TPS) lss[((size_t)m * (HS + 1) + H) * nx + a] = xrow[a];
  obj_part += quad_rows<T>(Fm, xrow, goal, no, r, TPS, cdiag);
  if (caff) obj_part += affine_rows<T>(clint, xrow, goal, no, r, TPS, clint[no + 1]);
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
  du2 = block_sum_any(du2, lsobj, kKmWaves);
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

// The slot, its horizon and the tile's first row of a refresh workgroup; false: nothing to do for it.
__device__ __forceinline__ bool it_rows_tile(const IlqrTableRows& a, int* slot, int* hs, int* first) {
  const int vg = blockIdx.x / a.tiles;
  const int s = a.slot_of ? __builtin_amdgcn_readfirstlane(a.slot_of[vg]) : vg;
  *slot = s;
  *first = (blockIdx.x - vg * a.tiles) * kItRows;
  if (a.refresh[s] == 0) return false;
  *hs = a.slot_h ? a.slot_h[s] : a.H;
  return true;
}

__global__ __launch_bounds__(kItThreads) void ilqr_fwd_table_kernel(const KstepMlpModel* __restrict__ models,
                                                                    const IlqrTableRows a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  double* buf0 = reinterpret_cast<double*>(smem_raw);
  double* buf1 = buf0 + kItRows * kKmActStride;
  int slot, Hs, t0;
  if (!it_rows_tile(a, &slot, &Hs, &t0) || t0 >= Hs) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const KstepMlpModel* md = models + (a.slot_model ? __builtin_amdgcn_readfirstlane(a.slot_model[slot]) : 0);
  const int nl = md->n_layers, act = md->act;
  const int nx = a.nx, nu = a.nu, kin = nx + nu;
  const int m = tid / kItTps, r = tid % kItTps;
  {
    const int t = t0 + m;
    const bool live = t < Hs;                                       // (rows past the slot's horizon: zeros)
    const double* xs = a.states + ((size_t)slot * (a.H + 1) + (live ? t : 0)) * nx;
    const double* us = a.ctrls + ((size_t)slot * a.H + (live ? t : 0)) * nu;
    const double* mean = md->norm[0];
    const double* sd = md->norm[1];
    for (int c = r; c < kin; c += kItTps) {
      const double v = c < nx ? xs[c] : us[c - nx];
      buf1[m * kKmActStride + c] = live ? (v - mean[c]) / sd[c] : 0.0;
    }
  }
  __syncthreads();
  const size_t lstride = (size_t)a.B * a.gpad * a.wmax;
  double* dz0 = a.dz + ((size_t)slot * a.gpad + t0) * a.wmax;
  for (int l = 0; l + 1 < nl; ++l) {
    const int in = md->dims[l], out = md->dims[l + 1];
    const double* W = md->w[l];
    const double* B = md->b[l];
    const double* bin = ((l + 1) & 1) ? buf1 : buf0;
    double* bout = (l & 1) ? buf1 : buf0;
    double* dzl = dz0 + (size_t)l * lstride;
    const int ct = (out + 15) / 16;
    const int ntw = w < ct ? (ct - w + kKmWaves - 1) / kKmWaves : 0;     // this wave's tiles (wave-uniform)
    switch (ntw) {
      case 1: it_hidden<1, true>(W, B, in, out, act, bin, bout, w, lane, dzl, a.wmax); break;
      case 2: it_hidden<2, true>(W, B, in, out, act, bin, bout, w, lane, dzl, a.wmax); break;
      case 3: it_hidden<3, true>(W, B, in, out, act, bin, bout, w, lane, dzl, a.wmax); break;
      case 4: it_hidden<4, true>(W, B, in, out, act, bin, bout, w, lane, dzl, a.wmax); break;
      default: break;
    }
    __syncthreads();
  }
}

// A tangent layer: bout = (bin W') * d[t of the row], columns >= out: 0.  dzr[r]: the stored derivatives of the
// step of accumulator row q + 4 r.
template <int NT>
__device__ __forceinline__ void it_tangent(const double* __restrict__ W, int in, int out, const double* bin, double* bout,
                                           int w, int lane, const double* const (&dzr)[4]) {
  const int i = lane & 15, q = lane >> 4;
  d4 acc[NT];
  it_mma<NT>(acc, W, in, out, bin, w, lane);
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int c = 16 * (w + kKmWaves * t) + i;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double d = dzr[r][c < out ? c : out - 1];
      bout[(q + 4 * r) * kKmActStride + c] = c < out ? acc[t][r] * d : 0.0;
    }
  }
}

__global__ __launch_bounds__(kItThreads) void ilqr_jac_table_kernel(const KstepMlpModel* __restrict__ models,
                                                                    const IlqrTableRows a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  double* buf0 = reinterpret_cast<double*>(smem_raw);
  double* buf1 = buf0 + kItRows * kKmActStride;
  int slot, Hs, j0;
  if (!it_rows_tile(a, &slot, &Hs, &j0)) return;
  const int nx = a.nx, nu = a.nu, kin = nx + nu;
  const int nrows = Hs * kin;                                     // tangent rows (t, c) of this slot
  if (j0 >= nrows) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const KstepMlpModel* md = models + (a.slot_model ? __builtin_amdgcn_readfirstlane(a.slot_model[slot]) : 0);
  const int nl = md->n_layers;
  const size_t lstride = (size_t)a.B * a.gpad * a.wmax;
  const double* dzs = a.dz + (size_t)slot * a.gpad * a.wmax;      // this slot's rows of layer 0
  // T_1[(t, c)][j] = d_1[t][j] W_1[j][c] / xu_std[c]: thread (m, r) walks the columns r, r + 16, ... of row m
  {
    const int m = tid / kItTps, r = tid % kItTps;
    const int jj = j0 + m;
    const bool live = jj < nrows;
    const int t = live ? jj / kin : 0, c = live ? jj - t * kin : 0;
    const int d1 = md->dims[1];
    const double* W1 = md->w[0];
    const double sd = md->norm[1][c];
    const double* d = dzs + (size_t)t * a.wmax;
    for (int j = r; j < d1; j += kItTps) buf0[m * kKmActStride + j] = live ? d[j] * W1[(size_t)j * kin + c] / sd : 0.0;
  }
  // the step and the input column of this lane's four accumulator rows
  const int i = lane & 15, q = lane >> 4;
  int rt[4], rc[4];
  const double* dzr[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int jj = j0 + q + 4 * r;
    const int t = jj / kin;
    rt[r] = jj < nrows ? t : -1;                                  // (-1: a row past the slot's last one, never stored)
    rc[r] = jj - t * kin;
    dzr[r] = dzs + (size_t)(t < Hs ? t : Hs - 1) * a.wmax;
  }
  __syncthreads();
  for (int l = 1; l < nl; ++l) {
    const int in = md->dims[l], out = md->dims[l + 1];
    const double* W = md->w[l];
    const double* bin = ((l + 1) & 1) ? buf1 : buf0;
    double* bout = (l & 1) ? buf1 : buf0;
    const int ct = (out + 15) / 16;
    const int ntw = w < ct ? (ct - w + kKmWaves - 1) / kKmWaves : 0;     // this wave's tiles (wave-uniform)
    if (l + 1 < nl) {
      const double* dl[4] = {dzr[0] + l * lstride, dzr[1] + l * lstride, dzr[2] + l * lstride, dzr[3] + l * lstride};
      switch (ntw) {
        case 1: it_tangent<1>(W, in, out, bin, bout, w, lane, dl); break;
        case 2: it_tangent<2>(W, in, out, bin, bout, w, lane, dl); break;
        case 3: it_tangent<3>(W, in, out, bin, bout, w, lane, dl); break;
        case 4: it_tangent<4>(W, in, out, bin, bout, w, lane, dl); break;
        default: break;
      }
      __syncthreads();
    } else if (ntw == 1) {
      // the output layer (one tile per wave): J[(t, c)][io] = (T W_out')[io] dy_std[io] + [io == c]
      d4 acc[1];
      it_mma<1>(acc, W, in, out, bin, w, lane);
      const int io = 16 * w + i;
      if (io < out) {
        const double ds = md->norm[3][io];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (rt[r] < 0) continue;
          const int c = rc[r];
          const double v = acc[0][r] * ds + (io == c ? 1.0 : 0.0);
          const size_t so = (size_t)slot * a.H + rt[r];
          if (c < nx) a.jx[(so * nx + io) * nx + c] = v;
          else a.ju[(so * nx + io) * nu + (c - nx)] = v;
        }
      }
    }
  }
}

}  // namespace ampc
