// mppi_table_kernels.hpp -- the MPPI rollout of a plan whose problems run on MLP models of any mix of depth, widths
// and activation (ampc_mppi_plan_set_model_table; gfx950, f64 only): the contract of mppi_rollout_kernel
// (mppi_kernels.hpp: costs[cost_off + n], term_last[p], term_mode 0 / 1, the fused-update partials or eps_out) on the
// model step of kstep_mlp_kernels.hpp, which reads plain nn.Linear parameters through a device table.
//
// Geometry, the same for every model: one workgroup = 256 threads = four waves owns 16 samples of one problem for all H
// steps.  The tile's problem is args.tile_prob[blockIdx.x], its model models[pr.model], read field by field through the
// pointer (wave-uniform loads; no by-value copy of the entry: kstep_mlp_kernels.hpp).
//
// Step (mppi.py:110-152 with MLP.pred_batch, mlp.py:229-236, unfolded), thread (m = tid / 16, r = tid % 16):
//   A = clip(eps + a) by comparison (a NaN poisons the sample);  eps <- A - a;  u = A scale;  ca += A eps   thread (m, j)
//   c += stage cost of (x_t, u_t): diagonal fast path where the values are produced, else dense Q / R / F rows
//        r, r + 16, ... of sample m, plus the affine part of a sum of quadratics
//   in = ([x, u] - xu_mean) / xu_std;  a_{l+1} = act(a_l W_l' + b_l);  x' = x + (z dy_std + dy_mean)
// The layers are km_fetch_group / km_mma_group of kstep_mlp_kernels.hpp (v_mfma_f64_16x16x4_f64 over 16-column output
// tiles, wave w takes the tiles w, w + 4, ..., weights from global memory / L2) with that file's padding rules:
// reduction indices >= in are selected to exact zeros, weight rows >= out land in columns stored as 0.  The output
// layer (one tile per wave) has its own epilogue here: the state update in LDS.
//
// LDS (doubles), fixed per plan by (nx, nu, horizon cap, cost stride) -- never by the models:
//   act[2][16][257]   the two activation buffers (kstep_mlp_kernels.hpp); the normalised input goes into act[1]
//   xu[16][81]        the raw [x | u] rows (odd stride)
//   norm[288]         xu_mean[80] xu_std[80] dy_mean[64] dy_std[64]                      -- kMtOffExtra = 9808 doubles
//   cost block + lo hi scale, the shifted sequence [max_h][nu], then -- fused update, where it fits the 160 KB --
//   the tile's clipped noise [max_h][16][nu] and [32] reduction slots (ampc_mppi_plan: lds_cost, lds_aseq, lds_eps, lds_red)
//
// Sums.  An output element accumulates over k in blocks of 16 in order, inside a block as the MFMA does: a function of
// the layer's own `in`.  A sample's cost: each of its 16 threads adds its terms in step order, the 16 partials meet in
// a butterfly of shuffles; the tile's partials add its 16 rows in order; mppi_combine_kernel / mppi_update_kernel add
// tiles / samples in their own fixed order.  All of it is a function of the model's widths, N, H, nu and the 16-row
// tile; no atomics.  A candidate's controls are the same bits alone, in any batch, at any position, from run to run.
#pragma once
#include "mppi_kernels.hpp"
#define AMPC_KM_LAYERS_ONLY          // the layer routines and the table entry, not the k-step kernel
#include "kstep_mlp_kernels.hpp"

namespace ampc {

constexpr int kMtRows = kKmRows;              // samples per workgroup
constexpr int kMtThreads = kKmThreads;
constexpr int kMtTps = kMtThreads / kMtRows;  // threads per sample: 16, a quarter wave
constexpr int kMtXuStride = kKmMaxIn + 1;
static_assert(kMtTps == 16 && kMaxNu <= kMtTps, "thread (m, j) owns control j of sample m");
// LDS map, in doubles
constexpr int kMtOffAct = 0;
constexpr int kMtOffXu = 2 * kMtRows * kKmActStride;
constexpr int kMtOffNorm = kMtOffXu + kMtRows * kMtXuStride;
constexpr int kMtOffExtra = (kMtOffNorm + 2 * kKmMaxIn + 2 * kKmMaxOut + 3) / 4 * 4;

// One layer for the NT tiles w, w + 4, ... of wave w: bout = act(bin W' + b), or -- last -- xu[:, c] += z dy_std + dy_mean.
template <int NT>
__device__ __forceinline__ void mt_layer(const double* __restrict__ W, const double* __restrict__ B, int in, int out,
                                         int act, bool last, const double* bin, double* bout, int w, int lane,
                                         double* xu, const double* norm) {
  const int i = lane & 15, q = lane >> 4;
  int roff[NT], col[NT];
  double bias[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    col[t] = 16 * (w + kKmWaves * t) + i;
    const int wr = col[t] < out ? col[t] : out - 1;
    roff[t] = wr * in;
    bias[t] = B[wr];
  }
  d4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
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
  // accumulator register r of lane (i, q): row q + 4 r, column col[t]
  if (!last) {
    // (z first, the activation in place one column tile at a time: kstep_mlp_kernels.hpp, km_layer)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) bout[(q + 4 * r) * kKmActStride + col[t]] = acc[t][r] + bias[t];
#pragma unroll 1
    for (int t = 0; t < NT; ++t) {
      const int c = 16 * (w + kKmWaves * t) + i;
      double* p = bout + q * kKmActStride + c;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double v = act_apply<double>(act, p[4 * r * kKmActStride]);
        p[4 * r * kKmActStride] = c < out ? v : 0.0;
      }
    }
    return;
  }
  // (the output layer has at most kKmMaxOut / 16 = 4 tiles: one per wave)
  if constexpr (NT == 1) {
    const int c = col[0];
    if (c >= out) return;
    const double dm = norm[2 * kKmMaxIn + c], ds = norm[2 * kKmMaxIn + kKmMaxOut + c];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double* x = xu + (q + 4 * r) * kMtXuStride + c;
      *x = *x + ((acc[0][r] + bias[0]) * ds + dm);
    }
  }
}

__global__ __launch_bounds__(kMtThreads) void mppi_rollout_table_kernel(const KstepMlpModel* __restrict__ models,
                                                                        const MppiArgs<double> args) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  double* lds = reinterpret_cast<double*>(smem_raw);
  constexpr int M = kMtRows, NTHR = kMtThreads, TPS = kMtTps;
  const int tile = blockIdx.x;
  const int p = args.tile_prob[tile];
  const MppiProblem<double> pr = args.probs[p];
  const KstepMlpModel* md = models + pr.model;
  const int nl = md->n_layers, act = md->act;
  const int nx = args.mlp.nx, nu = args.mlp.nu, kin = nx + nu, no = args.obs_dim;     // (no == nx: checked by the host)
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool diag = args.cost_diag != 0, affine = args.cost_affine != 0;
  const int cost_stride = args.cost_stride;
  const int first = (tile - pr.tile0) * M;
  const int H = pr.H, N = pr.N;

  double* buf0 = lds + kMtOffAct;
  double* buf1 = buf0 + M * kKmActStride;
  double* xu = lds + kMtOffXu;
  double* norm = lds + kMtOffNorm;
  double* aseq = lds + args.lds_aseq;    // [H][nu] shifted warm start
  double* cpar = lds + args.lds_cost;    // Q R F goal lin lint c0 c1 | lo hi scale
  const double* Qm = cpar;
  const double* Rm = Qm + no * no;
  const double* Fm = Rm + nu * nu;
  const double* goal = Fm + no * no;
  const double* lin = goal + no;
  const double* lint = lin + no;
  const double* blo = cpar + cost_stride;
  const double* bhi = blo + nu;
  const double* bsc = bhi + nu;

  // ---- prologue: constants, shifted sequence, initial state ----------------------------------------
  for (int i = tid; i < kin; i += NTHR) {
    norm[i] = md->norm[0][i];
    norm[kKmMaxIn + i] = md->norm[1][i];
  }
  for (int i = tid; i < nx; i += NTHR) {
    norm[2 * kKmMaxIn + i] = md->norm[2][i];
    norm[2 * kKmMaxIn + kKmMaxOut + i] = md->norm[3][i];
  }
  for (int i = tid; i < cost_stride; i += NTHR) cpar[i] = args.costs_par[(size_t)pr.cost_idx * cost_stride + i];
  for (int i = tid; i < 3 * nu; i += NTHR) cpar[cost_stride + i] = args.bounds[i];
  for (int i = tid; i < H * nu; i += NTHR) {
    const int t = i / nu, j = i - t * nu;
    const int ts = (t + 1 < H) ? t + 1 : H - 1;  // a[:-1] = a[1:]; a[-1] = a[-2]
    aseq[i] = args.act_in[pr.a_off + ts * nu + j];
  }
  const int m = tid / TPS, r = tid % TPS;   // sample-in-tile, helper index (= the control this thread owns)
  const int n = first + m;
  const bool valid = n < N;
  const double* eps_row = args.eps + pr.eps_off + (size_t)(valid ? n : 0) * H * nu;
  double* epso = args.eps_out + pr.epso_off;
  double* xrow = xu + m * kMtXuStride;
  double c_part = 0.0, ca_part = 0.0;
  double e_next = (valid && r < nu) ? eps_row[r] : 0.0;
  for (int c = r; c < nx; c += TPS) xrow[c] = args.x0[p * nx + c];
  __syncthreads();

  // actions of step t (mppi.py:134-139), thread (m, j = r)
  auto actions = [&](int t) {
    if (r < nu) {
      const double a = aseq[t * nu + r];
      double A = e_next + a;
      A = A < blo[r] ? blo[r] : A;           // by comparison: a NaN stays a NaN (mppi_kernels.hpp)
      A = A > bhi[r] ? bhi[r] : A;
      const double ec = A - a;
      if (valid && args.write_eps_out) epso[((size_t)t * N + n) * nu + r] = ec;
      if (args.lds_eps >= 0) lds[args.lds_eps + (t * M + m) * nu + r] = ec;
      ca_part += A * ec;
      const double u = A * bsc[r];
      xrow[nx + r] = u;
      if (diag) c_part += Rm[r * nu + r] * u * u;
      if (t + 1 < H) e_next = valid ? eps_row[(t + 1) * nu + r] : 0.0;
    }
  };
  actions(0);
  if (diag) c_part += quad_rows<double>(Qm, xrow, goal, no, r, TPS, true);        // stage cost of x_0
  if (affine) {
    if (diag) c_part += affine_rows<double>(lin, xrow, goal, no, r, TPS, 0.0);
    if (r == 0) c_part += (double)H * lint[no];                                   // c0, for the H stage costs at once
  }
  __syncthreads();

  for (int t = 0; t < H; ++t) {
    // ---- stage cost of (x_t, u_t), dense blocks --------------------------------------------------
    if (!diag) {
      c_part += quad_rows<double>(Qm, xrow, goal, no, r, TPS, false);
      c_part += quad_rows<double>(Rm, xrow + nx, nullptr, nu, r, TPS, false);
      if (affine) c_part += affine_rows<double>(lin, xrow, goal, no, r, TPS, 0.0);
    }
    // ---- dynamics --------------------------------------------------------------------------------
    for (int c = r; c < kin; c += TPS) buf1[m * kKmActStride + c] = (xrow[c] - norm[c]) / norm[kKmMaxIn + c];
    __syncthreads();
    // the next step's actions do not depend on this step's output; the control columns of xu are read again only
    // behind the layers' barriers
    if (t + 1 < H) actions(t + 1);
    for (int l = 0; l < nl; ++l) {
      const int in = md->dims[l], out = md->dims[l + 1];
      const double* W = md->w[l];
      const double* B = md->b[l];
      const double* bin = ((l + 1) & 1) ? buf1 : buf0;
      double* bout = (l & 1) ? buf1 : buf0;
      const bool last = l == nl - 1;
      const int ct = (out + 15) / 16;
      const int ntw = w < ct ? (ct - w + kKmWaves - 1) / kKmWaves : 0;     // this wave's tiles (wave-uniform)
      static_assert(kKmMaxTiles == 4, "one case per tile count");
      switch (ntw) {
        case 1: mt_layer<1>(W, B, in, out, act, last, bin, bout, w, lane, xu, norm); break;
        case 2: mt_layer<2>(W, B, in, out, act, last, bin, bout, w, lane, xu, norm); break;
        case 3: mt_layer<3>(W, B, in, out, act, last, bin, bout, w, lane, xu, norm); break;
        case 4: mt_layer<4>(W, B, in, out, act, last, bin, bout, w, lane, xu, norm); break;
        default: break;
      }
      __syncthreads();
    }
    // stage cost of x_{t+1}, diagonal blocks (x_H only pays the terminal cost)
    if (diag && t + 1 < H)
      for (int i = r; i < no; i += TPS) {
        const double d = xrow[i] - goal[i];
        c_part += (Qm[i * no + i] * d + lin[i]) * d;
      }
  }

  // ---- epilogue: terminal cost, reduce the 16 partials, write (mppi_kernels.hpp) ------------------------
  double term = quad_rows<double>(Fm, xrow, goal, no, r, TPS, diag);
  if (affine) term += affine_rows<double>(lint, xrow, goal, no, r, TPS, lint[no + 1]);
  double c = c_part + pr.lam_over_sigma * ca_part;
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

  // ---- fused softmin update, tile part: the tile publishes its minimum, sum_m S_m and sum_m S_m eps[t][m][j];
  // an all-inf tile publishes zero sums (the dead-tile rule of mppi_rollout_kernel)
  double* cred = lds + args.lds_red;
  double* sred = cred + M;
  if (r == 0) cred[m] = valid ? c : (double)INFINITY;
  __syncthreads();
  double mw = cred[0];
  for (int i = 1; i < M; ++i) mw = cred[i] < mw ? cred[i] : mw;
  const bool dead_tile = !(mw < (double)INFINITY);
  if (tid < M) sred[tid] = (first + tid < N && !dead_tile) ? exp(pr.neg_inv_lambda * (cred[tid] - mw)) : 0.0;
  __syncthreads();
  const double* el = lds + args.lds_eps;
  double* tp = args.tile_part + (size_t)tile * args.hnu_stride;
  for (int e = tid; e < H * nu; e += NTHR) {
    const int t = e / nu, j = e - t * nu;
    double s = 0.0;
    for (int i = 0; i < M; ++i) s += sred[i] * el[(t * M + i) * nu + j];
    tp[e] = s;
  }
  if (tid == 0) {
    double ss = 0.0;
    for (int i = 0; i < M; ++i) ss += sred[i];
    args.tile_stat[2 * tile] = mw;
    args.tile_stat[2 * tile + 1] = ss;
  }
}

}  // namespace ampc
