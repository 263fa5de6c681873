// kstep_sindy_kernels.hpp -- k-step prediction error of SINDy models over recorded trajectories (gfx950): the
// contract of kstep_error_kernel (kstep_kernels.hpp: one rollout of kmax steps per start point yields the error sums
// of every horizon 1..kmax) on the per-thread model step of sindy_kernels.hpp.
//
// Layout.  A row is one start point (row_base / row_rem as in kstep_kernels.hpp).  Grid (row tiles, models): a
// workgroup is ONE wave, a thread owns one row of ONE model.  State | control, the next state and the feature table
// live in LDS columns [i][lane] (conflict-free), as in mppi_rollout_sindy_kernel.  Step j loads control row
// base + j - 1 into the control columns, runs sindy_step and forms, in f64 from the model-precision state with the
// dimensions summed in order,
//   sq  = sum_d (x_d - obs[base + j]_d)^2
//   dsq = sum_d (((x_d - x_prev_d) - (obs[base + j]_d - obs[base + j - 1]_d)) * inv_std_d)^2      (optional: RMSMENS)
// (x_prev is still in the state columns while the step's result sits in the next-state columns).  The row's sums of
// kKsChunk consecutive steps are kept in an LDS block [step][lane]; when it is full, lane q sums step q's rows in row
// order and writes the per-tile partial part[m][tile][j]: the chunk's horizons are summed side by side, and the
// rollout is not interrupted once per step.
//
// Models of different libraries, coefficient sparsity and time_mode share a launch: the workgroup reads its model's
// SindyDev from a table in global memory, field by field through the pointer (uniform loads; a by-value descriptor
// array indexed by blockIdx is demoted to scratch, see kstep_kernels.hpp).  A program that fits kSindyStageBytes is
// copied to LDS first (sindy_stage; every pointer of the staged descriptor is an LDS pointer), larger programs and
// the direct-evaluation form (n_tab == 0) run from global memory as in sindy_forward_kernel.  Every LDS offset
// depends on the model's OWN sizes only; the launch reserves the bytes of the largest model.
//
// Masking.  Rows with j > rem keep running with control / observation indices clamped into their own trajectory;
// their error is dropped by a SELECT, never multiplied by 0.  Rows past n_rows behave as rows with rem = 0.  No index
// depends on a state value: a diverging rollout yields non-finite sums, nothing else.
//
// Determinism.  No atomics.  A row's error is summed over d in order, the tile's 64 rows in order by one lane, the
// per-tile partials over tiles in order by kstep_reduce_kernel.  A model's sums are the same bits alone, in any
// batch, in any position of it, and from run to run.
#pragma once
#include "kstep_kernels.hpp"
#include "sindy_kernels.hpp"

namespace ampc {

constexpr int kKsRows = 64;          // rows of a tile = threads of the workgroup (one wave)
constexpr int kKsChunk = 8;          // steps whose row errors are kept before they are summed
constexpr int kKsErrStride = 65;     // doubles per step of the error block: 64 rows + 1 pad (2 banks apart)

struct KstepSindyArgs {
  const double* obs;          // [total][nx]
  const double* ctrls;        // [total][nu]
  const double* inv_std;      // [nx] (only read when dpart != nullptr)
  const int* row_base;        // [n_rows]
  const int* row_rem;         // [n_rows]
  double* part;               // [n_models][tiles][kmax]
  double* dpart;              // same, delta errors; nullptr: not asked for
  int n_rows, tiles, kmax;
};

// LDS of one model: the columns [2 nx + nu + n_tab][64] in the model precision, the error block(s) in f64, then the
// staged program (stage_bytes: sindy_stage_bytes of the handle, 0 when it runs from global memory)
__host__ __device__ constexpr size_t kstep_sindy_col_elems(int nx, int nu, int n_tab) {
  return (size_t)(2 * nx + nu + n_tab) * kKsRows;
}
__host__ __device__ constexpr size_t kstep_sindy_err_doubles(bool delta) {
  return (size_t)(delta ? 2 : 1) * kKsChunk * kKsErrStride;
}
__host__ __device__ constexpr size_t kstep_sindy_lds_bytes(int nx, int nu, int n_tab, bool delta, size_t stage_bytes,
                                                           int esz) {
  return kstep_sindy_col_elems(nx, nu, n_tab) * esz + kstep_sindy_err_doubles(delta) * 8 + stage_bytes;
}

// the rollout of one tile with the model descriptor `m` (staged or global)
template <typename T>
__device__ __forceinline__ void kstep_sindy_rollout(const SindyDev<T>& m, const KstepSindyArgs& a, T* lds,
                                                    double* es, double* des) {
  constexpr int BS = kKsRows;
  const int lane = threadIdx.x, nx = m.nx, nu = m.nu, nv = nx + nu;
  const bool want_d = a.dpart != nullptr;
  const int tile = blockIdx.x, gr = tile * BS + lane;
  const bool live = gr < a.n_rows;
  const long long b = live ? a.row_base[gr] : 0;
  const int rem = live ? a.row_rem[gr] : 0;
  T* v = lds + lane;                        // [nv][BS]  x | u
  T* o = lds + nv * BS + lane;              // [nx][BS]  next state
  T* tr = lds + (nv + nx) * BS + lane;      // [n_tab][BS]  per-thread table
  for (int i = 0; i < nx; ++i) v[i * BS] = (T)a.obs[b * nx + i];
  const size_t pbase = ((size_t)blockIdx.y * a.tiles + tile) * a.kmax;
  for (int j = 1; j <= a.kmax; ++j) {
    const int k = j < rem ? j : rem;                                 // clamped: never past the trajectory
    const long long oc = b + k, op = b + (k > 0 ? k - 1 : 0);
    for (int q = 0; q < nu; ++q) v[(nx + q) * BS] = (T)a.ctrls[op * nu + q];
    sindy_step<T>(m, v, BS, o, BS, tr, BS);
    double s = 0.0, ds = 0.0;
    for (int i = 0; i < nx; ++i) {
      const T xn = o[i * BS];
      const double ob = a.obs[oc * nx + i];
      const double e = (double)xn - ob;
      s += e * e;
      if (want_d) {
        const double dd = (((double)xn - (double)v[i * BS]) - (ob - a.obs[op * nx + i])) * a.inv_std[i];
        ds += dd * dd;
      }
      v[i * BS] = xn;
    }
    const bool counted = j <= rem;
    const int slot = (j - 1) % kKsChunk;
    es[slot * kKsErrStride + lane] = counted ? s : 0.0;
    if (want_d) des[slot * kKsErrStride + lane] = counted ? ds : 0.0;
    if (slot == kKsChunk - 1 || j == a.kmax) {
      __syncthreads();
      if (lane <= slot) {                                            // lane q: step j - slot + q, rows in order
        const size_t pj = pbase + (size_t)(j - 1 - slot + lane);
        double ts = 0.0;
        for (int r = 0; r < BS; ++r) ts += es[lane * kKsErrStride + r];
        a.part[pj] = ts;
        if (want_d) {
          double tds = 0.0;
          for (int r = 0; r < BS; ++r) tds += des[lane * kKsErrStride + r];
          a.dpart[pj] = tds;
        }
      }
      __syncthreads();
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kKsRows) void kstep_sindy_kernel(const SindyDev<T>* __restrict__ descs,
                                                              const KstepSindyArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* lds = reinterpret_cast<T*>(smem_raw);
  const SindyDev<T>* d = descs + blockIdx.y;
  SindyDev<T> g;
  g.nx = d->nx; g.nu = d->nu; g.n_feat = d->n_feat; g.continuous = d->continuous; g.strict = d->strict;
  g.dt = d->dt;
  g.kind = d->kind; g.a0 = d->a0; g.a1 = d->a1; g.par = d->par; g.xi = d->xi;
  g.n_trig = d->n_trig; g.n_pow = d->n_pow; g.n_tab = d->n_tab; g.n_mon = d->n_mon; g.n_pool = d->n_pool;
  g.moff = d->moff; g.mcnt = d->mcnt; g.mpool = d->mpool; g.fx = d->fx; g.fy = d->fy;
  g.tvar = d->tvar; g.tpar = d->tpar; g.pvar = d->pvar; g.ppar = d->ppar;
  g.stage = d->stage;
  const bool want_d = a.dpart != nullptr;
  // (the column block is a multiple of 64 elements: the error block behind it is 8-byte aligned in either precision)
  double* es = reinterpret_cast<double*>(lds + kstep_sindy_col_elems(g.nx, g.nu, g.n_tab));
  double* des = es + kKsChunk * kKsErrStride;
  T* area = reinterpret_cast<T*>(es + kstep_sindy_err_doubles(want_d));
  if (g.stage) {
    const SindyDev<T> m = sindy_stage<T, true>(g, area, threadIdx.x, kKsRows);
    kstep_sindy_rollout<T>(m, a, lds, es, des);
  } else {
    kstep_sindy_rollout<T>(g, a, lds, es, des);
  }
}

}  // namespace ampc
