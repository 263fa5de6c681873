// lqr_kernels.hpp -- discrete LQR in f64, finite and infinite horizon (reference: autompc/control/lqr.py:15-47,
// 96-192).
//
// lqr_gains_kernel: one workgroup per Riccati problem, problems of different state dimension in one launch.
// Each problem runs the reference's recursion from P = F (padded to the model state):
//     M = P [A | B]                           (n x (n+nu))
//     G = [A | B]^T M                         ((n+nu) x (n+nu)): G_AA = A^T P A, G_AB = A^T P B (upper right),
//                                             G_BA = B^T P A (lower left), G_BB = B^T P B
//     X = (R + G_BB)^-1 G_BA                  (Gauss-Jordan with partial pivoting, nu <= 16, in LDS)
//     P <- (G_AA - G_AB X) + Q
// horizon + 1 times, and returns K = -X of the last P.  An infinite-horizon problem (horizon 0) runs the same update
// from P = Q until max|P_new - P_old| <= threshold (_inf_horz_dt_lqr, lqr.py:22-33) or max_iter updates have run; the
// maximum is taken where the update stores P (each lane reads the entry it is about to overwrite) and reduced over
// the wave and then the four waves, and a maximum does not depend on the order it is taken in.
// Nothing is assumed symmetric: Q, F and R are taken as
// given, as the reference takes them, and P is then not symmetric either.  The workspace holds P TRANSPOSED
// (Pt[k][i] = P[i][k]), so lqr_gemm_tn's X^T Y with X = Pt is P [A | B] with every load of the product
// coalesced; the update transposes 8 x 8 blocks between the lanes of a wave, so it loads and stores runs of 8.
// Every entry of every product is ONE thread's sequential sum over k = 0 .. K-1, so the result of
// a problem does not depend on which other problems share the launch or on their order.
//
// lqr_ctrl_kernel / lqr_record_kernel: one control step of the closed loop (FiniteHorizonLQR.run,
// lqr.py:174-192, driven by simulate(), utils/simulation.py:44-63).
#ifndef AMPC_LQR_KERNELS_HPP
#define AMPC_LQR_KERNELS_HPP
#include <hip/hip_runtime.h>

namespace ampc {

constexpr int kLqrMaxN = 256, kLqrMaxNu = 16;
constexpr int kLqrThreads = 256;
constexpr int kLqrTile = 64, kLqrKt = 16;
static_assert(kLqrThreads % 64 == 0, "the update of P hands values between the lanes of whole 64-lane waves");

// One Riccati problem.  Read field by field through a global pointer (uniform, scalar loads): a copy of the
// struct in registers indexed at run time is what spilled the plans' model table to scratch.
struct LqrDesc {
  int n, nu, no, horizon;     // horizon 0: iterate to the fixed point (threshold, max_iter)
  int id, max_iter, pad1, pad2;
  const double* ab;           // [n][n + nu] row-major: [A | B] of the controller model
  long long ws;               // workspace offset (doubles): P [n][n], M [n][n+nu], G [n+nu][n+nu]
  long long cost;             // cost offset (doubles): Q [no][no], R [nu][nu], F [no][no]
  long long k;                // gain offset (doubles): K [nu][n]
  double threshold;           // infinite horizon: stop once max|P_new - P_old| <= threshold
};

// max of two magnitudes in which a NaN sticks, whichever side it is on (so the order does not matter)
__device__ inline double lqr_nanmax(double a, double b) { return (b > a || b != b) ? b : a; }

// C[i][j] = sum_k X[k][i] Y[k][j]  (i < m, j < nn, k < K); X, Y, C row-major with leading dimensions
// ldx, ldy, ldc.  64 x 64 output tiles, 16-deep k slices staged in LDS, a 4 x 4 register block per thread.
__device__ inline void lqr_gemm_tn(const double* __restrict__ X, int ldx, const double* __restrict__ Y, int ldy,
                                   double* __restrict__ C, int ldc, int m, int nn, int K, double* lds) {
  double* xs = lds;
  double* ys = lds + kLqrKt * kLqrTile;
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  for (int i0 = 0; i0 < m; i0 += kLqrTile)
    for (int j0 = 0; j0 < nn; j0 += kLqrTile) {
      double acc[4][4];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0.0;
      for (int k0 = 0; k0 < K; k0 += kLqrKt) {
        for (int e = t; e < kLqrKt * kLqrTile; e += kLqrThreads) {
          const int kk = e >> 6, c = e & 63, k = k0 + kk;
          xs[e] = (k < K && i0 + c < m) ? X[(size_t)k * ldx + i0 + c] : 0.0;
          ys[e] = (k < K && j0 + c < nn) ? Y[(size_t)k * ldy + j0 + c] : 0.0;
        }
        __syncthreads();
        const int kn = K - k0 < kLqrKt ? K - k0 : kLqrKt;
        for (int kk = 0; kk < kn; ++kk) {
          double a[4], b[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) a[r] = xs[kk * kLqrTile + ty + 16 * r];
#pragma unroll
          for (int c = 0; c < 4; ++c) b[c] = ys[kk * kLqrTile + tx + 16 * c];
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[r][c] = fma(a[r], b[c], acc[r][c]);
        }
        __syncthreads();
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + ty + 16 * r;
        if (i >= m) continue;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int j = j0 + tx + 16 * c;
          if (j < nn) C[(size_t)i * ldc + j] = acc[r][c];
        }
      }
    }
}

// The body of lqr_gains_kernel, instantiated once per kind of problem: with inf == false every infinite-horizon
// statement folds away and what is left is the finite recursion as it was before those existed.
template <bool inf>
__device__ __forceinline__ void lqr_gains_body(const LqrDesc* __restrict__ d, double* __restrict__ ws,
                                               const double* __restrict__ cost, double* __restrict__ kout,
                                               int* __restrict__ status, double* tiles, double* aug, double* fac,
                                               double* s_red, int& s_piv, int& s_bad, int& s_conv) {
  const int n = d->n, nu = d->nu, no = d->no, H = d->horizon, id = d->id;
  const double* __restrict__ ab = d->ab;
  const int m = n + nu, w = nu + n;          // w: width of the augmented system [S | G_BA]
  double* Pt = ws + d->ws;                   // P transposed: Pt[k][i] = P[i][k]
  double* M = Pt + (size_t)n * n;
  double* G = M + (size_t)n * m;
  const double* Q = cost + d->cost;
  const double* R = Q + (size_t)no * no;
  const double* F = R + (size_t)nu * nu;
  double* K = kout + d->k;
  const int t = threadIdx.x;
  const double* P0 = inf ? Q : F;            // _inf_horz_dt_lqr starts from P = Q (lqr.py:23)
  for (int e = t; e < n * n; e += kLqrThreads) {
    const int i = e / n, j = e - i * n;
    Pt[e] = (i < no && j < no) ? P0[j * no + i] : 0.0;
  }
  if (t == 0) s_bad = s_conv = 0;
  __syncthreads();
  int it = 0;                                // Riccati updates performed so far
  // finite: H + 1 Riccati updates (lqr.py:36-40), then the gain (:42); infinite: updates until P stands still
  // (:24-29), then the gain (:31)
  for (;; ++it) {
    lqr_gemm_tn(Pt, n, ab, m, M, m, n, m, n, tiles);
    __syncthreads();
    lqr_gemm_tn(ab, m, M, m, G, m, m, m, n, tiles);
    __syncthreads();
    for (int e = t; e < nu * w; e += kLqrThreads) {
      const int r = e / w, c = e - r * w;
      aug[r * w + c] = c < nu ? R[r * nu + c] + G[(size_t)(n + r) * m + n + c] : G[(size_t)(n + r) * m + c - nu];
    }
    __syncthreads();
    for (int c = 0; c < nu; ++c) {
      if (t == 0) {                          // pivot: first row of largest magnitude (fixed order)
        int p = c;
        double best = fabs(aug[c * w + c]);
        for (int r = c + 1; r < nu; ++r) {
          const double v = fabs(aug[r * w + c]);
          if (v > best) { best = v; p = r; }
        }
        s_piv = p;
        if (!(best > 0.0) || !isfinite(best)) s_bad = 1;
      }
      __syncthreads();
      if (s_bad) break;
      const int p = s_piv;
      if (p != c)
        for (int j = c + t; j < w; j += kLqrThreads) {
          const double v = aug[c * w + j];
          aug[c * w + j] = aug[p * w + j];
          aug[p * w + j] = v;
        }
      __syncthreads();
      const double piv = aug[c * w + c];
      __syncthreads();
      for (int j = c + 1 + t; j < w; j += kLqrThreads) aug[c * w + j] /= piv;
      if (t < nu) fac[t] = aug[t * w + c];
      __syncthreads();
      for (int e = t; e < nu * (w - c - 1); e += kLqrThreads) {
        const int r = e / (w - c - 1), j = c + 1 + (e - r * (w - c - 1));
        if (r != c) aug[r * w + j] = fma(-fac[r], aug[c * w + j], aug[r * w + j]);
      }
      __syncthreads();
    }
    if (s_bad) break;
    if (inf ? s_conv : it == H + 1) {        // K = -(R + B^T P B)^-1 B^T P A
      for (int e = t; e < nu * n; e += kLqrThreads) {
        const int r = e / n, j = e - r * n;
        const double v = -aug[r * w + nu + j];
        K[e] = v;
        if (!isfinite(v)) s_bad = 1;
      }
      break;
    }
    // P[i][j] = (G_AA[i][j] - sum_r G_AB[i][r] X[r][j]) + Q[i][j] in 8 x 8 blocks, one per wave at a time: lane
    // (a, b) computes P[i0 + a][j0 + b] along rows of G, X and Q, takes P[i0 + b][j0 + a] from lane (b, a) and
    // stores it to Pt[j0 + a][i0 + b]: loads and stores both run over 8 consecutive doubles, with no barrier
    {
      const int lane = t & 63, a = lane >> 3, b = lane & 7, nb = (n + 7) >> 3;
      double dm = 0.0;                         // this lane's max|P_new - P_old| (a masked-off lane adds nothing)
      for (int blk = t >> 6; blk < nb * nb; blk += kLqrThreads / 64) {   // (uniform in the wave)
        const int bi = blk / nb, i0 = 8 * bi, j0 = 8 * (blk - bi * nb);
        const int i = i0 + a, j = j0 + b;
        double v = 0.0;
        if (i < n && j < n) {
          double y = 0.0;
          for (int r = 0; r < nu; ++r) y = fma(G[(size_t)i * m + n + r], aug[r * w + nu + j], y);
          const double q = (i < no && j < no) ? Q[i * no + j] : 0.0;
          v = (G[(size_t)i * m + j] - y) + q;
        }
        v = __shfl(v, 8 * b + a);              // every lane of the wave takes part
        if (i0 + b < n && j0 + a < n) {
          double* dst = Pt + (size_t)(j0 + a) * n + i0 + b;
          if (inf) dm = lqr_nanmax(dm, fabs(v - *dst));
          *dst = v;
        }
      }
      if (inf) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) dm = lqr_nanmax(dm, __shfl_xor(dm, off));
        if (lane == 0) s_red[t >> 6] = dm;
      }
    }
    __syncthreads();
    if (inf) {
      double dm = s_red[0];
#pragma unroll
      for (int wv = 1; wv < kLqrThreads / 64; ++wv) dm = lqr_nanmax(dm, s_red[wv]);
      if (dm != dm) {                          // NaN: the reference's loop ends on it and returns a NaN gain
        if (t == 0) s_bad = 1;
        ++it;
        break;
      }
      if (dm <= d->threshold) {                // (read here, once a step: nothing more to keep in registers)
        if (t == 0) s_conv = 1;                // read after the next pass's barriers
      } else if (it + 1 >= d->max_iter) {      // still moving at the cap
        if (t == 0) s_bad = 2;
        ++it;
        break;
      }
    }
  }
  __syncthreads();
  if (t == 0) {
    status[id] = s_bad;
    status[gridDim.x + id] = inf ? it : H + 1;
  }
  if (s_bad)
    for (int e = t; e < nu * n; e += kLqrThreads) K[e] = __builtin_nan("");
}

// Problems are launched in `order` (heaviest first, so a horizon-1000 problem starts at once);
// status[id] = 0 ok, 1 singular R + B^T P B or a non-finite value (the reference's LinAlgError / NaN), 2 an
// infinite-horizon problem whose P still moved by more than its threshold after max_iter updates (the reference's
// loop would not return).  status [2 * gridDim.x]: the second half takes the Riccati updates performed, horizon + 1 of
// a finite problem (one array, and the convergence flag in LDS: the products leave no scalar register to spare).
__global__ __launch_bounds__(kLqrThreads) void lqr_gains_kernel(const LqrDesc* __restrict__ descs,
                                                                 const int* __restrict__ order,
                                                                 double* __restrict__ ws,
                                                                 const double* __restrict__ cost,
                                                                 double* __restrict__ kout, int* __restrict__ status) {
  __shared__ double tiles[2 * kLqrKt * kLqrTile];
  __shared__ double aug[kLqrMaxNu * (kLqrMaxNu + kLqrMaxN)];
  __shared__ double fac[kLqrMaxNu];
  __shared__ double s_red[kLqrThreads / 64];
  __shared__ int s_piv, s_bad, s_conv;
  const LqrDesc* d = descs + order[blockIdx.x];
  if (d->horizon == 0)
    lqr_gains_body<true>(d, ws, cost, kout, status, tiles, aug, fac, s_red, s_piv, s_bad, s_conv);
  else
    lqr_gains_body<false>(d, ws, cost, kout, status, tiles, aug, fac, s_red, s_piv, s_bad, s_conv);
}

// One candidate of the closed loop.
struct LqrLoopDesc {
  int n, rule, n_basis, noclip;  // noclip 1: u = K (s - state0) as it is (InfiniteHorizonLQR.run, lqr.py:126-136)
                               // rule 0: state = observation, 1: ARX shift A s + B u then the observation
                               // slot overwritten (arx.py:94-99), 2: lift (koopman.py:105-122, 166-168)
  const double* ab;            // [n][n + nu]
  long long s;                 // state offset (doubles): two buffers of n, alternating per step
  long long k;                 // gain offset: K [nu][n]
  long long goal;              // goal offset: [no] (state0 = goal zero-padded to n, lqr.py:177-182)
  long long lift;              // lift program offset: (kind, parameter) pairs, mppi_kernels.hpp: state_lift_kernel
};

// Controller step of every candidate (one workgroup each): modelstate = update_state(state, u_prev, obs),
// u = clip(K (modelstate - state0)), not clipped where the problem's descriptor says so.  sim [B][snx]: the
// surrogate state, whose first `no` entries are the observation simulate() hands the controller; u [B][nu] holds
// u_prev on entry and u on exit.
__global__ __launch_bounds__(kLqrThreads) void lqr_ctrl_kernel(const LqrLoopDesc* __restrict__ descs,
                                                                double* __restrict__ states, int cur,
                                                                const double* __restrict__ sim, int snx, int no,
                                                                int nu, double* __restrict__ u,
                                                                const double* __restrict__ kbuf,
                                                                const double* __restrict__ gbuf,
                                                                const double* __restrict__ lbuf,
                                                                const double* __restrict__ lo,
                                                                const double* __restrict__ hi) {
  const int b = blockIdx.x, t = threadIdx.x;
  const LqrLoopDesc* d = descs + b;
  const int n = d->n, rule = d->rule;
  const double* __restrict__ ab = d->ab;
  const double* s_old = states + d->s + (size_t)cur * n;
  double* s_new = states + d->s + (size_t)(1 - cur) * n;
  const double* obs = sim + (size_t)b * snx;
  double* ub = u + (size_t)b * nu;
  const int m = n + nu;
  if (rule == 0) {
    for (int i = t; i < n; i += kLqrThreads) s_new[i] = obs[i];
  } else if (rule == 1) {
    for (int i = t; i < n; i += kLqrThreads) {
      if (i < no) {
        s_new[i] = obs[i];
        continue;
      }
      const double* row = ab + (size_t)i * m;
      double a = 0.0, c = 0.0;
      for (int j = 0; j < n; ++j) a = fma(row[j], s_old[j], a);
      for (int r = 0; r < nu; ++r) c = fma(row[n + r], ub[r], c);
      s_new[i] = a + c;
    }
  } else {
    const double* prog = lbuf + d->lift;
    for (int e = t; e < n; e += kLqrThreads) {
      const int f = e / no, j = e - f * no;
      const double o = obs[j];
      const int kind = (int)prog[2 * f];
      const double par = prog[2 * f + 1];
      double v = o;
      if (kind == 1) {                     // o ** p rounded once (as state_lift_kernel)
        const int pw = (int)par;
        double h = pw >= 1 ? o : 1.0, l = 0.0;
        for (int k = 1; k < pw; ++k) {
          const double ph = h * o;
          const double pe = fma(h, o, -ph) + l * o;
          h = ph + pe;
          l = pe - (h - ph);
        }
        v = h;
      } else if (kind == 2) {
        v = sin(par * o);
      } else if (kind == 3) {
        v = cos(par * o);
      }
      s_new[e] = v;
    }
  }
  __syncthreads();
  if (t < nu) {
    const double* kr = kbuf + d->k + (size_t)t * n;
    const double* g = gbuf + d->goal;
    double acc = 0.0;
    for (int j = 0; j < n; ++j) acc = fma(kr[j], s_new[j] - (j < no ? g[j] : 0.0), acc);
    if (!d->noclip) {
      acc = acc > hi[t] ? hi[t] : acc;    // np.minimum then np.maximum (NaN propagates)
      acc = acc < lo[t] ? lo[t] : acc;
    }
    ub[t] = acc;
  }
}

// sim <- next; traj_obs[b][step + 1] = next[b][:no]; traj_ctrls[b][step] = u[b]
__global__ void lqr_record_kernel(const double* __restrict__ next, const double* __restrict__ u,
                                  double* __restrict__ sim, double* __restrict__ traj_obs,
                                  double* __restrict__ traj_ctrls, int B, int snx, int no, int nu, int T1, int step) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B * snx) {
    const int p = i / snx, c = i - p * snx;
    const double v = next[i];
    sim[i] = v;
    if (c < no) traj_obs[((size_t)p * T1 + step + 1) * no + c] = v;
  }
  if (i < B * nu) {
    const int p = i / nu, c = i - p * nu;
    traj_ctrls[((size_t)p * T1 + step) * nu + c] = u[i];
  }
}

}  // namespace ampc
#endif
