// stable_kernels.hpp -- stable fits of Koopman models in f64 (reference: autompc/sysid/stable_koopman.py:47-167
// stabilize_discrete), one configuration per basis: the projected fast-gradient method on (S, U, B, Bcon), A =
// S^-1 U B S, run on the Gram (sysid/stable_fit.py states the recursion; this file follows it step for step).
//
// The Gram of the design [F | Y] comes from linfit_gram_kernel (linfit_kernels.hpp, gram_frame.hpp; the tile list
// holds the tile rows of F against all columns and the diagonal tiles of Y).  stable_gram_kernel sums the partial
// tiles over the row splits in order: G = [F'F | F'Y] ([nf][ldg], F'F symmetric to the bit: one summation per pair)
// and yy_t = Y_t'Y_t.  The least-squares W0 is linfit_solve_kernel's (the scaled Cholesky, its acceptance rule).
//
// stable_fgm_kernel: one workgroup per configuration runs the whole iteration.  With D = [A | Bcon] - W0, T = D G:
// e^2 = e0^2 + tr(T D'), e0^2 = sum yy - sum W0 o (F'Y)'; the gradients follow from T, S, S^-1, U, B.  Per trial two
// symmetric eigendecompositions (S clipped below at 1e-15, B to [0, 1]) and one polar factor M (M'M)^-1/2 through a
// third, polished by two Newton-Schulz steps; S^-1 from the decomposition of S.  The eigensolver is two-sided cyclic
// Jacobi in the round-robin parallel order (stable_pair), matrix and vectors resident in LDS: per round n / 2
// rotations are computed, then applied together as 2 x 2 block updates A <- J'AJ (every block owned by one thread, in
// place) and V <- V J.  A pair is rotated when |a_pq| > 2^-53 (|a_pp| + |a_qq|); a sweep without rotation ends the
// iteration, kStableSweeps without that is status 1.  The other matrices live in a per-configuration global scratch
// block (L2-resident: under 1 MB at n = 64); products are plain fma chains in k order, the trace a per-thread strided
// sum, a fixed xor tree per wave and the waves in order.  No atomics: a configuration's result depends on nothing but
// its Gram.
#ifndef AMPC_STABLE_KERNELS_HPP
#define AMPC_STABLE_KERNELS_HPP
#include <hip/hip_runtime.h>

#include "gram_frame.hpp"

namespace ampc {

constexpr int kStableMaxN = 64, kStableMaxCtrl = 16;
constexpr int kStableThreads = 512, kStableWaves = kStableThreads / 64;
constexpr int kStableLd = kStableMaxN + 1;               // LDS row stride: odd, column walks are conflict-free
constexpr int kStableSweeps = 30;                        // stable_fit.JACOBI_SWEEPS
constexpr int kStableMaxOuter = 30, kStableLs = 20, kStableLsFirst = 100;
constexpr double kStableLsParam = 1.5, kStableAlpha0 = 0.5, kStableFloor = 1e-15, kStableConverged = 1e-12;
constexpr double kStablePolarEps = 0x1p-40, kStableJacobiEps = 0x1p-53;
constexpr size_t kStableLdsBytes = (size_t)2 * kStableMaxN * kStableLd * sizeof(double);

// doubles of scratch per configuration: 21 n x n, 4 n x nu and 3 n x nf matrices (stable_fgm_kernel's layout)
__host__ __device__ constexpr long long stable_ws_doubles(int n, int nu) {
  return 21LL * n * n + 4LL * n * nu + 3LL * n * (n + nu);
}

// grid (blocks over nf * (nf + nt) + nt entries).  part: [splits][wp][wp]; G: [nf][wp]; yy: [nt]
__global__ void stable_gram_kernel(const double* __restrict__ part, double* __restrict__ G, double* __restrict__ yy,
                                   int splits, int nf, int nt, int wp) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x, w = nf + nt;
  if (e >= nf * w + nt) return;
  if (e >= nf * w) {
    const int c = nf + (e - nf * w);
    yy[e - nf * w] = gram_split_sum(part, splits, wp, wp, c, c, true);
    return;
  }
  const int r = e / w, c = e - r * w;
  const int a = (c < nf && c < r) ? c : r, b = (c < nf && c < r) ? r : c;      // one summation per pair
  G[(size_t)r * wp + c] = gram_split_sum(part, splits, wp, wp, a, b, true);
}

// One configuration.  Read field by field through a global pointer (uniform loads), as LinfitSolveDesc.
struct StableDesc {
  const double* G;          // [nf][ldg]: F'F, F'Y from column nf
  const double* W0;         // [n][nf]: the least-squares coefficients
  const double* yy;         // [n]
  const int* w0_status;     // linfit_solve_kernel's status of W0
  double* ws;               // stable_ws_doubles(n, nu) doubles
  double* out;              // [n][nf]
  double tie;
  int n, nu, ldg, id;
};

// pair a (0 .. m / 2 - 1) of round r (0 .. m - 2) on m (even) indices: stable_fit.jacobi_pairs
__device__ inline void stable_pair(int m, int r, int a, int& p, int& q) {
  int x, y;
  if (a == 0) { x = m - 1; y = r; }
  else { x = (r + a) % (m - 1); y = (r - a + (m - 1)) % (m - 1); }
  p = x < y ? x : y;
  q = x < y ? y : x;
}

// C [rows][cols] (+)= op(A) op(B) over `inner`; SUB: C = C - product.  Ends with a barrier.
template <bool TA, bool TB, bool SUB>
__device__ inline void stable_mm(double* C, int ldc, const double* A, int lda, const double* B, int ldb, int rows,
                                 int cols, int inner) {
  for (int e = threadIdx.x; e < rows * cols; e += kStableThreads) {
    const int r = e / cols, c = e - r * cols;
    double acc = 0.0;
    for (int k = 0; k < inner; ++k) {
      const double a = TA ? A[(size_t)k * lda + r] : A[(size_t)r * lda + k];
      const double b = TB ? B[(size_t)c * ldb + k] : B[(size_t)k * ldb + c];
      acc = fma(a, b, acc);
    }
    C[(size_t)r * ldc + c] = SUB ? C[(size_t)r * ldc + c] - acc : acc;
  }
  __syncthreads();
}

struct StableShared {
  double sc[kStableMaxN / 2], ss[kStableMaxN / 2];
  int sp[kStableMaxN / 2], sq[kStableMaxN / 2], srot[kStableMaxN / 2];
  double lam[kStableMaxN], f1[kStableMaxN], f2[kStableMaxN];
  double red[kStableWaves];
  double cond;
  int rot, bad;
};

// Eigendecomposition of the symmetric n x n matrix in A (LDS, stride kStableLd): on return its diagonal is in
// sh.lam, the vectors are the columns of V.  Uniform return: false at the sweep cap.
__device__ inline bool stable_jacobi(double* A, double* V, int n, StableShared& sh) {
  const int t = threadIdx.x, m = n + (n & 1), h = m / 2;
  constexpr int L = kStableLd;
  if (m > n)
    for (int i = t; i < m; i += kStableThreads) A[i * L + n] = A[n * L + i] = 0.0;
  for (int e = t; e < m * m; e += kStableThreads) V[(e / m) * L + e % m] = e / m == e % m ? 1.0 : 0.0;
  __syncthreads();
  bool done = false;
  for (int sweep = 0; sweep < kStableSweeps && !done; ++sweep) {
    if (t == 0) sh.rot = 0;
    __syncthreads();
    for (int r = 0; r < m - 1; ++r) {
      if (t < h) {
        int p, q;
        stable_pair(m, r, t, p, q);
        const double app = A[p * L + p], aqq = A[q * L + q], apq = A[p * L + q];
        const bool rot = fabs(apq) > kStableJacobiEps * (fabs(app) + fabs(aqq));
        double c = 1.0, s = 0.0;
        if (rot) {
          const double tau = (aqq - app) / (2.0 * apq);
          const double tt = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
          c = 1.0 / sqrt(1.0 + tt * tt);
          s = tt * c;
          sh.rot = 1;             // no race: every lane that writes here writes the same value; read after the sweep
        }
        sh.sp[t] = p; sh.sq[t] = q; sh.sc[t] = c; sh.ss[t] = s; sh.srot[t] = rot;
      }
      __syncthreads();
      for (int e = t; e < h * h; e += kStableThreads) {
        const int a = e / h, b = e - a * h;
        const int pa = sh.sp[a], qa = sh.sq[a], pb = sh.sp[b], qb = sh.sq[b];
        const double ca = sh.sc[a], sa = sh.ss[a], cb = sh.sc[b], sb = sh.ss[b];
        const double x00 = A[pa * L + pb], x01 = A[pa * L + qb], x10 = A[qa * L + pb], x11 = A[qa * L + qb];
        const double y00 = ca * x00 - sa * x10, y01 = ca * x01 - sa * x11;       // rows: J_a' X
        const double y10 = sa * x00 + ca * x10, y11 = sa * x01 + ca * x11;
        double z00 = cb * y00 - sb * y01, z01 = sb * y00 + cb * y01;             // columns: (.) J_b
        double z10 = cb * y10 - sb * y11, z11 = sb * y10 + cb * y11;
        if (a == b && sh.srot[a]) z01 = z10 = 0.0;
        A[pa * L + pb] = z00; A[pa * L + qb] = z01; A[qa * L + pb] = z10; A[qa * L + qb] = z11;
      }
      // no barrier between the update of A above and that of V below: one touches A alone, the other V alone, and
      // both only read sp / sq / sc / ss / srot, which nothing writes between the barrier above and the one below
      for (int e = t; e < m * h; e += kStableThreads) {
        const int i = e / h, b = e - i * h;
        const int pb = sh.sp[b], qb = sh.sq[b];
        const double cb = sh.sc[b], sb = sh.ss[b];
        const double v0 = V[i * L + pb], v1 = V[i * L + qb];
        V[i * L + pb] = cb * v0 - sb * v1;
        V[i * L + qb] = sb * v0 + cb * v1;
      }
      __syncthreads();
    }
    done = sh.rot == 0;
    __syncthreads();
  }
  for (int i = t; i < n; i += kStableThreads) sh.lam[i] = A[i * L + i];
  __syncthreads();
  return done;
}

// X [n][n] = V diag(f) V', symmetric to the bit
__device__ inline void stable_spectral(double* X, const double* V, const double* f, int n) {
  constexpr int L = kStableLd;
  for (int e = threadIdx.x; e < n * n; e += kStableThreads) {
    const int i = e / n, j = e - i * n;
    double acc = 0.0;
    for (int k = 0; k < n; ++k) acc = fma(f[k], V[i * L + k] * V[j * L + k], acc);
    X[e] = acc;
  }
  __syncthreads();
}

// A (LDS) = the symmetric part of Y - step g
__device__ inline void stable_load_sym(double* A, const double* Y, const double* g, double step, int n) {
  for (int e = threadIdx.x; e < n * n; e += kStableThreads) {
    const int i = e / n, j = e - i * n;
    A[i * kStableLd + j] = 0.5 * ((Y[i * n + j] - g[i * n + j] * step) + (Y[j * n + i] - g[j * n + i] * step));
  }
  __syncthreads();
}

// A (LDS) = M'M
__device__ inline void stable_load_gram(double* A, const double* M, int n) {
  for (int e = threadIdx.x; e < n * n; e += kStableThreads) {
    const int i = e / n, j = e - i * n;
    double acc = 0.0;
    for (int k = 0; k < n; ++k) acc = fma(M[k * n + i], M[k * n + j], acc);
    A[i * kStableLd + j] = acc;
  }
  __syncthreads();
}

// every thread returns the sum of v over the workgroup: the waves' xor trees, then the waves in order
__device__ inline double stable_block_sum(double v, StableShared& sh) {
  for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) sh.red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < kStableWaves; ++w) s = s + sh.red[w];
  __syncthreads();
  return s;
}

// One iterate's matrices in the scratch block
struct StableIt {
  double *S, *U, *B, *Sinv, *R, *Bc, *T;
  double cond;
};

// The polar factor of M ([n][n], global; overwritten) into U: M (M'M)^-1/2 by the eigensolver, two Newton-Schulz
// steps.  X1, X2: scratch.  On return sh.lam holds the eigenvalues of M'M and V their vectors; decomposed: they hold
// them already (the caller ran the eigensolver on M'M).  Uniform false: declined.
__device__ inline bool stable_polar(double* U, double* M, double* X1, double* X2, double* H, double* A, double* V,
                                    int n, StableShared& sh, bool decomposed = false) {
  const int t = threadIdx.x;
  bool ok = true;
  if (!decomposed) {
    stable_load_gram(A, M, n);
    ok = stable_jacobi(A, V, n, sh);
  }
  if (t == 0) {
    double lo = sh.lam[0], hi = sh.lam[0];
    bool fin = true;
    for (int i = 0; i < n; ++i) {
      lo = fmin(lo, sh.lam[i]); hi = fmax(hi, sh.lam[i]);
      fin = fin && isfinite(sh.lam[i]);
      sh.f1[i] = 1.0 / sqrt(sh.lam[i]);
    }
    sh.bad = !(fin && lo > kStablePolarEps * hi);
  }
  __syncthreads();
  const bool bad = sh.bad != 0;
  __syncthreads();
  if (!ok || bad) return false;
  stable_spectral(H, V, sh.f1, n);
  stable_mm<false, false, false>(X1, n, M, n, H, n, n, n, n);
  double* cur = X1;
  double* nxt = M;
  for (int k = 0; k < 2; ++k) {
    stable_mm<true, false, false>(X2, n, cur, n, cur, n, n, n, n);
    for (int e = t; e < n * n; e += kStableThreads) X2[e] = (e / n == e % n ? 1.5 : 0.0) - 0.5 * X2[e];
    __syncthreads();
    stable_mm<false, false, false>(k == 1 ? U : nxt, n, cur, n, X2, n, n, n, n);
    cur = nxt;
  }
  return true;
}

// R = S^-1 U B S, D = [R | Bcon] - W0, T = D G; returns e = sqrt(e0^2 + tr(T D')) to every thread
__device__ inline double stable_finish(const StableIt& it, double* X1, double* X2, double* D, const double* G, int ldg,
                                       const double* W0, double e0sq, int n, int nu, StableShared& sh) {
  const int t = threadIdx.x, nf = n + nu;
  stable_mm<false, false, false>(X1, n, it.B, n, it.S, n, n, n, n);
  stable_mm<false, false, false>(X2, n, it.U, n, X1, n, n, n, n);
  stable_mm<false, false, false>(it.R, n, it.Sinv, n, X2, n, n, n, n);
  for (int e = t; e < n * nf; e += kStableThreads) {
    const int r = e / nf, c = e - r * nf;
    D[e] = (c < n ? it.R[r * n + c] : it.Bc[r * nu + c - n]) - W0[e];
  }
  __syncthreads();
  stable_mm<false, false, false>(it.T, nf, D, nf, G, ldg, n, nf, nf);
  double tr = 0.0;
  for (int e = t; e < n * nf; e += kStableThreads) tr = fma(it.T[e], D[e], tr);
  tr = stable_block_sum(tr, sh);
  const double v = e0sq + tr;
  return sqrt(v > 0.0 ? v : 0.0);                          // (NaN passes through)
}

// grid (configurations), block kStableThreads, dynamic LDS kStableLdsBytes.  status: 0, 1 (not fitted here) or 2 (a
// decision within tie); error, iterations, trials, margin as stable_fit.fgm_on_gram.
__global__ __launch_bounds__(kStableThreads) void stable_fgm_kernel(const StableDesc* __restrict__ descs,
                                                                    int* __restrict__ status,
                                                                    double* __restrict__ error_out,
                                                                    int* __restrict__ iterations,
                                                                    int* __restrict__ trials_out,
                                                                    double* __restrict__ margin_out) {
  extern __shared__ __attribute__((aligned(16))) double stable_lds[];
  __shared__ StableShared sh;
  double* A = stable_lds;
  double* V = stable_lds + kStableMaxN * kStableLd;
  const StableDesc* d = descs + blockIdx.x;
  const int t = threadIdx.x, n = d->n, nu = d->nu, nf = n + nu, ldg = d->ldg, id = d->id;
  const double* G = d->G;
  const double* W0 = d->W0;
  const double tie = d->tie;
  double* out = d->out;
  const int N2 = n * n, NU = n * nu, NF = n * nf;
  double* w = d->ws;
  StableIt its[2];
  for (int k = 0; k < 2; ++k) {
    its[k].S = w; its[k].U = w + N2; its[k].B = w + 2 * N2; its[k].Sinv = w + 3 * N2; its[k].R = w + 4 * N2;
    its[k].Bc = w + 5 * N2; its[k].T = w + 5 * N2 + NU;
    its[k].cond = 1.0;
    w += 5 * N2 + NU + NF;
  }
  double* Ys = w; double* Yu = w + N2; double* Yb = w + 2 * N2; double* Ybc = w + 3 * N2;
  w += 3 * N2 + NU;
  double* gS = w; double* gU = w + N2; double* gB = w + 2 * N2; double* gBc = w + 3 * N2;
  w += 3 * N2 + NU;
  double* M = w; double* H = w + N2; double* X1 = w + 2 * N2; double* X2 = w + 3 * N2; double* X3 = w + 4 * N2;
  double* D = w + 5 * N2;

  bool ok = *d->w0_status == 0;
  double error = 0.0, margin = __builtin_inf(), e0sq = 0.0, norm_y = 0.0;
  int n_iter = 0, n_trials = 0, cur = 0;

  if (ok) {
    // e0^2 = sum yy - sum W0 o (F'Y)', |Y|_F
    double a = 0.0, b = 0.0;
    for (int e = t; e < n; e += kStableThreads) a = a + d->yy[e];
    for (int e = t; e < NF; e += kStableThreads) {
      const int r = e / nf, c = e - r * nf;
      b = fma(W0[e], G[(size_t)c * ldg + nf + r], b);
    }
    a = stable_block_sum(a, sh);
    b = stable_block_sum(b, sh);
    e0sq = a - b > 0.0 ? a - b : 0.0;
    norm_y = sqrt(a);
    ok = isfinite(a) && isfinite(b);
  }
  if (ok) {
    // S = I, [U, B] the polar decomposition of the least-squares A with B clipped to [0, 1], Bcon its control part
    StableIt& it = its[0];
    for (int e = t; e < N2; e += kStableThreads) {
      const int r = e / n, c = e - r * n;
      M[e] = W0[r * nf + c];
      it.S[e] = it.Sinv[e] = r == c ? 1.0 : 0.0;
    }
    for (int e = t; e < NU; e += kStableThreads) it.Bc[e] = W0[(e / nu) * nf + n + e % nu];
    __syncthreads();
    // one decomposition of M'M serves both: B from sh.lam and V first (stable_polar overwrites M, not them)
    stable_load_gram(A, M, n);
    ok = stable_jacobi(A, V, n, sh);
    if (ok) {
      for (int i = t; i < n; i += kStableThreads) {
        const double s = sqrt(sh.lam[i]);
        sh.f2[i] = s < 1.0 ? s : 1.0;                    // (lam < 0 -> NaN: the polar test below declines)
      }
      __syncthreads();
      stable_spectral(it.B, V, sh.f2, n);
      ok = stable_polar(it.U, M, X1, X2, H, A, V, n, sh, true);
    }
    if (ok) {
      error = stable_finish(it, X1, X2, D, G, ldg, W0, e0sq, n, nu, sh);
      ok = isfinite(error);
    }
  }
  if (ok) {
    for (int e = t; e < N2; e += kStableThreads) { Ys[e] = its[0].S[e]; Yu[e] = its[0].U[e]; Yb[e] = its[0].B[e]; }
    for (int e = t; e < NU; e += kStableThreads) Ybc[e] = its[0].Bc[e];
    __syncthreads();
    double step = 1.0, alpha = kStableAlpha0;
    int i = 1, restarti = 1, inner0 = 1;
    while (ok && i < kStableMaxOuter) {
      ++n_iter;
      const StableIt& c = its[cur];
      StableIt& x = its[cur ^ 1];
      // the gradients at the current iterate
      stable_mm<false, false, false>(X1, n, c.Sinv, n, c.T, nf, n, n, n);              // t1
      stable_mm<false, false, false>(X2, n, X1, n, c.S, n, n, n, n);                   // x1 = t1 S
      stable_mm<true, false, false>(X3, n, c.U, n, X1, n, n, n, n);                    // x2 = U' t1
      stable_mm<false, false, false>(gS, n, c.B, n, X3, n, n, n, n);
      stable_mm<false, true, true>(gS, n, X1, n, c.R, n, n, n, n);                     // gS = B x2 - t1 A'
      stable_mm<false, false, false>(gU, n, X2, n, c.B, n, n, n, n);
      stable_mm<true, false, false>(gB, n, c.U, n, X2, n, n, n, n);
      for (int e = t; e < NU; e += kStableThreads) gBc[e] = c.T[(e / nu) * nf + n + e % nu];
      __syncthreads();
      double error_next = __builtin_inf();
      int inner = 1;
      step *= 2.0;
      while (ok && error_next > error && ((i == 1 && inner <= kStableLsFirst) || inner <= kStableLs)) {
        // project onto the feasible set
        stable_load_sym(A, Ys, gS, step, n);
        ok = stable_jacobi(A, V, n, sh);
        if (!ok) break;
        if (t == 0) {
          double lo = __builtin_inf(), hi = 0.0;
          for (int k = 0; k < n; ++k) {
            const double l = sh.lam[k] > kStableFloor ? sh.lam[k] : kStableFloor;
            sh.f1[k] = l; sh.f2[k] = 1.0 / l;
            lo = fmin(lo, l); hi = fmax(hi, l);
          }
          sh.cond = hi / lo;
        }
        __syncthreads();
        x.cond = sh.cond;
        stable_spectral(x.S, V, sh.f1, n);
        stable_spectral(x.Sinv, V, sh.f2, n);
        for (int e = t; e < N2; e += kStableThreads) M[e] = Yu[e] - gU[e] * step;
        __syncthreads();
        ok = stable_polar(x.U, M, X1, X2, H, A, V, n, sh);
        if (!ok) break;
        stable_load_sym(A, Yb, gB, step, n);
        ok = stable_jacobi(A, V, n, sh);
        if (!ok) break;
        for (int k = t; k < n; k += kStableThreads) {
          const double l = sh.lam[k];
          sh.f1[k] = l < 0.0 ? 0.0 : (l > 1.0 ? 1.0 : l);
        }
        __syncthreads();
        stable_spectral(x.B, V, sh.f1, n);
        for (int e = t; e < NU; e += kStableThreads) x.Bc[e] = Ybc[e] - gBc[e] * step;
        __syncthreads();
        error_next = stable_finish(x, X1, X2, D, G, ldg, W0, e0sq, n, nu, sh);
        if (!isfinite(error_next)) { ok = false; break; }
        ++n_trials;
        if (error > 0.0) margin = fmin(margin, fabs(error_next - error) / error);
        step /= kStableLsParam;
        ++inner;
      }
      if (!ok) break;
      if (i == 1) inner0 = inner;
      const double a2 = alpha * alpha;
      double alpha_next = (sqrt(a2 * a2 + 4.0 * a2) - a2) / 2.0;
      const double beta = alpha * (1.0 - alpha) / (a2 + alpha_next);
      if (inner >= kStableLs + 1) {                        // the line search failed
        if (restarti == 1) {                               // restart the FGM from the current iterate
          restarti = 0;
          alpha_next = kStableAlpha0;
          for (int e = t; e < N2; e += kStableThreads) { Ys[e] = c.S[e]; Yu[e] = c.U[e]; Yb[e] = c.B[e]; }
          for (int e = t; e < NU; e += kStableThreads) Ybc[e] = c.Bc[e];
          __syncthreads();
          error_next = error;
          double shrink = 1.0;                             // lsparam ** inner0, by multiplication as the host form
          for (int k = 0; k < inner0; ++k) shrink *= kStableLsParam;
          step = 1.0 / (c.cond * c.cond) / shrink;
        } else {
          break;
        }
      } else {
        restarti = 1;
        for (int e = t; e < N2; e += kStableThreads) {
          Ys[e] = x.S[e] + beta * (x.S[e] - c.S[e]);
          Yu[e] = x.U[e] + beta * (x.U[e] - c.U[e]);
          Yb[e] = x.B[e] + beta * (x.B[e] - c.B[e]);
        }
        for (int e = t; e < NU; e += kStableThreads) Ybc[e] = x.Bc[e] + beta * (x.Bc[e] - c.Bc[e]);
        __syncthreads();
        cur ^= 1;
      }
      ++i;
      error = error_next;
      alpha = alpha_next;
      const double thr = kStableConverged * norm_y;
      if (thr > 0.0) margin = fmin(margin, fabs(error - thr) / thr);
      if (error < thr) break;
    }
  }
  // [A | Bcon] of the current iterate
  int bad = 0;
  if (ok) {
    const StableIt& c = its[cur];
    for (int e = t; e < NF; e += kStableThreads) {
      const int r = e / nf, cc = e - r * nf;
      const double v = cc < n ? c.R[r * n + cc] : c.Bc[r * nu + cc - n];
      out[e] = v;
      if (!isfinite(v)) bad = 1;
    }
  }
  bad = __syncthreads_or(bad || !ok);
  if (bad)
    for (int e = t; e < NF; e += kStableThreads) out[e] = __builtin_nan("");
  if (t == 0) {
    status[id] = bad ? 1 : (margin <= tie ? 2 : 0);
    error_out[id] = bad ? __builtin_nan("") : error;
    iterations[id] = bad ? 0 : n_iter;
    trials_out[id] = bad ? 0 : n_trials;
    margin_out[id] = bad ? __builtin_inf() : margin;
  }
}

}  // namespace ampc
#endif
