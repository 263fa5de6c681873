// lasso_kernels.hpp -- lasso fits of Koopman models in f64 (reference: autompc/sysid/koopman.py:150-156, sklearn's
// Lasso with its defaults), many (basis, alpha) configurations per call: cyclic coordinate descent on the Gram.
//
// The Gram of the design [1 | F | Y] comes from linfit_gram_kernel (linfit_kernels.hpp, gram_frame.hpp; its tile list
// here holds the tile rows of [1 | F] against all columns and the diagonal tiles of Y).  lasso_centre_kernel sums the
// partial tiles over the row splits in order (gram_split_sum) and centres through the constant column: with m rows,
// mu = sum F / m, ybar = sum Y / m,
//   G = F'F - m mu mu'      Q = F'Y - m mu ybar'      yy_t = Y_t'Y_t - m ybar_t^2
// G is stored [nf][ldp] (ldp = nf rounded up to 64, padding zero) and symmetric to the bit (each pair is summed once),
// Q transposed [nt][ldp].  bad[design] is set when the centring took half the digits of a column's sum of squares
// (centred < 2^-26 raw, raw != 0) or a value is not finite.
//
// lasso_cd_kernel: one wave per (configuration, target), no LDS, no barrier.  Lane l holds elements l, l + 64, .. of
// w, H = G w, Q_t and diag(G) in registers; the coordinate loop is a serial chain (read H_i, w_i by v_readlane, soft
// threshold, H += d G[i][:]), row i + 1 of G is loaded from L2 while step i computes.  Every product and sum is
// rounded on its own (no contraction), in the order of sysid/lasso_fit.py; the dot products of the gap are per-lane
// sums in slot order followed by a fixed xor tree: a pair's result depends on nothing but its Gram, alpha and target.
#ifndef AMPC_LASSO_KERNELS_HPP
#define AMPC_LASSO_KERNELS_HPP
#include <hip/hip_runtime.h>

#include "gram_frame.hpp"

namespace ampc {

constexpr int kLassoMaxFeat = 272;                       // 256 states + 16 controls
constexpr int kLassoSlots = (kLassoMaxFeat + 63) / 64;   // register slots per lane
constexpr int kLassoMaxSweeps = 1000;                    // sklearn's max_iter
constexpr double kLassoTol = 1e-4;                       // sklearn's tol

struct LassoDesign {
  const double* part;     // [splits][wp][wp] partial tiles of the Gram of [1 | F | Y]
  double* G;              // [nf][ldp]
  double* Qt;             // [nt][ldp]
  double* yy;             // [nt]
  int* bad;               // one flag
  int nf, nt, wp, ldp, splits;
  double m;               // design rows
};

// entry (a, b) of the raw Gram: the ordered sum of its partial tiles (of Y only the diagonal tiles exist, and only
// they are asked for)
__device__ inline double lasso_raw(const LassoDesign& d, int a, int b) {
  return gram_split_sum(d.part, d.splits, d.wp, d.wp, a, b, true);
}

// grid (blocks over (nf + nt) * ldp + nt entries, designs)
__global__ void lasso_centre_kernel(const LassoDesign* __restrict__ designs) {
#pragma clang fp contract(off)
  const LassoDesign d = designs[blockIdx.y];
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const int nf = d.nf, nt = d.nt, ldp = d.ldp;
  if (e >= (nf + nt) * ldp + nt) return;
  if (e >= (nf + nt) * ldp) {                            // yy_t
    const int t = e - (nf + nt) * ldp, c = 1 + nf + t;
    const double raw = lasso_raw(d, c, c), yb = lasso_raw(d, 0, c) / d.m;
    const double v = raw - d.m * (yb * yb);
    d.yy[t] = v;
    if (!isfinite(v) || (raw != 0.0 && v < 0x1p-26 * raw)) *d.bad = 1;
    return;
  }
  const int r = e / ldp, j = e - r * ldp;
  if (r < nf) {                                          // G[r][j]
    double v = 0.0;
    if (j < nf) {
      const int a = r < j ? r : j, b = r < j ? j : r;    // one summation per pair
      const double raw = lasso_raw(d, 1 + a, 1 + b);
      const double ma = lasso_raw(d, 0, 1 + a) / d.m, mb = lasso_raw(d, 0, 1 + b) / d.m;
      v = raw - d.m * (ma * mb);
      if (!isfinite(v) || (a == b && raw != 0.0 && v < 0x1p-26 * raw)) *d.bad = 1;
    }
    d.G[(size_t)r * ldp + j] = v;
  } else {                                               // Qt[t][j]
    const int t = r - nf;
    double v = 0.0;
    if (j < nf) {
      const double raw = lasso_raw(d, 1 + j, 1 + nf + t);
      const double mj = lasso_raw(d, 0, 1 + j) / d.m, yb = lasso_raw(d, 0, 1 + nf + t) / d.m;
      v = raw - d.m * (mj * yb);
      if (!isfinite(v)) *d.bad = 1;
    }
    d.Qt[(size_t)t * ldp + j] = v;
  }
}

// One (configuration, target).  Read field by field through a global pointer (uniform loads), as LinfitSolveDesc.
struct LassoPair {
  const double* G;        // [nf][ldp]
  const double* q;        // [ldp]: the target's row of Qt
  const double* yy;       // the target's yy
  const int* bad;         // the design's flag
  double* out;            // [nf]
  double alpha;           // lasso_alpha * m
  int nf, ldp, id, pad;
};

__device__ inline double lasso_lane(double v, int l) {
  const int lo = __builtin_amdgcn_readlane((int)(__double_as_longlong(v) & 0xffffffffLL), l);
  const int hi = __builtin_amdgcn_readlane((int)(__double_as_longlong(v) >> 32), l);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// fixed xor tree over the 64 lanes; every lane ends with the same bits
__device__ inline double lasso_wave_sum(double v) {
#pragma clang fp contract(off)
  for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
  return v;
}
__device__ inline double lasso_wave_max(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// grid (pairs), block 64.  status [pairs]: 0, or 1 when the design is bad or a result is not finite; margins
// [pairs][2]: the smallest |gap - tol| / tol over the gap checks and |d_w_max / w_max - 1e-4| / 1e-4 over the sweeps.
__global__ __launch_bounds__(64) void lasso_cd_kernel(const LassoPair* __restrict__ pairs, int* __restrict__ status,
                                                      double* __restrict__ margins, int* __restrict__ sweeps) {
#pragma clang fp contract(off)
  const LassoPair* p = pairs + blockIdx.x;
  const int lane = threadIdx.x, nf = p->nf, ldp = p->ldp, id = p->id;
  const int ns = ldp >> 6;
  const double* __restrict__ G = p->G;
  const double alpha = p->alpha, yy = *p->yy, tol = kLassoTol * yy;
  double* out = p->out;
  if (*p->bad) {
    for (int j = lane; j < nf; j += 64) out[j] = __builtin_nan("");
    if (lane == 0) {
      status[id] = 1; sweeps[id] = 0;
      margins[2 * id] = margins[2 * id + 1] = __builtin_inf();
    }
    return;
  }
  double w[kLassoSlots], H[kLassoSlots], q[kLassoSlots], dg[kLassoSlots], row[kLassoSlots], nxt[kLassoSlots];
#pragma unroll
  for (int k = 0; k < kLassoSlots; ++k) {
    const int j = lane + 64 * k;
    w[k] = H[k] = 0.0;
    q[k] = k < ns ? p->q[j] : 0.0;
    dg[k] = (k < ns && j < nf) ? G[(size_t)j * ldp + j] : 0.0;
    nxt[k] = k < ns ? G[j] : 0.0;                           // row 0
  }
  double mgap = __builtin_inf(), mratio = __builtin_inf();
  int it = 0;
  for (;; ++it) {
    double dmax = 0.0, wmax = 0.0;
#pragma unroll
    for (int s = 0; s < kLassoSlots; ++s) {
      if (s >= ns) break;
      const int lim = nf - 64 * s < 64 ? nf - 64 * s : 64;
      for (int l = 0; l < lim; ++l) {
        const int i = 64 * s + l, in = i + 1 < nf ? i + 1 : 0;
#pragma unroll
        for (int k = 0; k < kLassoSlots; ++k) {
          row[k] = nxt[k];
          if (k < ns) nxt[k] = G[(size_t)in * ldp + lane + 64 * k];
        }
        const double gii = lasso_lane(dg[s], l);
        if (gii == 0.0) continue;
        const double wi = lasso_lane(w[s], l);
        const double tmp = lasso_lane(q[s], l) - lasso_lane(H[s], l) + wi * gii;
        const double mag = fabs(tmp) - alpha;
        const double sg = tmp > 0.0 ? 1.0 : tmp < 0.0 ? -1.0 : 0.0;
        const double wn = sg * (mag > 0.0 ? mag : 0.0) / gii;
        const double d = wn - wi;
        if (wn != wi) {
#pragma unroll
          for (int k = 0; k < kLassoSlots; ++k)
            if (k < ns) H[k] = H[k] + d * row[k];
          if (lane == l) w[s] = wn;
        }
        dmax = fmax(dmax, fabs(d));
        wmax = fmax(wmax, fabs(wn));
      }
    }
    double ratio = 0.0;
    if (wmax > 0.0) {
      ratio = dmax / wmax;
      mratio = fmin(mratio, fabs(ratio - kLassoTol) / kLassoTol);
    }
    bool stop = false;
    if (wmax == 0.0 || ratio < kLassoTol || it == kLassoMaxSweeps - 1) {
      double dn = 0.0, wq = 0.0, wh = 0.0, l1 = 0.0;
#pragma unroll
      for (int k = 0; k < kLassoSlots; ++k) {
        if (k >= ns) break;
        dn = fmax(dn, fabs(q[k] - H[k]));
        wq = wq + w[k] * q[k];
        wh = wh + w[k] * H[k];
        l1 = l1 + fabs(w[k]);
      }
      dn = lasso_wave_max(dn);
      wq = lasso_wave_sum(wq);
      wh = lasso_wave_sum(wh);
      l1 = lasso_wave_sum(l1);
      const double r2 = yy - 2.0 * wq + wh, ry = yy - wq;
      double c = 1.0, gap = r2;
      if (dn > alpha) {
        c = alpha / dn;
        gap = 0.5 * (r2 + r2 * (c * c));
      }
      gap = gap + (alpha * l1 - c * ry);
      if (tol > 0.0) mgap = fmin(mgap, fabs(gap - tol) / tol);
      stop = gap < tol;
    }
    if (stop) break;
    if (dmax == 0.0) { it = kLassoMaxSweeps - 1; break; }   // nothing moved: every later sweep is this one again
    if (it == kLassoMaxSweeps - 1) break;
    // the sweep left row 0 in nxt (in wraps to 0 after the last feature)
  }
  int bad = 0;
#pragma unroll
  for (int k = 0; k < kLassoSlots; ++k) {
    const int j = lane + 64 * k;
    if (k < ns && j < nf) {
      out[j] = w[k];
      if (!isfinite(w[k])) bad = 1;
    }
  }
  bad = __any(bad);
  if (lane == 0) {
    status[id] = bad ? 1 : 0;
    sweeps[id] = it + 1;
    margins[2 * id] = mgap;
    margins[2 * id + 1] = mratio;
  }
}

}  // namespace ampc
#endif
