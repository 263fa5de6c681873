// sindyfit_frame.hpp -- what the two kernel families of the thresholded SINDy fit share (sindyfit_kernels.hpp: up to
// 272 features; sindyfit_wide_kernels.hpp: up to 2048): the per-column rule of [Theta | Y] and its evaluation, the
// Gram pass's view of the data, the descriptor of a (configuration, target) pair.  No kernels.
#ifndef AMPC_SINDYFIT_FRAME_HPP
#define AMPC_SINDYFIT_FRAME_HPP
#include <hip/hip_runtime.h>

#include "gram_frame.hpp"
#include "sindy_kernels.hpp"

namespace ampc {

constexpr int kSindyfitMaxState = 64, kSindyfitMaxCtrl = 16;

enum { SFC_NEXT_OBS = 7, SFC_YCONT = 8, SFC_ZERO = 9 };   // column kinds behind the library's SF_* kinds

// How one column of [Theta | Y] is formed from a data row.
struct SindyfitCol {
  int kind;     // SF_ID .. SF_MONO: a library feature; SFC_NEXT_OBS: obs[t + 1][a0]; SFC_YCONT: ycont[t][a0]; SFC_ZERO
  int a0, a1;   // variables (index into [obs | ctrls]); SF_MONO: first (variable, exponent) pair and their number
  int pad;
  double par;   // frequency / exponent
  __host__ __device__ static SindyfitCol zero() { return SindyfitCol{SFC_ZERO, 0, 0, 0, 0.0}; }     // a padding column
};

struct SindyfitDesign;

struct SindyfitGramArgs {
  const double* obs;          // [R][nx]
  const double* ctrls;        // [R][nu]
  const double* ycont;        // [R][nx] or nullptr (no design has continuous targets then)
  const int* row_start;       // [R]: first row of the row's trajectory; -1: the row has no successor (no design row)
  const SindyfitDesign* designs;
  int R, nx, nu, splits;
};

__device__ inline double sindyfit_var(const SindyfitGramArgs& a, int g, int i) {
  return i < a.nx ? a.obs[(size_t)g * a.nx + i] : a.ctrls[(size_t)g * a.nu + (i - a.nx)];
}

__device__ inline double sindyfit_value(const SindyfitGramArgs& a, const SindyfitCol c, const int* __restrict__ pool,
                                        int g) {
  if (c.kind == SFC_ZERO) return 0.0;
  if (c.kind == SFC_NEXT_OBS) return a.obs[(size_t)(g + 1) * a.nx + c.a0];
  if (c.kind == SFC_YCONT) return a.ycont[(size_t)g * a.nx + c.a0];
  if (c.kind == SF_MONO) {
    double val = 1.0;
    for (int j = 0; j < c.a1; ++j)
      val *= sindy_ipow<double>(sindyfit_var(a, g, pool[2 * (c.a0 + j)]), pool[2 * (c.a0 + j) + 1]);
    return val;
  }
  return sindy_feature<double>(c.kind, sindyfit_var(a, g, c.a0), sindyfit_var(a, g, c.a1), c.par);
}

// One (configuration, target) pair.  Read field by field through a global pointer (uniform loads).
struct SindyfitSolveDesc {
  int n, tcol, id, pad;       // features, the target's column of G, output slot (pair index)
  const double* g;            // the design's Gram [.][ldg]
  long long ldg;
  long long ws;               // workspace offset (doubles): [n + 1][n]
  long long out;              // coefficient offset (doubles): [n]
  double threshold;
};

}  // namespace ampc
#endif
