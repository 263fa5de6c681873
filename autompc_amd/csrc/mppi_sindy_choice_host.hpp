// mppi_sindy_choice_host.hpp -- which rollout kernel a single-model SINDy MPPI plan launches, and with how much LDS
// (launch_mppi.cpp takes the decision from here; ampc_mppi_plan_set_geometry, ampc_mppi_plan_sindy_launch and the
// device-free ampc_mppi_sindy_launch_choice report it), and the LDS need of sindy_forward_kernel (api_model.cpp).
// No device call and no HIP type: a stand-alone host program can include it.
#pragma once
#include <cstddef>

// What the decision reads of a handle that holds a SINDy model and of the plan on it.
struct MppiSindyShape {
  int esz;               // bytes of the compute type (8 / 4)
  int nx, nu, n_tab;     // n_tab == 0: direct evaluation (no product table)
  size_t stage_bytes;    // sindy_stage_bytes of the handle: 0 when the program is not copied to LDS
  int cost_stride;       // elements of one cost block
  int max_h;             // the plan's horizon cap
  long long samples;     // 64 x the plan's tiles
};

struct MppiSindyChoice {
  int spread;            // 1: mppi_rollout_sindy_fp_kernel (features spread over lanes), 0: mppi_rollout_sindy_kernel
  int lanes;             // lanes per sample: 16 / 32 / 64 lane-spread, 1 one thread per sample
  int staged;            // the launched kernel copies the feature program to LDS
  size_t lds_bytes;      // dynamic LDS of the launch, the staged program included
};

// Bytes of the staged program (sindy_stage_bytes) from the elements sindy_prog_elems counts.
inline size_t sindy_stage_bytes_of(size_t prog_elems, int n_tab, int esz, size_t stage_limit) {
  if (n_tab == 0) return 0;
  const size_t b = prog_elems * (size_t)esz;
  return b <= stage_limit ? b + 2 * (size_t)esz : 0;
}

// sindy_forward_kernel: per-thread columns [x|u], next x, value table for 64 threads, then the staged program.
inline size_t sindy_forward_lds_bytes(int esz, int nx, int nu, int n_tab, size_t stage_bytes) {
  return (size_t)(2 * nx + nu + n_tab) * 64 * (size_t)esz + stage_bytes;
}

// mppi_rollout_sindy_kernel: the same columns, the shared cost block and bounds, then the staged program.
inline size_t mppi_sindy_thread_lds_bytes(const MppiSindyShape& s, size_t stage_bytes) {
  return ((size_t)(2 * s.nx + s.nu + s.n_tab) * 64 + s.cost_stride + 3 * s.nu + 2) * (size_t)s.esz + stage_bytes;
}

// Elements of a sample's noise row / shifted action sequence in the lane-spread kernel.
inline int mppi_sindy_hcap(int max_h, int nu) { return (max_h * nu + 3) / 4 * 4; }

// mppi_rollout_sindy_fp_kernel with G lanes per sample: 64 / G samples of (x|u, table, noise row, shifted actions).
inline size_t mppi_sindy_spread_lds_bytes(const MppiSindyShape& s, int G) {
  const int hcap = mppi_sindy_hcap(s.max_h, s.nu);
  return ((size_t)(64 / G) * (s.nx + s.nu + s.n_tab + 2 * hcap) + s.cost_stride + 3 * s.nu + 2) * (size_t)s.esz +
         s.stage_bytes;
}

// fp_allowed: AMPC_SINDY_FP != 0; g_forced: AMPC_SINDY_G (16 / 32 / 64 override the lanes, anything else does not).
//  * lane-spread when the program is staged, has a product table and at most eight states, and the map fits;
//    lanes per sample: all 64 while that still leaves the chip waves to spare, else 32 / 16
//  * else one thread per sample; when the columns fit but the staged program on top of them does not, the kernel
//    runs from global memory (an unstaged descriptor) instead of asking for more LDS than a workgroup can have
// A result with lds_bytes > lds_limit means that the columns alone do not fit: the caller refuses.
inline MppiSindyChoice mppi_sindy_choice(const MppiSindyShape& s, int fp_allowed, int g_forced, size_t lds_limit) {
  int G = s.samples <= 2048 ? 64 : (s.samples <= 8192 ? 32 : 16);
  if (g_forced == 16 || g_forced == 32 || g_forced == 64) G = g_forced;
  const size_t lbf = mppi_sindy_spread_lds_bytes(s, G);
  if (fp_allowed && s.stage_bytes > 0 && s.n_tab > 0 && s.nx <= 8 && lbf <= lds_limit) return {1, G, 1, lbf};
  const size_t lb = mppi_sindy_thread_lds_bytes(s, s.stage_bytes);
  if (s.stage_bytes > 0 && lb > lds_limit) return {0, 1, 0, mppi_sindy_thread_lds_bytes(s, 0)};
  return {0, 1, s.stage_bytes > 0 ? 1 : 0, lb};
}
