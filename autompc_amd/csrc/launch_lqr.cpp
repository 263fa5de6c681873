// launch_lqr.cpp -- launchers of the LQR kernels (lqr_kernels.hpp).  f64 only: compiled once (csrc/build.py).
#include "host_common.hpp"
#include "lqr_kernels.hpp"

// Riccati gains of n problems, descriptors and launch order already on the device.  status [2 n]: status, then the
// Riccati updates performed.
int lqr_launch_gains(hipStream_t st, int n, const void* descs, const void* order, void* ws, const void* cost,
                     void* kout, void* status) {
  hipLaunchKernelGGL(lqr_gains_kernel, dim3(n), dim3(kLqrThreads), 0, st, (const LqrDesc*)descs,
                     (const int*)order, (double*)ws, (const double*)cost, (double*)kout, (int*)status);
  HIP_OK(hipGetLastError());
  return 0;
}

// Controller step of B candidates (the state buffers alternate: `cur` holds the state on entry).
int lqr_launch_ctrl(hipStream_t st, int B, const void* descs, void* states, int cur, const void* sim, int snx,
                    int no, int nu, void* u, const void* kbuf, const void* gbuf, const void* lbuf, const void* lo,
                    const void* hi) {
  hipLaunchKernelGGL(lqr_ctrl_kernel, dim3(B), dim3(kLqrThreads), 0, st, (const LqrLoopDesc*)descs,
                     (double*)states, cur, (const double*)sim, snx, no, nu, (double*)u, (const double*)kbuf,
                     (const double*)gbuf, (const double*)lbuf, (const double*)lo, (const double*)hi);
  HIP_OK(hipGetLastError());
  return 0;
}

int lqr_launch_record(hipStream_t st, int B, const void* next, const void* u, void* sim, void* tobs, void* tctl,
                      int snx, int no, int nu, int T1, int step) {
  const int n = B * (snx > nu ? snx : nu);
  hipLaunchKernelGGL(lqr_record_kernel, dim3((n + 255) / 256), dim3(256), 0, st, (const double*)next,
                     (const double*)u, (double*)sim, (double*)tobs, (double*)tctl, B, snx, no, nu, T1, step);
  HIP_OK(hipGetLastError());
  return 0;
}

size_t lqr_desc_bytes() { return sizeof(LqrDesc); }
size_t lqr_loop_desc_bytes() { return sizeof(LqrLoopDesc); }

// host-side descriptor packing (the layouts live with the kernels)
void lqr_pack_desc(void* dst, int n, int nu, int no, int horizon, int id, const double* ab, long long ws,
                   long long cost, long long k, double threshold, int max_iter) {
  LqrDesc d{};
  d.n = n; d.nu = nu; d.no = no; d.horizon = horizon; d.id = id;
  d.ab = ab; d.ws = ws; d.cost = cost; d.k = k;
  d.threshold = threshold; d.max_iter = max_iter;
  std::memcpy(dst, &d, sizeof d);
}

void lqr_pack_loop_desc(void* dst, int n, int rule, int n_basis, int noclip, const double* ab, long long s,
                        long long k, long long goal, long long lift) {
  LqrLoopDesc d{};
  d.n = n; d.rule = rule; d.n_basis = n_basis; d.noclip = noclip;
  d.ab = ab; d.s = s; d.k = k; d.goal = goal; d.lift = lift;
  std::memcpy(dst, &d, sizeof d);
}
