// Probe the lane layout and issue rate of v_mfma_f64_4x4x4_4b_f64 on this GPU (one-hot inputs), and the
// swapped-operand ("transposed layer") use of it and of v_mfma_f64_16x16x4_f64 that TileNet::CHAIN relies on.
// Build: hipcc --offload-arch=gfx950 -O2 tools/mfma44_probe.cpp -o variants/mfma44_probe
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>

__global__ void probe(const double* a, const double* b, double* d) {
  const int l = threadIdx.x;
  d[l] = __builtin_amdgcn_mfma_f64_4x4x4f64(a[l], b[l], 0.0, 0, 0, 0);
}

// Swapped operands.  w = the packed WEIGHT fragment W[k = l/16][n = l%16], x = the ACTIVATION fragment
// act[row = l%16][k = l/16] (the layouts the tile feeds as B and A).  mfma(w, x) must leave
//   16x16x4: register r of lane l = sum_k W[k][unit = l/16 + 4 r] * act[sample = l%16][k]
// i.e. [unit 4 r + q][sample i] -- the activation fragment of k-step r of a layer that consumes these units;
//   4x4x4:   lane l = sum_k Wt[k][col = l/16] * act[sample = l%16][k]   with wt packed W[k = l/16][col = l%4].
__global__ void swapped(const double* w, const double* x, const double* wt, double* d16, double* d4) {
  const int l = threadIdx.x;
  typedef double d4_t __attribute__((ext_vector_type(4)));
  const d4_t r = __builtin_amdgcn_mfma_f64_16x16x4f64(w[l], x[l], d4_t{0, 0, 0, 0}, 0, 0, 0);
  for (int i = 0; i < 4; ++i) d16[4 * l + i] = r[i];
  d4[l] = __builtin_amdgcn_mfma_f64_4x4x4f64(wt[l], x[l], 0.0, 0, 0, 0);
}

static int check_swapped() {
  double W[4][16], X[16][4], hw[64], hx[64], hwt[64], h16[256], h4[64];
  for (int k = 0; k < 4; ++k) for (int n = 0; n < 16; ++n) W[k][n] = 1.0 + 0.37 * k - 0.11 * n + 0.013 * k * n;
  for (int i = 0; i < 16; ++i) for (int k = 0; k < 4; ++k) X[i][k] = 0.5 - 0.21 * i + 0.77 * k - 0.019 * i * k;
  for (int l = 0; l < 64; ++l) { hw[l] = W[l / 16][l % 16]; hx[l] = X[l % 16][l / 16]; hwt[l] = W[l / 16][l % 4]; }
  double *dw, *dx, *dwt, *d16, *d4;
  hipMalloc(&dw, 512); hipMalloc(&dx, 512); hipMalloc(&dwt, 512); hipMalloc(&d16, 2048); hipMalloc(&d4, 512);
  hipMemcpy(dw, hw, 512, hipMemcpyHostToDevice); hipMemcpy(dx, hx, 512, hipMemcpyHostToDevice);
  hipMemcpy(dwt, hwt, 512, hipMemcpyHostToDevice);
  swapped<<<1, 64>>>(dw, dx, dwt, d16, d4);
  hipMemcpy(h16, d16, 2048, hipMemcpyDeviceToHost); hipMemcpy(h4, d4, 512, hipMemcpyDeviceToHost);
  int bad = 0;
  for (int l = 0; l < 64; ++l) {
    const int i = l % 16, q = l / 16;
    for (int r = 0; r < 4; ++r) {
      double s = 0;
      for (int k = 0; k < 4; ++k) s = __builtin_fma(W[k][q + 4 * r], X[i][k], s);
      if (h16[4 * l + r] != s) ++bad;
    }
    double s = 0;
    for (int k = 0; k < 4; ++k) s = __builtin_fma(W[k][q], X[i][k], s);
    if (h4[l] != s) ++bad;
  }
  printf("swapped operands: 16x16x4 register r of lane l = [unit l/16 + 4 r][sample l%%16], "
         "4x4x4 lane l = [col l/16][sample l%%16]: %s (%d mismatches against a k-ordered fma chain)\n",
         bad ? "NO" : "yes", bad);
  return bad;
}

__global__ void rate(double* out, int iters) {
  double a = 1.0 + threadIdx.x * 1e-9, b = 1.0 - threadIdx.x * 1e-9;
  double c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0, c5 = 0, c6 = 0, c7 = 0;
  for (int i = 0; i < iters; ++i) {
    c0 = __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, c0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, c1, 0, 0, 0);
    c2 = __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, c2, 0, 0, 0);
    c3 = __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, c3, 0, 0, 0);
    c4 = __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, c4, 0, 0, 0);
    c5 = __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, c5, 0, 0, 0);
    c6 = __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, c6, 0, 0, 0);
    c7 = __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, c7, 0, 0, 0);
  }
  out[blockIdx.x * blockDim.x + threadIdx.x] = c0 + c1 + c2 + c3 + c4 + c5 + c6 + c7;
}

int main() {
  check_swapped();
  double *da, *db, *dd;
  hipMalloc(&da, 64 * 8); hipMalloc(&db, 64 * 8); hipMalloc(&dd, 64 * 8);
  // For every (la, lb): which output lanes see a[la]*b[lb]?
  std::vector<double> ha(64), hb(64), hd(64);
  printf("A lane -> (pairs with B lanes) -> D lanes\n");
  for (int la = 0; la < 64; ++la) {
    for (int lb = 0; lb < 64; ++lb) {
      for (int i = 0; i < 64; ++i) { ha[i] = 0; hb[i] = 0; }
      ha[la] = 1; hb[lb] = 1;
      hipMemcpy(da, ha.data(), 512, hipMemcpyHostToDevice);
      hipMemcpy(db, hb.data(), 512, hipMemcpyHostToDevice);
      probe<<<1, 64>>>(da, db, dd);
      hipMemcpy(hd.data(), dd, 512, hipMemcpyDeviceToHost);
      for (int i = 0; i < 64; ++i)
        if (hd[i] != 0) printf("a%d b%d -> d%d\n", la, lb, i);
    }
  }
  // issue rate: 8 independent accumulators, 2 waves per SIMD on every CU
  double* out;
  const int blocks = 256 * 2, thr = 256, iters = 20000;
  hipMalloc(&out, (size_t)blocks * thr * 8);
  rate<<<blocks, thr>>>(out, 100);
  hipDeviceSynchronize();
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  hipEventRecord(e0);
  rate<<<blocks, thr>>>(out, iters);
  hipEventRecord(e1); hipEventSynchronize(e1);
  float ms; hipEventElapsedTime(&ms, e0, e1);
  const double mfmas = (double)blocks * (thr / 64) * iters * 8;
  printf("4x4x4 f64: %.3f ms, %.1f TFLOP/s (512 flop each), %.1f cycles per MFMA per SIMD at 2.4 GHz\n", ms,
         mfmas * 512 / (ms * 1e-3) / 1e12, (ms * 1e-3) * 2.4e9 / (mfmas / (256 * 4)));
  return 0;
}
