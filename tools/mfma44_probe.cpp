// Probe the lane layout and issue rate of v_mfma_f64_4x4x4_4b_f64 on this GPU (one-hot inputs), and the
// swapped-operand ("transposed layer") use of it and of v_mfma_f64_16x16x4_f64 that TileNet::CHAIN relies on, and the
// bias as the last link of the 16x16x4's k chain (TileNet::BIAS0_IN_K): fma(b, 1.0, acc) against a separate add.
// Build: hipcc --offload-arch=gfx950 -O2 tools/mfma44_probe.cpp -o variants/mfma44_probe
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
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

// The bias through the last K column.  One block per trial; a = first operand [i = l%16][k = l/16], b = second operand
// [k = l/16][j = l%16], c = the accumulator going in (register r of lane l = [row l/16 + 4 r][col l%16]).
__global__ void bias_link(const double* a, const double* b, const double* c, double* d) {
  const int l = threadIdx.x, t = blockIdx.x;
  typedef double d4_t __attribute__((ext_vector_type(4)));
  d4_t acc;
  for (int i = 0; i < 4; ++i) acc[i] = c[256 * t + 4 * l + i];
  acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[64 * t + l], b[64 * t + l], acc, 0, 0, 0);
  for (int i = 0; i < 4; ++i) d[256 * t + 4 * l + i] = acc[i];
}

// Column k = 3 of one operand holds 1.0, of the other the bias of its row (weights first, TileNet::CHAIN's order) or
// column (weights second).  Expected: the k-ordered fma chain over k = 0..2 on the incoming accumulator, then a
// SEPARATE add of the bias -- what the epilogue's v_add_f64 gave.  Biases of 1e-8 .. 1e8 times the sum's magnitude.
static int check_bias_link(bool weights_first) {
  const int trials = 1024;
  std::vector<double> ha(64 * trials), hb(64 * trials), hc(256 * trials), hd(256 * trials), bias(16 * trials);
  srand(weights_first ? 1 : 2);
  auto rnd = [] { return 2.0 * rand() / RAND_MAX - 1.0; };
  for (int t = 0; t < trials; ++t) {
    const double mag = pow(10.0, (t % 17) - 8);          // bias / sum: 1e-8 .. 1e8
    for (int u = 0; u < 16; ++u) bias[16 * t + u] = mag * rnd();
    for (int l = 0; l < 64; ++l) {
      const int k = l / 16, n = l % 16;
      const double w = k == 3 ? bias[16 * t + n] : rnd(), x = k == 3 ? 1.0 : rnd();
      ha[64 * t + l] = weights_first ? w : x;
      hb[64 * t + l] = weights_first ? x : w;
    }
    for (int e = 0; e < 256; ++e) hc[256 * t + e] = (t & 1) ? rnd() : 0.0;    // (layer 0's last k-step / its only one)
  }
  double *da, *db, *dc, *dd;
  hipMalloc(&da, ha.size() * 8); hipMalloc(&db, hb.size() * 8); hipMalloc(&dc, hc.size() * 8); hipMalloc(&dd, hd.size() * 8);
  hipMemcpy(da, ha.data(), ha.size() * 8, hipMemcpyHostToDevice); hipMemcpy(db, hb.data(), hb.size() * 8, hipMemcpyHostToDevice);
  hipMemcpy(dc, hc.data(), hc.size() * 8, hipMemcpyHostToDevice);
  bias_link<<<trials, 64>>>(da, db, dc, dd);
  hipMemcpy(hd.data(), dd, hd.size() * 8, hipMemcpyDeviceToHost);
  hipFree(da); hipFree(db); hipFree(dc); hipFree(dd);
  int bad = 0;
  for (int t = 0; t < trials; ++t)
    for (int l = 0; l < 64; ++l)
      for (int r = 0; r < 4; ++r) {
        const int row = l / 16 + 4 * r, col = l % 16;     // D[row][col] = sum_k A[row][k] B[k][col]
        volatile double s = hc[256 * t + 4 * l + r];
        for (int k = 0; k < 3; ++k) s = __builtin_fma(ha[64 * t + 16 * k + row], hb[64 * t + 16 * k + col], s);
        const volatile double b = bias[16 * t + (weights_first ? row : col)];
        const volatile double want = s + b;               // the separate add
        if (hd[256 * t + 4 * l + r] != want) ++bad;
      }
  printf("bias as the last link of the 16x16x4 k chain, weights as the %s operand: %d mismatches in %d values against "
         "the k-ordered fma chain followed by a separate add\n", weights_first ? "first" : "second", bad, 256 * trials);
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
  check_bias_link(true);
  check_bias_link(false);
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
