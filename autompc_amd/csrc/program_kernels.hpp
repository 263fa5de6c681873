// program_kernels.hpp -- analytic dynamics as a straight-line program (ampc_set_program): x' = f(x, u) written as
// a list of three-address instructions over value slots, interpreted one row per lane.
//
//   instruction word  (op, dst, a, b)          slots 0 .. nx+nu-1 hold the row's [x | u] on entry
//     PO_CONST  v[dst] = consts[a]             PO_SIN .. PO_TANH  v[dst] = f(v[a])  (device library, full precision)
//     PO_ADD / SUB / MUL / DIV / MIN / MAX     v[dst] = v[a] op v[b]
//     PO_NEG / PO_ABS                          v[dst] = -v[a], |v[a]|
//     PO_POWI   v[dst] = v[a] ** b             b an integer in -64..64: repeated multiplication, left to right
//     PO_SIGN   v[dst] = sign(v[a])            -1, 0 or +1, NaN stays NaN      } exact; in derived (JVP) programs:
//     PO_LT     v[dst] = v[a] < v[b] ? 1 : 0                                   } the tangents of abs, min and max
//   output i of the row is v[out_slot[i]].
//
// Rounding contract: every instruction rounds once, in T, in list order -- contraction is off in the interpreter, so
// a * b + c stays two roundings as in the host evaluation (sysid/program.py), and add / sub / mul / div / sqrt / abs /
// min / max / integer power agree with numpy bit for bit.
//
// LDS: the slots are [slot][lane] (consecutive lanes on consecutive words: no bank conflicts), n_slots * 64 * sizeof(T)
// bytes; the rollout adds [nx][lane] for the hand-over of a step's outputs.  With the limits below the largest request
// is (256 + 64) * 64 * 8 bytes = 160 KB, exactly what a workgroup can have.  The instruction words, the constant pool
// and out_slot are indexed by wave-uniform values only, so they arrive through scalar loads and the opcode switch is
// a scalar branch; every result leaves through ordinary vector stores.
//
// Jacobians: a handle may hold, beside its program, the program's JVP (ampc_set_program_jvp; derived on the host,
// sysid/program.py): 2 (nx + nu) inputs [x | u | dx | du], 2 nx outputs [f | J . (dx, du)], the same instruction set,
// run by the same interpreter.  program_jacobian_kernel gives every (row, unit direction) pair a lane;
// ilqr_program_jacobian_kernel does the same for the rows of an iLQR plan's nominal trajectories (one shared body:
// program_jacobian_lane).  The interpreter takes the column stride as a template parameter: 64 here, 16 where the
// iLQR line search keeps one column per candidate row (ilqr_kernels.hpp, DYN = 3).
#pragma once
#include <hip/hip_runtime.h>
#include "mlp_kernels.hpp"             // RowMap: the rows of an iLQR plan

namespace ampc {

enum ProgOp {
  PO_CONST = 0, PO_ADD, PO_SUB, PO_MUL, PO_DIV, PO_NEG, PO_SIN, PO_COS, PO_EXP, PO_SQRT, PO_ABS, PO_TANH, PO_POWI,
  PO_MIN, PO_MAX, PO_SIGN, PO_LT, PO_COUNT
};

static constexpr int kProgMaxSlots = 256;    // value slots of a program (inputs included)
static constexpr int kProgMaxInstr = 4096;   // instructions of a program
static constexpr int kProgMaxNx = 64;        // outputs / states
static constexpr int kProgMaxPow = 64;       // |exponent| of PO_POWI
static constexpr int kProgLanes = 64;        // rows per workgroup: one wave

template <typename T> struct ProgDev {
  int nx, nu, n_slots, n_instr;
  const int4* code;        // [n_instr] (op, dst, a, b)
  const T* consts;         // [n_const]
  const int* out_slot;     // [nx]
};

__device__ __forceinline__ double prog_sin(double x) { return sin(x); }
__device__ __forceinline__ float prog_sin(float x) { return sinf(x); }
__device__ __forceinline__ double prog_cos(double x) { return cos(x); }
__device__ __forceinline__ float prog_cos(float x) { return cosf(x); }
__device__ __forceinline__ double prog_exp(double x) { return exp(x); }
__device__ __forceinline__ float prog_exp(float x) { return expf(x); }
__device__ __forceinline__ double prog_tanh(double x) { return tanh(x); }
__device__ __forceinline__ float prog_tanh(float x) { return tanhf(x); }
__device__ __forceinline__ double prog_sqrt(double x) { return sqrt(x); }     // (correctly rounded, as is T's '/')
__device__ __forceinline__ float prog_sqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ double prog_abs(double x) { return fabs(x); }
__device__ __forceinline__ float prog_abs(float x) { return fabsf(x); }

// The interpreter: v points at the lane's column of the [slot][S] array.  Straight line, no barrier: a lane
// touches its own column only.
template <typename T, int S = kProgLanes> __device__ __forceinline__ void program_run(const ProgDev<T>& p, T* v) {
#pragma clang fp contract(off)
  for (int i = 0; i < p.n_instr; ++i) {
    const int4 w = p.code[i];
    T r;
    if (w.x == PO_CONST) {
      r = p.consts[w.z];
    } else {
      const T a = v[w.z * S];
      switch (w.x) {
        case PO_ADD: r = a + v[w.w * S]; break;
        case PO_SUB: r = a - v[w.w * S]; break;
        case PO_MUL: r = a * v[w.w * S]; break;
        case PO_DIV: r = a / v[w.w * S]; break;
        case PO_MIN: { const T b = v[w.w * S]; r = (b != b || b < a) ? b : a; } break;   // (NaN propagates, as np.minimum)
        case PO_MAX: { const T b = v[w.w * S]; r = (b != b || b > a) ? b : a; } break;
        case PO_NEG: r = -a; break;
        case PO_SIN: r = prog_sin(a); break;
        case PO_COS: r = prog_cos(a); break;
        case PO_EXP: r = prog_exp(a); break;
        case PO_SQRT: r = prog_sqrt(a); break;
        case PO_ABS: r = prog_abs(a); break;
        case PO_TANH: r = prog_tanh(a); break;
        case PO_SIGN: r = a > (T)0 ? (T)1 : (a < (T)0 ? (T)-1 : (a == (T)0 ? (T)0 : a)); break;   // (as np.sign)
        case PO_LT: r = a < v[w.w * S] ? (T)1 : (T)0; break;
        default: {                               // PO_POWI: ((a * a) * a) * ..., then the reciprocal of that
          const int e = w.w < 0 ? -w.w : w.w;
          r = e == 0 ? (T)1 : a;
          for (int k = 1; k < e; ++k) r = r * a;
          if (w.w < 0) r = (T)1 / r;
        } break;
      }
    }
    v[w.y * S] = r;
  }
}

// x_next[r] = f(x[r], u[r]) for B rows, one row per lane.  A row's inputs are all in LDS before its first output is
// written, so x_next may be x.  Rows at or past B neither read nor write.
template <typename T>
__global__ __launch_bounds__(kProgLanes) void program_forward_kernel(const ProgDev<T> p, const T* x, const T* u,
                                                                     T* x_next, int B) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  constexpr int S = kProgLanes;
  T* v = reinterpret_cast<T*>(smem_raw) + threadIdx.x;
  const long long r = (long long)blockIdx.x * S + threadIdx.x;
  if (r >= B) return;
  for (int i = 0; i < p.nx; ++i) v[i * S] = x[r * p.nx + i];
  for (int j = 0; j < p.nu; ++j) v[(p.nx + j) * S] = u[r * p.nu + j];
  program_run<T>(p, v);
  for (int i = 0; i < p.nx; ++i) x_next[r * p.nx + i] = v[p.out_slot[i] * S];
}

// obs[n][0] = x0[n], obs[n][t+1] = f(obs[n][t], ctrls[n][t]): one lane per trajectory, the state stays in LDS between
// steps.  A step's outputs go through a second LDS area [nx][lane] before they become the next inputs, so an output
// that is an input slot, or a permutation of the inputs, reads nothing already overwritten.
template <typename T>
__global__ __launch_bounds__(kProgLanes) void program_rollout_kernel(const ProgDev<T> p, const T* __restrict__ x0,
                                                                     const T* __restrict__ ctrls, T* __restrict__ obs,
                                                                     int n, int n_steps) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  constexpr int S = kProgLanes;
  T* v = reinterpret_cast<T*>(smem_raw) + threadIdx.x;
  T* hand = v + (size_t)p.n_slots * S;
  const long long r = (long long)blockIdx.x * S + threadIdx.x;
  if (r >= n) return;
  const int nx = p.nx, nu = p.nu;
  T* row = obs + r * (n_steps + 1) * nx;
  const T* uc = ctrls + r * n_steps * nu;
  for (int i = 0; i < nx; ++i) { const T x = x0[r * nx + i]; v[i * S] = x; row[i] = x; }
  for (int t = 0; t < n_steps; ++t) {
    for (int j = 0; j < nu; ++j) v[(nx + j) * S] = uc[(long long)t * nu + j];
    program_run<T>(p, v);
    for (int i = 0; i < nx; ++i) hand[i * S] = v[p.out_slot[i] * S];
    row += nx;
    for (int i = 0; i < nx; ++i) { const T x = hand[i * S]; v[i * S] = x; row[i] = x; }
  }
}

// One (row, unit direction j) pair of the JVP program q on the lane's column v: [x | u] of the row into slots
// 0 .. nv-1 (nv = nx + nu), the unit seed e_j into slots nv .. 2nv-1, q, then column j of the row's Jacobian --
// Jx[i][j] for j < nx, Ju[i][j - nx] otherwise; with `out`, the j == 0 lane also writes the value outputs.  The
// values are recomputed per direction: one interpreter, one rounding contract, for every kernel that calls this.
template <typename T>
__device__ __forceinline__ void program_jacobian_lane(const ProgDev<T>& q, T* v, const T* __restrict__ x,
                                                      const T* __restrict__ u, int j, T* __restrict__ out,
                                                      T* __restrict__ Jx, T* __restrict__ Ju, int nx, int nu) {
  constexpr int S = kProgLanes;
  const int nv = nx + nu;
  for (int i = 0; i < nx; ++i) v[i * S] = x[i];
  for (int i = 0; i < nu; ++i) v[(nx + i) * S] = u[i];
  for (int i = 0; i < nv; ++i) v[(nv + i) * S] = i == j ? (T)1 : (T)0;
  program_run<T>(q, v);
  if (out != nullptr && j == 0)
    for (int i = 0; i < nx; ++i) out[i] = v[q.out_slot[i] * S];
  if (j < nx) {
    for (int i = 0; i < nx; ++i) Jx[i * nx + j] = v[q.out_slot[nx + i] * S];
  } else {
    for (int i = 0; i < nx; ++i) Ju[i * nu + (j - nx)] = v[q.out_slot[nx + i] * S];
  }
}

// (next, jx, ju) of B rows from the JVP program q (header comment): lane l of the launch is row l / nv, direction
// l % nv (program_jacobian_lane).  Lanes at or past B * nv return before touching memory.
template <typename T>
__global__ __launch_bounds__(kProgLanes) void program_jacobian_kernel(const ProgDev<T> q, const T* __restrict__ x,
                                                                      const T* __restrict__ u, T* __restrict__ out,
                                                                      T* __restrict__ jx, T* __restrict__ ju, int B,
                                                                      int nx, int nu) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* v = reinterpret_cast<T*>(smem_raw) + threadIdx.x;
  const int nv = nx + nu;
  const long long l = (long long)blockIdx.x * kProgLanes + threadIdx.x;
  if (l >= (long long)B * nv) return;
  const long long r = l / nv;
  program_jacobian_lane<T>(q, v, x + r * nx, u + r * nu, (int)(l - r * nv), out + r * nx, jx + r * nx * nx,
                           ju + r * nx * nu, nx, nu);
}

// The Jacobian refresh of an iLQR plan on a program (launch_mlp.cpp): lane l is (plan row l / nv, direction l % nv),
// n plan rows in all.  A row is read and written through the plan's RowMap as the other refresh kernels do: slot
// rm.group(r), step rm.step(r), states [slot][H + 1][nx], ctrls [slot][H][nu], output row rm.out_row(r) of jx / ju.
// Rows of slots that did not ask for a refresh, rows past a slot's horizon and lanes past n * nv neither read nor write.
template <typename T>
__global__ __launch_bounds__(kProgLanes) void ilqr_program_jacobian_kernel(const ProgDev<T> q,
                                                                           const T* __restrict__ states,
                                                                           const T* __restrict__ ctrls,
                                                                           T* __restrict__ jx, T* __restrict__ ju,
                                                                           int n, const RowMap rm) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* v = reinterpret_cast<T*>(smem_raw) + threadIdx.x;
  const int nx = q.nx, nu = q.nu, nv = nx + nu;
  const long long l = (long long)blockIdx.x * kProgLanes + threadIdx.x;
  if (l >= (long long)n * nv) return;
  const int r = (int)(l / nv);
  if (!rm.live(r)) return;
  const T* x = states + (size_t)rm.group(r) * rm.s_stride + (size_t)rm.step(r) * nx;
  const T* u = ctrls + (size_t)rm.group(r) * rm.c_stride + (size_t)rm.step(r) * nu;
  const size_t o = (size_t)rm.out_row(r);
  program_jacobian_lane<T>(q, v, x, u, (int)(l - (long long)r * nv), (T*)nullptr, jx + o * nx * nx, ju + o * nx * nu,
                           nx, nu);
}

}  // namespace ampc
