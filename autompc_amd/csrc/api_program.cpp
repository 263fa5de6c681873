// api_program.cpp -- analytic dynamics as a straight-line program on a handle: ampc_set_program and
// ampc_set_program_jvp (validation on the host, staging), ampc_program_set_ilqr (the iLQR opt-in), the batched
// prediction and the Jacobians of such a handle and ampc_program_rollout (program_kernels.hpp).
//
// A malformed program never reaches a kernel: every opcode, slot, constant index, definition-before-use and limit is
// checked here, before anything is uploaded, and answered with a return code and an ampc_last_error() text.
#include "host_common.hpp"

static const char* const kProgOpNames[PO_COUNT] = {"const", "add", "sub", "mul", "div", "neg", "sin", "cos", "exp",
                                                   "sqrt", "abs", "tanh", "powi", "min", "max", "sign", "lt"};

static bool prog_is_binary(int op) {
  return op == PO_ADD || op == PO_SUB || op == PO_MUL || op == PO_DIV || op == PO_MIN || op == PO_MAX || op == PO_LT;
}

// Everything ampc_set_program (n_in = nx + nu inputs, n_out = nx outputs) and ampc_set_program_jvp (2 (nx + nu) inputs,
// 2 nx outputs) check of the arrays, nothing touched: 0, or the refusal.
static int program_check(const std::string& fn, int n_in, int n_out, int n_slots, int n_instr, const int* code,
                         int n_const, const int* out_slot) {
  REQUIRE(n_slots >= n_in && n_slots <= kProgMaxSlots,
          fn + ": n_slots must cover the " + std::to_string(n_in) + " input slots and be at most " +
              std::to_string(kProgMaxSlots) + " (the slots of 64 rows live in LDS)");
  REQUIRE(n_instr >= 0 && n_instr <= kProgMaxInstr, fn + ": at most " + std::to_string(kProgMaxInstr) + " instructions");
  REQUIRE(n_const >= 0 && n_const <= kProgMaxInstr, fn + ": at most 4096 constants");
  std::vector<char> defined(n_slots, 0);
  for (int i = 0; i < n_in; ++i) defined[i] = 1;
  for (int i = 0; i < n_instr; ++i) {
    const int op = code[4 * i], dst = code[4 * i + 1], a = code[4 * i + 2], b = code[4 * i + 3];
    const std::string at = fn + ": instruction " + std::to_string(i);
    REQUIRE(op >= 0 && op < PO_COUNT, at + ": unknown opcode " + std::to_string(op));
    const std::string who = at + " (" + kProgOpNames[op] + ")";
    REQUIRE(dst >= 0 && dst < n_slots, who + ": destination slot outside 0..n_slots-1");
    if (op == PO_CONST) {
      REQUIRE(a >= 0 && a < n_const, who + ": constant index outside 0..n_const-1");
    } else {
      REQUIRE(a >= 0 && a < n_slots, who + ": operand slot outside 0..n_slots-1");
      REQUIRE(defined[a], who + ": reads slot " + std::to_string(a) + " before anything wrote it");
      if (prog_is_binary(op)) {
        REQUIRE(b >= 0 && b < n_slots, who + ": operand slot outside 0..n_slots-1");
        REQUIRE(defined[b], who + ": reads slot " + std::to_string(b) + " before anything wrote it");
      } else if (op == PO_POWI) {
        REQUIRE(b >= -kProgMaxPow && b <= kProgMaxPow, who + ": exponent outside -64..64");
      }
    }
    defined[dst] = 1;
  }
  for (int i = 0; i < n_out; ++i) {
    REQUIRE(out_slot[i] >= 0 && out_slot[i] < n_slots, fn + ": out_slot[" + std::to_string(i) + "] outside 0..n_slots-1");
    REQUIRE(defined[out_slot[i]], fn + ": out_slot[" + std::to_string(i) + "] names a slot nothing wrote");
  }
  return 0;
}

// code, then out_slot, into `ints`; the constants in the handle's precision into `flts`
static int program_upload(ampc_handle* h, DevBuf* ints_buf, DevBuf* flts, int n_out, int n_instr, const int* code,
                          int n_const, const double* consts, const int* out_slot) {
  HIP_OK(hipSetDevice(h->device));
  std::vector<int> ints(4 * (size_t)n_instr + n_out);
  if (n_instr > 0) std::memcpy(ints.data(), code, 4 * (size_t)n_instr * sizeof(int));
  std::memcpy(ints.data() + 4 * (size_t)n_instr, out_slot, n_out * sizeof(int));
  HIP_OK(hipStreamSynchronize(h->stream));       // (a launch in flight may still read the previous program)
  HIP_OK(ints_buf->reserve(ints.size() * sizeof(int)));
  HIP_OK(hipMemcpy(ints_buf->p, ints.data(), ints.size() * sizeof(int), hipMemcpyHostToDevice));
  HIP_OK(flts->reserve((size_t)(n_const > 0 ? n_const : 1) * h->esz()));
  if (n_const > 0) {
    if (h->precision == AMPC_F64) HIP_OK(upload_converted<double>(flts->p, consts, n_const, h->stream));
    else HIP_OK(upload_converted<float>(flts->p, consts, n_const, h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));
  }
  return 0;
}

extern "C" int ampc_set_program(ampc_handle* h, int nx, int nu, int n_slots, int n_instr, const int* code, int n_const,
                                const double* consts, const int* out_slot) {
  REQUIRE(h && out_slot && (n_instr == 0 || code) && (n_const == 0 || consts), "ampc_set_program: NULL argument");
  REQUIRE(nx >= 1 && nx <= kProgMaxNx && nu >= 1 && nu <= kMaxNu, "ampc_set_program: nx in 1..64, nu in 1..16");
  if (int rc = program_check("ampc_set_program", nx + nu, nx, n_slots, n_instr, code, n_const, out_slot)) return rc;
  if (int rc = program_upload(h, &h->prog_int, &h->prog_flt, nx, n_instr, code, n_const, consts, out_slot)) return rc;
  h->nx = nx; h->nu = nu; h->p_nslots = n_slots; h->p_ninstr = n_instr; h->p_nconst = n_const;
  std::memset(&h->md, 0, sizeof(h->md));
  std::memset(&h->mf, 0, sizeof(h->mf));
  h->md.nx = h->mf.nx = nx; h->md.nu = h->mf.nu = nu; h->md.kin = h->mf.kin = nx + nu;
  h->n_hidden = 0;
  h->lin_n = 0;
  h->has_prog = true;
  h->has_jvp = false;            // (a JVP staged before belongs to the previous program)
  h->prog_ilqr = false;
  h->has_mlp = h->has_sindy = h->has_lin = false;
  return 0;
}

extern "C" int ampc_set_program_jvp(ampc_handle* h, int n_slots, int n_instr, const int* code, int n_const,
                                    const double* consts, const int* out_slot) {
  REQUIRE(h && out_slot && (n_instr == 0 || code) && (n_const == 0 || consts), "ampc_set_program_jvp: NULL argument");
  REQUIRE(h->has_prog, "ampc_set_program_jvp: the handle holds no program (ampc_set_program comes first)");
  const int nx = h->nx, nv = h->nx + h->nu;
  if (int rc = program_check("ampc_set_program_jvp", 2 * nv, 2 * nx, n_slots, n_instr, code, n_const, out_slot)) return rc;
  h->has_jvp = false;
  h->prog_ilqr = false;
  if (int rc = program_upload(h, &h->jvp_int, &h->jvp_flt, 2 * nx, n_instr, code, n_const, consts, out_slot)) return rc;
  h->j_nslots = n_slots; h->j_ninstr = n_instr; h->j_nconst = n_const;
  h->has_jvp = true;
  return 0;
}

extern "C" int ampc_program_set_ilqr(ampc_handle* h, int enable) {
  REQUIRE(h, "ampc_program_set_ilqr: NULL handle");
  REQUIRE(h->has_prog, "ampc_program_set_ilqr: the handle holds no analytic dynamics program (ampc_set_program comes first)");
  REQUIRE(h->has_jvp, "ampc_program_set_ilqr: the handle's program has no JVP staged (ampc_set_program_jvp comes first): "
                      "iLQR linearises its controller model");
  h->prog_ilqr = enable != 0;
  return 0;
}

template <typename T>
static int program_pred_impl(ampc_handle* h, const double* states, const double* ctrls, double* out, int n) {
  const int nx = h->nx, nu = h->nu;
  HIP_OK(h->s_states.reserve((size_t)n * nx * sizeof(T)));
  HIP_OK(h->s_ctrls.reserve((size_t)n * nu * sizeof(T)));
  HIP_OK(h->s_out.reserve((size_t)n * nx * sizeof(T)));
  HIP_OK(upload_converted<T>(h->s_states.p, states, (size_t)n * nx, h->stream));
  HIP_OK(upload_converted<T>(h->s_ctrls.p, ctrls, (size_t)n * nu, h->stream));
  const size_t lb = (size_t)h->p_nslots * kProgLanes * sizeof(T);
  HIP_OK(allow_lds(program_forward_kernel<T>, lb));
  hipLaunchKernelGGL(program_forward_kernel<T>, dim3((n + kProgLanes - 1) / kProgLanes), dim3(kProgLanes), lb, h->stream,
                     prog_of<T>(h), (const T*)h->s_states.p, (const T*)h->s_ctrls.p, (T*)h->s_out.p, n);
  HIP_OK(hipGetLastError());
  HIP_OK(download_converted<T>(out, h->s_out.p, (size_t)n * nx, h->stream));
  return 0;
}

// ampc_mlp_pred_batch on a program handle (api_model.cpp)
int program_pred_batch(ampc_handle* h, const double* states, const double* ctrls, double* out, int n) {
  if (n <= 0) return 0;
  HIP_OK(hipSetDevice(h->device));
  return h->precision == AMPC_F64 ? program_pred_impl<double>(h, states, ctrls, out, n)
                                  : program_pred_impl<float>(h, states, ctrls, out, n);
}

template <typename T>
static int program_diff_impl(ampc_handle* h, const double* states, const double* ctrls, double* out, double* jx,
                             double* ju, int n) {
  const int nx = h->nx, nu = h->nu, nv = nx + nu;
  HIP_OK(h->s_states.reserve((size_t)n * nx * sizeof(T)));
  HIP_OK(h->s_ctrls.reserve((size_t)n * nu * sizeof(T)));
  HIP_OK(h->s_out.reserve((size_t)n * nx * sizeof(T)));
  HIP_OK(h->s_jx.reserve((size_t)n * nx * nx * sizeof(T)));
  HIP_OK(h->s_ju.reserve((size_t)n * nx * nu * sizeof(T)));
  HIP_OK(upload_converted<T>(h->s_states.p, states, (size_t)n * nx, h->stream));
  HIP_OK(upload_converted<T>(h->s_ctrls.p, ctrls, (size_t)n * nu, h->stream));
  const size_t lb = (size_t)h->j_nslots * kProgLanes * sizeof(T);          // at most 256 * 64 * 8 = 128 KB
  const long long lanes = (long long)n * nv;
  HIP_OK(allow_lds(program_jacobian_kernel<T>, lb));
  hipLaunchKernelGGL(program_jacobian_kernel<T>, dim3((unsigned)((lanes + kProgLanes - 1) / kProgLanes)), dim3(kProgLanes),
                     lb, h->stream, jvp_of<T>(h), (const T*)h->s_states.p, (const T*)h->s_ctrls.p, (T*)h->s_out.p,
                     (T*)h->s_jx.p, (T*)h->s_ju.p, n, nx, nu);
  HIP_OK(hipGetLastError());
  HIP_OK(download_converted<T>(out, h->s_out.p, (size_t)n * nx, h->stream));
  HIP_OK(download_converted<T>(jx, h->s_jx.p, (size_t)n * nx * nx, h->stream));
  HIP_OK(download_converted<T>(ju, h->s_ju.p, (size_t)n * nx * nu, h->stream));
  return 0;
}

extern "C" int ampc_program_pred_diff_batch(ampc_handle* h, const double* states, const double* ctrls, double* out,
                                            double* jx, double* ju, int n) {
  REQUIRE(h && states && ctrls && out && jx && ju, "ampc_program_pred_diff_batch: NULL argument");
  REQUIRE(h->has_prog, "ampc_program_pred_diff_batch: the handle holds no program (ampc_set_program)");
  REQUIRE(h->has_jvp, kProgNoJacobian);
  if (n <= 0) return 0;
  REQUIRE((double)n * h->nx * (h->nx + h->nu) < 2147483647.0,
          "ampc_program_pred_diff_batch: n * nx * (nx + nu) must stay below 2^31; split the batch");
  HIP_OK(hipSetDevice(h->device));
  return h->precision == AMPC_F64 ? program_diff_impl<double>(h, states, ctrls, out, jx, ju, n)
                                  : program_diff_impl<float>(h, states, ctrls, out, jx, ju, n);
}

template <typename T>
static int program_rollout_impl(ampc_handle* h, int n, int n_steps, const double* x0, const double* ctrls,
                                double* obs_out) {
  const int nx = h->nx, nu = h->nu;
  const size_t n_obs = (size_t)n * (n_steps + 1) * nx, n_ctl = (size_t)n * n_steps * nu;
  HIP_OK(h->s_states.reserve((size_t)n * nx * sizeof(T)));
  HIP_OK(h->s_ctrls.reserve((n_ctl ? n_ctl : 1) * sizeof(T)));
  HIP_OK(h->s_out.reserve(n_obs * sizeof(T)));
  HIP_OK(upload_converted<T>(h->s_states.p, x0, (size_t)n * nx, h->stream));
  if (n_ctl) HIP_OK(upload_converted<T>(h->s_ctrls.p, ctrls, n_ctl, h->stream));
  const size_t lb = (size_t)(h->p_nslots + nx) * kProgLanes * sizeof(T);   // slots + the outputs' hand-over area
  HIP_OK(allow_lds(program_rollout_kernel<T>, lb));
  hipLaunchKernelGGL(program_rollout_kernel<T>, dim3((n + kProgLanes - 1) / kProgLanes), dim3(kProgLanes), lb, h->stream,
                     prog_of<T>(h), (const T*)h->s_states.p, (const T*)h->s_ctrls.p, (T*)h->s_out.p, n, n_steps);
  HIP_OK(hipGetLastError());
  HIP_OK(download_converted<T>(obs_out, h->s_out.p, n_obs, h->stream));
  return 0;
}

extern "C" int ampc_program_rollout(ampc_handle* h, int n, int n_steps, const double* x0, const double* ctrls,
                                    double* obs_out) {
  REQUIRE(h && x0 && obs_out && (ctrls || n_steps == 0), "ampc_program_rollout: NULL argument");
  REQUIRE(h->has_prog, "ampc_program_rollout: the handle holds no program (ampc_set_program)");
  REQUIRE(n_steps >= 0, "ampc_program_rollout: n_steps < 0");
  if (n <= 0) return 0;
  REQUIRE((double)n * (n_steps + 1) * (h->nx > h->nu ? h->nx : h->nu) < 2147483647.0,
          "ampc_program_rollout: n * (n_steps + 1) * max(nx, nu) must stay below 2^31; split the batch");
  HIP_OK(hipSetDevice(h->device));
  return h->precision == AMPC_F64 ? program_rollout_impl<double>(h, n, n_steps, x0, ctrls, obs_out)
                                  : program_rollout_impl<float>(h, n, n_steps, x0, ctrls, obs_out);
}
