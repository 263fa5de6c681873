/*
 * autompc_hip.h -- C ABI of libautompc_hip.so, the MI355X (gfx950) MPC inner-solve library.
 *
 * The reference (williamedwards/autompc) is pure Python and has no FFI; its hot path is reached
 * through two Python ABCs.  Each entry point below states which reference function(s) it
 * replaces (file:line relative to the reference tree).  The Python classes in autompc_amd/
 * bind these with ctypes and reproduce the reference's Controller / Model plugin surface.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error; ampc_last_error() returns the message
 *     of the calling thread's last failure.  Nothing throws across this boundary.
 *   - all host arrays are caller-owned, contiguous, row-major, IEEE float64 ("double").  The
 *     library converts to its compute precision (AMPC_F64 or AMPC_F32) on the device.
 *   - a handle is bound to one HIP device and one stream; calls on one handle must be
 *     serialised by the caller (the reference is single-threaded).  Different handles may be
 *     used from different threads / processes (one per GPU).
 *   - "_dev" variants take DEVICE pointers (in the handle's compute precision) and only enqueue
 *     work on the handle's stream: no host synchronisation, no PCIe traffic.
 */
#ifndef AUTOMPC_HIP_H
#define AUTOMPC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ampc_handle ampc_handle;
typedef struct ampc_mppi_plan ampc_mppi_plan;
typedef struct ampc_ilqr_plan ampc_ilqr_plan;
typedef struct ampc_lqr_plan ampc_lqr_plan;
typedef struct ampc_mlpfit_plan ampc_mlpfit_plan;

enum { AMPC_F64 = 0, AMPC_F32 = 1 };
enum { AMPC_ACT_RELU = 0, AMPC_ACT_TANH = 1, AMPC_ACT_SIGMOID = 2, AMPC_ACT_SELU = 3 };
/* MPPI terminal-cost mode: 0 = the reference's behaviour (terminal cost of the LAST particle
 * added to every particle, mppi.py:79-82,146-148); 1 = per-particle terminal cost. */
enum { AMPC_TERM_REFERENCE = 0, AMPC_TERM_PER_PARTICLE = 1 };

const char* ampc_last_error(void);
int ampc_version(void);   /* 100 * major + minor; 104: + ampc_mppi_run_legacy; 105: + ampc_set_affine_quad_costs;
                           * 106: + ampc_ilqr_solve_queue_var, ampc_ilqr_closed_loop_var, ampc_set_indicator_costs,
                           *      ampc_mppi_plan_set_models, ampc_ilqr_plan_set_models; 107: + ampc_set_mlp_dev, ampc_ilqr_plan_set_constants;
                           * 108: + ampc_kstep_errors; 109: + ampc_lqr_*; 110: + ampc_linfit_fit;
                           * 111: + ampc_kstep_errors_linear; 112: + ampc_kstep_errors_sindy;
                           * 113: + ampc_sindy_fit; 114: + ampc_lasso_fit; + ampc_stable_fit, + ampc_mlpfit_*, + ampc_kstep_errors_mlp,
                           *      + ampc_mppi_plan_set_model_table, + ampc_ilqr_plan_set_model_table, + ampc_mppi_plan_set_sindy_models,
                           *      + ampc_ilqr_plan_set_sindy_models, + ampc_mppi_plan_set_linear_models, + ampc_mppi_closed_loop_linear,
                           *      + ampc_ilqr_plan_set_linear_models, + ampc_ilqr_closed_loop_linear, + ampc_ilqr_linear_table_layout,
                           *      + ampc_lqr_gains_ex, + ampc_lqr_plan_set_loop_ex, + ampc_set_program, + ampc_program_rollout,
                           *      + ampc_set_program_jvp, + ampc_program_pred_diff_batch, + ampc_program_set_ilqr, + ampc_ilqr_plan_jacobians
                           *      (no bump: callers detect them by their symbols) */
int ampc_device_count(void);

/* ---- handle ------------------------------------------------------------------------------ */
/* stream: a hipStream_t to enqueue on (e.g. torch's current stream), or NULL to let the library
 * create its own. */
int ampc_create(int device, int precision, void* stream, ampc_handle** out);
int ampc_destroy(ampc_handle* h);
int ampc_synchronize(ampc_handle* h);
int ampc_precision(const ampc_handle* h);

/* ---- model: MLP surrogate dynamics --------------------------------------------------------
 * Replaces the state held by autompc.sysid.MLP (mlp.py:137-165 net, :308-321 parameters).
 * weights[l] is torch.nn.Linear layout [out_l][in_l]; l = 0..n_hidden (last = output layer).
 * nx <= 64, hidden widths 16..256 (MPPI, prediction and Jacobians: tests/test_gpu_mppi.py
 * test_mppi_wide_states_with_wide_networks_vs_oracle runs 40 / 48 / 64 states against 192..256-unit layers);
 * iLQR plans on MLP models: nx + nu <= 63, the four- / twelve-row line search for nx <= 32 (else the sixteen-row kernel).
 * x' = x + dy_mean + dy_std * net(([x,u] - xu_mean) / xu_std)          (mlp.py:219-236)
 * activation: 0 relu, 1 tanh, 2 sigmoid, 3 selu (mlp.py:44-51); 4 identity (ampc_set_linear). */
int ampc_set_mlp(ampc_handle* h, int nx, int nu, int n_hidden, const int* hidden_sizes,
                 int activation, const double* const* weights, const double* const* biases,
                 const double* xu_mean, const double* xu_std, const double* dy_mean,
                 const double* dy_std);

/* The same model from DEVICE memory: every pointer (the two pointer arrays themselves are host arrays) is a
 * float64 array in the memory of the handle's device, laid out as above -- what a PyTorch-ROCm fit of the
 * network leaves behind (mlp.py:177-217: the reference trains on its torch device and predicts there,
 * mlp.py:229-236; its weights never visit numpy).  The normalisers are folded and the MFMA fragment
 * packings written by two kernels on the handle's stream (csrc/api_model.cpp), bit for bit what
 * ampc_set_mlp produces from the same numbers; no host copy of the parameters is made.  The arrays are
 * only read and may be released when the call returns; work that produces them must be complete
 * (synchronise the producing stream) before the call. */
int ampc_set_mlp_dev(ampc_handle* h, int nx, int nu, int n_hidden, const int* hidden_sizes,
                     int activation, const double* const* weights_dev, const double* const* biases_dev,
                     const double* xu_mean_dev, const double* xu_std_dev, const double* dy_mean_dev,
                     const double* dy_std_dev);

/* ---- kernels specialised for the staged model's shape -------------------------------------------
 * The reference's MLP configuration space is 1-4 hidden layers of 16-256 units (mlp.py:113-122).
 * Kernels specialised for a model shape (all dimensions, strides and LDS offsets immediates; 1.1-1.9x
 * faster than the run-time-shape kernels) are built in for the benchmark systems' default networks
 * (csrc/shapes.hpp).  For any other MLP shape the library compiles them itself: once a handle has
 * both a model and a cost (the observation dimension is part of the shape), an out-of-process hipcc
 * build of a "shape plugin" starts in the background -- cached on disk in $AMPC_JIT_CACHE (default
 * <package>/jit_cache; ~/.cache/autompc_amd when the package directory is read-only), keyed by precision, shape and a hash of the kernel sources -- and plans
 * created after it has finished use it; until then the run-time-shape kernels run.  Results are
 * bit-identical either way.  AMPC_JIT=0 in the environment disables it.
 *   ampc_jit_status  0 nothing to do (registered shape, SINDy / wide linear model, JIT disabled), 1 building,
 *                    2 ready, -1 failed; msg (optional) receives the plugin path or the build log's path
 *   ampc_jit_wait    block until the handle's shape is ready (returns 0) or failed (< 0)            */
int ampc_jit_status(ampc_handle* h, char* msg, int msg_len);
/* build = 0: this handle never STARTS (nor waits for) a run-time build -- for models that live for one evaluation
 * (a tuner fits a model per configuration, pipeline.py:138-145: a 5 s build for 40 ms of use); a plugin that is
 * already loaded or cached is still used.  Default 1.  Call before the model is staged. */
int ampc_handle_set_jit(ampc_handle* h, int build);
int ampc_jit_wait(ampc_handle* h);
/* Which kernels a plan launches (pass one plan, NULL for the other): 0 run-time-shape, 1 a shape
 * registered at build time, 2 a shape plugin compiled at run time, 3 the run-time-shape four-row rollout kernel
 * (small MPPI problems: f64, hidden width <= 64 -- <= 128 with at most two hidden layers --, at most
 * 32 states, and so few samples that sixteen-row tiles would leave most compute units idle). */
int ampc_plan_kernel_kind(const ampc_mppi_plan* mppi, const ampc_ilqr_plan* ilqr);

/* ---- model: linear dynamics (alternative to ampc_set_mlp) ----------------------------------
 * x' = A x + B u with A [nx][nx], B [nx][nu] row-major: the prediction of autompc.sysid.ARX
 * (arx.py:151-164, state = stacked observation/control history + constant 1) and
 * autompc.sysid.Koopman (koopman.py:170-184, state = lifted observation).  The model is staged
 * as a one-hidden-layer identity-activation network (activation code 4), so the MLP entry
 * points below (ampc_mlp_pred_batch / _pred_diff_batch, whose Jacobians are then A and B) and
 * every solver serve it unchanged.  Costs see the first obs_dim state entries
 * (mppi.py:73-82, ilqr.py:124-128).
 * Up to 64 states: above 32 (long-history ARX, large Koopman lifts; e.g. ARX with history 2 on
 * HalfCheetah: 41) the MFMA tile carries three or four output column tiles; iLQR plans need
 * nx + nu <= 63 (the augmented Quu system lives in one wave).
 * 65 .. 256 states (ARX history 3..10 on HalfCheetah: 66..235, arx.py:27,37-45): a dedicated
 * K-tiled MFMA kernel family (csrc/linear_kernels.hpp) serves ampc_mlp_pred_batch /
 * _pred_diff_batch, MPPI plans and the closed loop; iLQR plans are refused there. */
int ampc_set_linear(ampc_handle* h, int nx, int nu, const double* A, const double* B);

/* Model.pred_batch (model.py:109-130, mlp.py:229-236): out[n][nx]. */
int ampc_mlp_pred_batch(ampc_handle* h, const double* states, const double* ctrls, double* out,
                        int n);
/* Model.pred_diff_batch (model.py:155-184, mlp.py:281-305): out[n][nx], jx[n][nx][nx],
 * ju[n][nx][nu].  Analytic Jacobian chain instead of the reference's autograd. */
int ampc_mlp_pred_diff_batch(ampc_handle* h, const double* states, const double* ctrls,
                             double* out, double* jx, double* ju, int n);

/* ---- model: SINDy feature-library dynamics (alternative to ampc_set_mlp) -------------------
 * Replaces the inference half of autompc.sysid.SINDy (sindy.py:173-244; the fit stays on the
 * host).  Feature k is kind[k] applied to variables v = [x, u]:
 *   0 v_a   1 sin(p v_a)   2 cos(p v_a)   3 v_a sin(p v_b)   4 v_a cos(p v_b)   5 v_a ** p
 * with a = arg0[k], b = arg1[k], p = param[k]; xi [nx][n_feat] are the coefficients.
 *   6 monomial  prod_j v_{pair_var[j]} ** pair_exp[j]  over the arg1[k] (1..10) pairs starting at
 *     pair arg0[k] of the pair list (n_pairs, pair_var, pair_exp; NULL / 0 without monomials):
 *     the polynomial cross terms of basis_funcs.py:27-93 (sindy.py:143-145), gradient :74-84.
 *   discrete:   x' = Theta(v) xi'        continuous:  x' = x + dt Theta(v) xi'        (nx <= 64)
 * strict_reference != 0 reproduces the reference Jacobian's quirks (interaction terms counted
 * twice, polynomial gradient without the exponent factor; basis_funcs.py:24-25), as pinned by
 * tests/golden/sindy_*.npz (the reference's own pred_diff_batch outputs).  MPPI plans, iLQR
 * plans and the closed loop all work on a handle holding a SINDy model. */
int ampc_set_sindy(ampc_handle* h, int nx, int nu, int n_feat, const int* kind, const int* arg0,
                   const int* arg1, const double* param, const double* xi, int continuous,
                   double dt, int strict_reference, int n_pairs, const int* pair_var,
                   const int* pair_exp);
int ampc_sindy_pred_batch(ampc_handle* h, const double* states, const double* ctrls, double* out,
                          int n);
int ampc_sindy_pred_diff_batch(ampc_handle* h, const double* states, const double* ctrls,
                               double* out, double* jx, double* ju, int n);
/* Dynamic LDS (bytes) that the prediction kernel requests for a SINDy model of these feature-program sizes
 * (n_tab == 0: direct evaluation), and whether it copies the program to LDS; no handle and no device needed.
 * Returns -1, with ampc_last_error() naming the staged program, where ampc_sindy_pred_batch refuses the model:
 * a request beyond the 160 KB a workgroup can have is refused before any launch. */
int ampc_sindy_pred_lds(int f64, int nx, int nu, int n_feat, int n_trig, int n_pow, int n_mon, int n_pool,
                        int n_tab, int* staged, int* lds_bytes);

/* ---- model: analytic dynamics as a straight-line program (a SIMULATION model) ---------------
 * The closed-form true dynamics of a benchmark (benchmarks/cartpole.py, cartpole_v2.py: a handful of + - * / sin cos
 * on the observation and the control) as a list of three-address instructions over value slots, interpreted on the
 * device one row per lane (csrc/program_kernels.hpp).  Slots 0 .. nx+nu-1 hold [x | u] on entry; instruction i is
 * code[i] = (op, dst, a, b):
 *    0 const  v[dst] = consts[a]         1 add   2 sub   3 mul   4 div   v[dst] = v[a] op v[b]
 *    5 neg    6 sin   7 cos   8 exp   9 sqrt   10 abs   11 tanh          v[dst] = f(v[a])
 *   12 powi   v[dst] = v[a] ** b, b an integer in -64..64: ((v*v)*v).., then the reciprocal for b < 0
 *   13 min   14 max  (a NaN operand gives NaN, as numpy.minimum / maximum)
 *   15 sign  v[dst] = -1, 0 or +1 (NaN stays NaN)    16 lt  v[dst] = v[a] < v[b] ? 1 : 0    (both exact)
 * and output i is v[out_slot[i]].  Every instruction rounds once in the handle's precision, in list order, with no
 * contraction: the exactly rounded operations (all but sin / cos / exp / tanh) reproduce a numpy evaluation of the
 * same list bit for bit.  Limits: nx <= 64, nu <= 16, n_slots <= 256, n_instr <= 4096 (256 slots plus the rollout's
 * 64 hand-over rows of 64 lanes of f64 are the 160 KB of LDS a workgroup can have).
 * Everything is validated on the host before anything is uploaded -- unknown opcode, dst / operand slot >= n_slots,
 * constant index >= n_const, a slot >= nx+nu read before it is written, an out_slot nothing wrote, a limit -- and a
 * malformed program is a return code with an ampc_last_error() text, never a launch.
 * A handle holding a program serves ampc_mlp_pred_batch, ampc_program_rollout and, as `surrogate`, every closed loop
 * (a model whose state starts with the observation).  It has no Jacobians (the _pred_diff_batch entries refuse it)
 * and is no controller model (MPPI / iLQR plan creation and the LQR model list refuse it) -- until
 * ampc_set_program_jvp stages the program's JVP beside it (below). */
int ampc_set_program(ampc_handle* h, int nx, int nu, int n_slots, int n_instr, const int* code, int n_const,
                     const double* consts, const int* out_slot);
/* obs_out[n][n_steps+1][nx]: row 0 is x0[n][nx], row t+1 the program applied to row t and ctrls[n][t][nu]; one
 * launch, one lane per trajectory, the state stays on chip between steps (utils/data_generation.py's loops).  Row t+1
 * equals what ampc_mlp_pred_batch returns for row t bit for bit. */
int ampc_program_rollout(ampc_handle* h, int n, int n_steps, const double* x0, const double* ctrls,
                         double* obs_out);
/* The JVP (Jacobian-vector product, forward-mode derivative) of the handle's program, as a program of the same format
 * and instruction set with 2 (nx + nu) inputs [x | u | dx | du] -- slots 0 .. 2(nx+nu)-1 on entry -- and 2 nx outputs
 * [f(x, u) | J(x, u) . (dx, du)] in out_slot[2 nx].  Needs a handle that holds a program (ampc_set_program first); the
 * same limits (n_slots <= 256, n_instr <= 4096) and the same host-side validation as ampc_set_program, every refusal a
 * return code with an ampc_last_error() text before anything is uploaded.  The constants are converted to the
 * handle's precision.  ampc_set_program and every other ampc_set_* model call drop a staged JVP.
 * The library CANNOT check that the JVP belongs to the program: it runs what it is given (sysid/program.py derives it).
 * A handle with a program and its JVP
 *   - has Jacobians: ampc_program_pred_diff_batch, and ampc_mlp_pred_diff_batch forwards to it;
 *   - is an MPPI controller model: ampc_mppi_plan_create accepts it (csrc/mppi_program_kernels.hpp: one sample per
 *     lane; (n_slots + nx) * 64 values and the cost block must fit the 160 KB of LDS, refused otherwise), and
 *     ampc_mppi_solve / _run / _run_legacy / _closed_loop[_scored] work as for any plan, the program's state being the
 *     observation.  ampc_mppi_plan_set_models, the three model tables, ampc_mppi_plan_set_state_lift and
 *     ampc_lqr_plan_set_models refuse a program with or without a JVP; ampc_ilqr_plan_create refuses it until
 *     ampc_program_set_ilqr (below) has been called on the handle. */
int ampc_set_program_jvp(ampc_handle* h, int n_slots, int n_instr, const int* code, int n_const, const double* consts,
                         const int* out_slot);
/* out[n][nx], jx[n][nx][nx], ju[n][nx][nu] of n rows from the staged JVP: one lane per (row, input direction), the
 * value recomputed per direction by the same interpreter, so out equals ampc_mlp_pred_batch bit for bit and a JVP of
 * exactly rounded operations equals its host evaluation bit for bit.  f64 and f32 handles. */
int ampc_program_pred_diff_batch(ampc_handle* h, const double* states, const double* ctrls, double* out, double* jx,
                                 double* ju, int n);
/* The opt-in that makes a program with its JVP an iLQR controller model: the perfect-model iLQR plan.  Needs a handle
 * that holds a program AND a staged JVP (a return code and an ampc_last_error() text naming what is missing otherwise);
 * enable != 0 sets the flag, 0 clears it.  ampc_set_program, ampc_set_program_jvp and every other ampc_set_* model call
 * clear it, where they drop the JVP.  With the flag set ampc_ilqr_plan_create accepts the handle if it is f64 (an f32
 * program handle is refused), nx + nu <= 63, the cost blocks are on nx observations and have no indicator terms, and
 * the line search fits the 160 KB of LDS: [16][nx + nu + 1] rows, [16][nx] next states, the forward program's
 * [n_slots][16] value slots and the Riccati / cost workspace.  The line search (csrc/ilqr_kernels.hpp, DYN = 3) runs
 * the interpreter on one column per candidate row, the Jacobian refresh (csrc/program_kernels.hpp) the JVP on one lane
 * per (plan row, input direction); ampc_ilqr_solve, _solve_queue[_var] with per-problem horizons and
 * ampc_ilqr_closed_loop[_var] against any surrogate work as on a SINDy plan, the program's state being the observation.
 * Every launch reads the program and the JVP the handle holds THEN: a solve refuses a handle whose JVP or flag was
 * dropped, or whose program has more value slots than the plan was built for.  ampc_ilqr_plan_set_models, the three
 * model tables and model_index are refused on such a plan. */
int ampc_program_set_ilqr(ampc_handle* h, int enable);

/* ---- cost / bounds ------------------------------------------------------------------------
 * Replaces QuadCost (quad_cost.py:7-51) as read through Cost.eval_* (cost.py:66-213).
 * n_costs blocks (one per tuning candidate), each Q[no][no], R[nu][nu], F[no][no], goal[no]. */
int ampc_set_quad_costs(ampc_handle* h, int n_costs, int obs_dim, const double* Q,
                        const double* R, const double* F, const double* goal);
/* A sum of quadratic terms (SumCost._sum_results, sum_cost.py:49-54, over quad_cost.py:7-51) whose
 * goals differ -- what QuadCostFactory + GaussRegFactory produce (gauss_reg_factory.py:37-45: goal =
 * mean of the data; sum_cost_factory.py) and what the reference's MPPI / iLQR evaluate term by term
 * through Cost.eval_* (mppi.py:73-82, ilqr.py:124-129,159-174).  About the first term's goal g the
 * sum is an affine-quadratic form, per block:
 *   stage     (x-g)'Q(x-g) + lin'(x-g) + consts[0] + u'Ru          Q = sum Q_k, R = sum R_k,
 *   terminal  (x-g)'F(x-g) + lin_term'(x-g) + consts[1]            F = sum F_k,
 *   lin = sum (Q_k+Q_k')(g-g_k),  consts[0] = sum (g-g_k)'Q_k(g-g_k)   (lin_term, consts[1]: with F_k)
 * lin [n_costs][obs_dim], lin_term [n_costs][obs_dim], consts [n_costs][2]; any of the three may be
 * NULL (zeros: ampc_set_quad_costs).  iLQR's stage gradient is (Q+Q')(x-g) + lin; its terminal
 * gradient is (F+F')x as the reference computes it term by term (cost.py:195: no goal, hence no
 * lin_term), or (F+F')(x-g) + lin_term under ampc_ilqr_plan_set_terminal_goal(1). */
int ampc_set_affine_quad_costs(ampc_handle* h, int n_costs, int obs_dim, const double* Q,
                               const double* R, const double* F, const double* goal,
                               const double* lin, const double* lin_term, const double* consts);
/* Indicator terms of an MPPI controller's cost.  The reference's MPPI charges whatever Cost the task holds,
 * term by term (mppi.py:73-82 over sum_cost.py:49-54): e.g. QuadCost + ThresholdCost, or a bare
 * BoxThresholdCost -- 1 per time step whose observation violates the term, no control or terminal part
 * (thresh_cost.py:27-38, 73-83).  The n_terms (<= 8) terms are added to the stage cost x_0 .. x_{H-1} of
 * EVERY cost block of the handle; kinds / params as ampc_score_trajectories (1 threshold: goal[no]
 * obs_range_lo obs_range_hi threshold; 2 box: lower[no] upper[no]).  Call after ampc_set_quad_costs /
 * ampc_set_affine_quad_costs (the quadratic part; all zeros for a cost without one), which fix obs_dim;
 * n_terms = 0 removes the terms.  MPPI plans and the MPPI closed loop evaluate them (every model family);
 * ampc_ilqr_plan_create refuses a handle that has them (no gradient / Hessian). */
int ampc_set_indicator_costs(ampc_handle* h, int n_terms, const int* kinds, const double* params);
/* Task.get_ctrl_bounds (task.py:257-267): lo[nu], hi[nu] (MPPI requires finite bounds,
 * mppi.py:100-102; iLQR clips only if bounded, ilqr.py:62-64). */
int ampc_set_ctrl_bounds(ampc_handle* h, const double* lo, const double* hi);

/* ---- MPPI ---------------------------------------------------------------------------------
 * A plan owns device buffers for a batch of B independent MPPI problems (B = 1 for the plain
 * Controller.run() path; B = candidates-per-GPU for the tuning evaluator).
 * Problem p has num_path[p] samples, horizon[p] steps, noise variance sigma[p], temperature
 * lmda[p] and cost block cost_index[p]  (MPPI.__init__, mppi.py:87-105). */
int ampc_mppi_plan_create(ampc_handle* h, int B, const int* num_path, const int* horizon,
                          const double* sigma, const double* lmda, const int* cost_index,
                          int term_mode, ampc_mppi_plan** out);
int ampc_mppi_plan_destroy(ampc_mppi_plan* p);
/* Fix the launch geometry instead of letting the library derive it from the batch: tile_rows
 * (0 automatic, or 4 / 16 / 32 / 64 samples per rollout workgroup; a height that does not fit LDS
 * for the staged model / horizon, or 4 for a model the four-row kernel does not cover, is an error) and horizon_cap (the LDS / partial-sum layout is sized
 * for max(horizon_cap, longest horizon in the plan)).  Summation orders inside a solve depend on
 * the geometry; with both fixed, a problem's results are bit-identical whatever else shares the
 * plan -- the candidate evaluator uses this so that a candidate's surrogate score
 * (pipeline_tuner.py:213-258) is the same for any sharding of the batch.  Resets device buffers:
 * call before ampc_mppi_upload. */
int ampc_mppi_plan_set_geometry(ampc_mppi_plan* p, int tile_rows, int horizon_cap);
/* Host -> device.  Any pointer may be NULL (left unchanged on the device).
 *   x0      [B][nx]                       model state each solve starts from
 *   act_seq [sum_p H_p*nu]                warm-start sequences, problem-major, units of umax
 *   eps     [sum_p N_p*H_p*nu]            noise exactly as numpy draws it: per problem
 *                                         [N][H][nu] (mppi.py:126 before the transpose)       */
int ampc_mppi_upload(ampc_mppi_plan* p, const double* x0, const double* act_seq,
                     const double* eps);
/* Fill the plan's noise buffer on the device: eps ~ N(0, sigma_p) from Philox4x32-10 keyed by
 * (seed, stream, noise id of the problem, element).  `stream` (< 2^56) is the caller's step
 * counter.  Statistically equivalent to, not bit-identical with, numpy's draw (mppi.py:21-24).
 * Callers that draw stream, stream + 1, ... with one seed get the next draw formed by the previous solve's
 * update launch (the same values; this call then only swaps two buffers) -- AMPC_NOISE_AHEAD=0 disables. */
int ampc_mppi_generate_eps(ampc_mppi_plan* p, uint64_t seed, uint64_t stream);
/* The reference's noise draw itself, on the device: fills the plan's noise buffer with what
 *   np.random.normal(scale=sqrt(sigma_p), size=(N_p, H_p, nu))          (mppi.py:16-24, :126)
 * returns for every problem in turn when numpy's global LEGACY generator (MT19937 + polar method
 * with its cached second value) is in the state (key[624], pos, has_gauss, cached) -- the tuple
 * np.random.get_state() returns -- and hands back the state the generator is left in, to be
 * installed with np.random.set_state().  The raw MT19937 stream, the uniform doubles and every
 * accept / reject decision are bit-identical to numpy's; so are the normals when
 * ampc_legacy_log_mode() != 0 (see below).  Synchronises. */
/* Whether ampc_mppi_legacy_normal's normals are numpy's bit for bit.  numpy's legacy_gauss calls
 * the C library's log(); at first use the library locates glibc's log tables in the loaded libm
 * and checks its operation-by-operation restatement of glibc's algorithm (glibc >= 2.28,
 * sysdeps/ieee754/dbl-64/e_log.c) against log() itself:
 *   1  log() is glibc's FMA build and is reproduced exactly      } normals bit-identical
 *   2  log() is glibc's non-FMA build and is reproduced exactly  } to numpy's
 *   0  another log(): the device uses its own (normals within 3 ulp of numpy's; generator state,
 *      uniforms and accept / reject decisions still exact). */
int ampc_legacy_log_mode(void);
/* key_out may be key itself (the generator's own memory: the state is updated in place). */
int ampc_mppi_legacy_normal(ampc_mppi_plan* p, const uint32_t* key, int pos, int has_gauss,
                            double cached, uint32_t* key_out, int* pos_out, int* has_gauss_out,
                            double* cached_out);
/* How many draws of this plan were repeated because a wait inside the draw kernel expired (its workgroups look
 * back at their predecessors' pair counts with a bounded wait; under heavy contention from other streams or
 * processes a wait can run out).  A repeated draw starts from the same generator state and gives the same values;
 * the count is diagnostic.  AMPC_POLAR_SPIN_LIMIT in the environment shortens the first attempt's bound (tests). */
int ampc_mppi_plan_legacy_redraws(const ampc_mppi_plan* p, long long* count);
/* Jump polynomials of MT19937 (autompc_amd/data/mt19937_jump.npz, computed by tools/mt_jump.py):
 * polys[n_polys][624] = bits of t^(s * jump_blocks * 624) mod phi for s = 1 .. n_polys.  With a
 * table installed (process-wide) ampc_mppi_legacy_normal generates the raw stream block-parallel
 * (one workgroup per jump_blocks blocks) instead of sequentially; results are identical.  Up to 4
 * tables with different jump_blocks may be installed side by side: a stream is generated with the
 * shortest segments whose table covers it. */
int ampc_set_mt_jump_table(const uint32_t* polys, int n_polys, int jump_blocks);
/* ids[B]: the noise id of every problem (default: its index in the plan).  The candidate
 * evaluator passes each candidate's GLOBAL index, so that the noise -- and therefore the
 * surrogate score pipeline_tuner.py:213-258 returns for it -- does not depend on how a batch of
 * candidates is sharded over GPUs or on the candidate's position in its shard.
 * Noise already drawn with ampc_mppi_generate_eps is drawn again with the new ids (same seed and stream);
 * ampc_mppi_plan_set_geometry likewise re-draws it for the rebuilt plan. */
int ampc_mppi_plan_set_noise_ids(ampc_mppi_plan* p, const uint32_t* ids);
/* One MPPI solve per problem, enqueued on the handle's stream (MPPI.do_rollouts + update,
 * mppi.py:110-152): shift warm start, rollout all samples, softmin weights, update act_seq. */
int ampc_mppi_solve(ampc_mppi_plan* p);
/* Device -> host (synchronises).  Any pointer may be NULL.
 *   act_seq [sum_p H_p*nu]   updated sequences;  u [B][nu] = act_seq[p][0] * umax
 *   costs   [sum_p N_p]      per-sample costs (mppi.py:150-152)
 *   eps_out [sum_p H_p*N_p*nu] post-clip noise, per problem [H][N][nu] (as do_rollouts returns) */
int ampc_mppi_download(ampc_mppi_plan* p, double* act_seq, double* u, double* costs,
                       double* eps_out);
/* MPPI.run (mppi.py:154-168) for the plan's B controllers in ONE call with one host synchronisation:
 *   x0 [B][nx] in;  act_seq (optional, NULL = keep the device's warm start) in;
 *   noise: 0 = the plan's noise buffer as it is (ampc_mppi_upload / ampc_mppi_legacy_normal),
 *          1 = fresh Philox noise keyed by (seed, stream), as ampc_mppi_generate_eps;
 *   solve;  u [B][nu] = act_seq[p][0] * umax out.
 * Equivalent to ampc_mppi_upload + ampc_mppi_generate_eps + ampc_mppi_solve + ampc_mppi_download(u),
 * without their intermediate synchronisations (the drop-in classes' hot call). */
int ampc_mppi_run(ampc_mppi_plan* p, const double* x0, const double* act_seq, int noise, uint64_t seed,
                  uint64_t stream, double* u);
/* ampc_mppi_run with the reference's own noise: ampc_mppi_legacy_normal (numpy's legacy draw from
 * the generator state key / pos / has_gauss / cached, mppi.py:16-24, :126) + ampc_mppi_run(noise 0) in
 * one call with ONE synchronisation; the state after the draw comes back as from
 * ampc_mppi_legacy_normal (key_out may be key).  The default mode of the drop-in MPPI.run(). */
int ampc_mppi_run_legacy(ampc_mppi_plan* p, const double* x0, const double* act_seq, const uint32_t* key,
                         int pos, int has_gauss, double cached, uint32_t* key_out, int* pos_out,
                         int* has_gauss_out, double* cached_out, double* u);
/* Overwrite x0 of every problem from a device buffer [B][nx] in compute precision (closed-loop
 * evaluator: no host round trip). */
int ampc_mppi_set_x0_dev(ampc_mppi_plan* p, const void* x0_dev);
/* Kernel-level introspection for bench.py: grid size (workgroups) and samples per workgroup of
 * the rollout launch, algorithmic FLOPs and bytes of one solve. */
int ampc_mppi_plan_info(const ampc_mppi_plan* p, int* n_workgroups, int* samples_per_wg,
                        double* flops, double* bytes);
/* Which rollout kernel ampc_mppi_solve launches for a plan whose handle holds a SINDy model (read-only; the
 * launcher takes the same decision from the same function, with AMPC_SINDY_FP / AMPC_SINDY_G as they stand):
 * spread 1 = features spread over `lanes` (16 / 32 / 64) lanes per sample, 0 = one thread per sample (lanes 1);
 * staged = the kernel copies the feature program to LDS; lds_bytes = dynamic LDS of the launch, the staged program
 * included.  A one-thread launch whose columns fit the 160 KB of a workgroup only without the staged program runs
 * unstaged (staged 0).  Refused for a plan that holds a table of models. */
int ampc_mppi_plan_sindy_launch(const ampc_mppi_plan* p, int* spread, int* lanes, int* staged, int* lds_bytes);
/* The same decision from sizes alone (no handle, no device): a plan of `samples` samples (every problem's count
 * rounded up to 64) and horizon cap max_h on a model of these feature-program sizes; fp_allowed / g_forced stand
 * for AMPC_SINDY_FP / AMPC_SINDY_G.  Returns -1 where ampc_mppi_plan_create would refuse the plan. */
int ampc_mppi_sindy_launch_choice(int f64, int nx, int nu, int n_feat, int n_trig, int n_pow, int n_mon, int n_pool,
                                  int n_tab, int cost_stride, int max_h, long long samples, int fp_allowed,
                                  int g_forced, int* spread, int* lanes, int* staged, int* lds_bytes);

/* keep_eps_out = 0: do not materialise the clipped noise in HBM (it is only needed by
 * ampc_mppi_download(eps_out); the solve itself keeps it in LDS).  Default 1. */
int ampc_mppi_plan_set_outputs(ampc_mppi_plan* p, int keep_eps_out);

/* Per-kernel timing for the roofline report: when enabled, every ampc_mppi_solve brackets the
 * rollout and update launches with HIP events on the handle's stream.  ampc_mppi_plan_timing
 * synchronises, returns the AVERAGE duration (ms) of each kernel over the solves since the last
 * call, and resets the counters.  enable = n > 1: only every n-th solve is bracketed (the three event records
 * of a solve cost about 11 us on the stream: 3.7 % of a config-3 solve). */
int ampc_mppi_plan_set_timing(ampc_mppi_plan* p, int enable);
int ampc_mppi_plan_timing(ampc_mppi_plan* p, double* rollout_ms, double* update_ms, int* count);

/* ---- closed loop on the surrogate (device resident) ---------------------------------------
 * simulate() (utils/simulation.py:11-64) for the B controllers of a plan, as the tuner's
 * eval_cfg drives it (pipeline_tuner.py:222-231): n_steps x { MPPI solve from the current
 * observation; obs <- surrogate.pred(obs, u) } with no host round trip per step.
 * surrogate: handle holding the simulation model (NULL = the plan's own model); it shares the
 * plan's device, precision and dimensions; its work is enqueued on the plan's stream.
 * eps_all: NULL -> device Philox noise keyed by (seed, step, noise id); else host noise for every step,
 *          [n_steps][sum_p N_p*H_p*nu], each step laid out as ampc_mppi_upload expects.
 * traj_obs [B][n_steps+1][nx], traj_ctrls [B][n_steps+1][nu] (last control row zero, as
 * simulate() returns them).  Scoring (Cost.__call__, cost.py:27-41) is left to the caller. */
int ampc_mppi_closed_loop(ampc_mppi_plan* p, ampc_handle* surrogate, const double* init_obs,
                          int n_steps, uint64_t seed, const double* eps_all, double* traj_obs,
                          double* traj_ctrls);
/* Index of the first control step of the plan's NEXT closed loop (default 0): step s of that loop
 * draws its device noise from the Philox stream (seed, first_step + s, noise id).  An episode that
 * is run in several segments -- simulate() with a user termination condition
 * (utils/simulation.py:62-63, tasks/task.py:92-101) evaluated on the host between segments, each
 * segment starting from the state the previous one ended in -- thereby consumes exactly the noise
 * the unsegmented episode would.  One-shot: the closed loop that consumes the offset resets it to 0. */
int ampc_mppi_plan_set_step_offset(ampc_mppi_plan* p, uint64_t first_step);
/* Controller models whose state is REBUILT from every observation -- autompc.sysid.Koopman:
 * update_state(state, ctrl, obs) = lift(obs) (koopman.py:166-168), state = the basis functions applied
 * to the observation, basis-major [f_0(o_0..o_{no-1}), f_1(..), ...] (koopman.py:105-122) -- in the
 * device closed loop.  simulate() (utils/simulation.py:44-58) advances the SIMULATION model's state
 * with its own prediction and hands the controller only the observation (the first obs_dim entries);
 * with a lift set, ampc_mppi_closed_loop[_scored] does the same: init_obs is then the simulation
 * model's initial state [B][surrogate nx], every solve starts from x0 = lift(observation), and the
 * recorded rows traj_obs are [B][n_steps+1][surrogate nx].  The surrogate only has to share the
 * controls and start its state with the observation.
 *   kinds[k]: 0 identity, 1 o ** params[k] (integer power), 2 sin(params[k] o), 3 cos(params[k] o);
 *   n_basis * obs_dim must equal the controller model's state dimension;  n_basis = 0 removes the lift. */
int ampc_mppi_plan_set_state_lift(ampc_mppi_plan* p, int n_basis, const int* kinds, const double* params);

/* ---- trajectory scoring --------------------------------------------------------------------
 * Cost.__call__ (costs/cost.py:27-41) for n_traj finished trajectories of n_rows rows each:
 *   score = sum_t [eval_obs_cost(obs_t) + eval_ctrl_cost(ctrl_t)] + eval_term_obs_cost(obs_last)
 * with the task cost given as a sum of n_terms terms (SumCost._sum_results, sum_cost.py:49-54);
 * kinds[k] selects the term, its parameters are concatenated in `params` in term order:
 *   0 quadratic  (quad_cost.py:7-51)        Q[no*no] R[nu*nu] F[no*no] goal[no]
 *   1 threshold  (thresh_cost.py:8-38)      goal[no] obs_range_lo obs_range_hi threshold
 *                1 per row where max_{lo<=i<hi} |obs_i - goal_i| > threshold
 *   2 box        (thresh_cost.py:40-83)     lower[no] upper[no]  (+-inf allowed)
 *                1 per row where any obs_i < lower_i or obs_i > upper_i
 * obs [n_traj][n_rows][state_dim] (the observation is the first obs_dim entries of a row),
 * ctrls [n_traj][n_rows][ctrl_dim], scores [n_traj].  The handle only provides the device,
 * stream and precision; no model needs to be set. */
int ampc_score_trajectories(ampc_handle* h, int n_traj, int n_rows, int state_dim, int obs_dim,
                            int ctrl_dim, const double* obs, const double* ctrls, int n_terms,
                            const int* kinds, const double* params, double* scores);

/* ampc_mppi_closed_loop followed by ampc_score_trajectories on the device-resident trajectories:
 * the whole of eval_cfg's simulate + cost(traj) (pipeline_tuner.py:222-233) with only the B
 * scores coming back.  obs_dim is the one given to ampc_set_quad_costs.  traj_obs / traj_ctrls
 * may be NULL. */
int ampc_mppi_closed_loop_scored(ampc_mppi_plan* p, ampc_handle* surrogate, const double* init_obs,
                                 int n_steps, uint64_t seed, const double* eps_all, int n_terms,
                                 const int* kinds, const double* params, double* scores,
                                 double* traj_obs, double* traj_ctrls);

/* ---- iLQR ---------------------------------------------------------------------------------
 * B independent problems of horizon H (IterativeLQR.compute_ilqr_default, ilqr.py:100-265, with
 * its constants u_threshold 1e-3, ls_max_iter 10, ls_discount 0.2, ls_cost_threshold 0.3).
 * clip_to_bounds != 0 clips controls to the handle's bounds in the forward pass (ilqr.py:62-64,
 * 203-204).  Per problem:  x0 [B][nx], uguess [B][H][nu] in;  states [B][H+1][nx],
 * ctrls [B][H][nu], Ks [B][H][nu][nx], ks [B][H][nu], converged/iters/status [B], objective [B]
 * out (any output pointer may be NULL).
 * status: 0 ok; 1 singular Quu (the reference raises numpy.linalg.LinAlgError, ilqr.py:179);
 *         2 line search produced no candidate. */
int ampc_ilqr_plan_create(ampc_handle* h, int B, int horizon, double dt, const int* cost_index,
                          int clip_to_bounds, ampc_ilqr_plan** out);
int ampc_ilqr_plan_destroy(ampc_ilqr_plan* p);
/* Per-kernel timing for the roofline report: when enabled, every iteration of ampc_ilqr_solve
 * brackets its four launches with HIP events on the handle's stream.  ampc_ilqr_plan_timing
 * synchronises and returns the AVERAGE duration (ms) per iteration of
 *   kernel_ms[0] backward sweep   [1] line search + acceptance   [2] forward pass (activation
 *   derivatives of the accepted trajectory)   [3] Jacobian chain
 * over the iterations since the last call, and their number; then resets the counters.
 * enable = n > 1: a queue (ampc_ilqr_solve_queue) brackets only every n-th iteration. */
int ampc_ilqr_plan_set_timing(ampc_ilqr_plan* p, int enable);
int ampc_ilqr_plan_timing(ampc_ilqr_plan* p, double* kernel_ms, int* iterations);
/* Work of the last ampc_ilqr_solve: iterations performed (the largest per-problem count; the
 * polled loop may have queued a few no-op launches beyond it, which the timing averages skip), and
 * candidate rows the line searches rolled out, summed over the plan's problems.  The reference rolls out all ls_max_iter = 10 step
 * sizes in every iteration (ilqr.py:196-205) and then accepts the first that passes its test; the
 * f64 MLP path rolls them out four at a time and stops at the first accepted one (same decisions,
 * same results: a multiple of 4 rows per iteration) or -- many problems per launch, once some search
 * needs a third four-row pass -- all of them in one pass of a twelve-row tile (ls_max_iter rows per
 * iteration; same results again, csrc/ilqr_lsw.hpp).  Either pointer may be NULL. */
int ampc_ilqr_plan_stats(ampc_ilqr_plan* p, long long* iterations, long long* candidate_rows);
/* The plan's per-row Jacobians of its handle's model, as the last refresh left them: jx[B * horizon][nx][nx],
 * ju[B * horizon][nx][nu], row b * horizon + t for step t of slot b.  write == 0 copies them out, write != 0 copies
 * the caller's arrays in (a test's way to see which rows a refresh leaves alone).  Synchronises the plan's stream.
 * Refused on plans that keep no such rows: wide linear models and plans with a model table. */
int ampc_ilqr_plan_jacobians(ampc_ilqr_plan* p, double* jx, double* ju, int write);
/* use_goal = 0 (default): the backward sweep is seeded with the terminal gradient exactly as the
 * reference computes it, (F + F') x_N -- Cost.eval_term_obs_cost_diff ignores the goal
 * (cost.py:195, 208-211).  use_goal != 0: (F + F') (x_N - goal), the derivative of the terminal
 * cost actually charged; what QuadCost(strict_reference=False) asks for. */
int ampc_ilqr_plan_set_terminal_goal(ampc_ilqr_plan* p, int use_goal);
/* The constants compute_ilqr_default takes as arguments (ilqr.py:100-101; defaults u_threshold 1e-3,
 * ls_max_iter 10, ls_discount 0.2, ls_cost_threshold 0.3 -- what a new plan holds): convergence / early-exit
 * norm, number of step sizes alpha_j = ls_discount^j (1..16: they are the rows of one MFMA tile), and the
 * acceptance ratio.  max_iter is an argument of every solve.  Applies to the solves that follow. */
int ampc_ilqr_plan_set_constants(ampc_ilqr_plan* p, double u_threshold, int ls_max_iter, double ls_discount,
                                 double ls_cost_threshold);
int ampc_ilqr_solve(ampc_ilqr_plan* p, const double* x0, const double* uguess, int max_iter,
                    double* states, double* ctrls, double* Ks, double* ks, int* converged,
                    int* iters, int* status, double* objective);

/* Continuous batching: n_problems independent problems streamed through the plan's B slots.
 * ampc_ilqr_solve runs a batch for as long as its slowest problem; here a slot whose problem has
 * converged, failed or used up max_iter iterations takes the next unsolved problem at the following
 * iteration boundary -- on the device, with no host round trip (the finished problem's results go to
 * its output row, the new problem's guess is rolled out by the same launch that line-searches the
 * other slots) -- so every slot stays busy until the queue is empty.  Each problem's arithmetic is
 * exactly that of a one-problem ampc_ilqr_solve (IterativeLQR.compute_ilqr_default, ilqr.py:100-265):
 * results are bit-identical to it, whatever shares the plan.  What the tuner's candidate evaluator
 * feeds (one problem per candidate and control step, ilqr.py:267-295) and what bench.py's c4 times.
 *   x0 [n][nx];  uguess [n][H][nu] or NULL (zeros: IterativeLQR.run's guess, ilqr.py:280-281);
 *   cost_index [n] or NULL (block 0);  outputs as ampc_ilqr_solve, [n] rows, any may be NULL.
 * The plan's horizon, dt, bounds mode and terminal-gradient mode apply to every problem. */
int ampc_ilqr_solve_queue(ampc_ilqr_plan* p, int n_problems, const double* x0, const double* uguess,
                          const int* cost_index, int max_iter, double* states, double* ctrls,
                          double* Ks, double* ks, int* converged, int* iters, int* status,
                          double* objective);

/* ampc_ilqr_solve_queue with a horizon per problem: horizon[n], each in [1, the plan's horizon H] (NULL: H for
 * every problem = ampc_ilqr_solve_queue).  The tuner's iLQR candidates differ in their horizon
 * (IterativeLQRFactory: 5..25, control/ilqr.py:31-41); with this they share ONE plan of H = the longest -- a
 * slot's sweep, line search and Jacobian refresh run over its own problem's horizon, the launches are shared.
 * All arrays keep H as their stride: uguess [n][H][nu] (rows past a problem's horizon are ignored), outputs
 * states [n][H+1][nx], ctrls [n][H][nu], Ks [n][H][nu][nx], ks [n][H][nu] (rows past it are zero).  A
 * problem's results are bit-identical to ampc_ilqr_solve on a one-problem plan of its own horizon.
 * model_index[n] (NULL: the plan's own model for every problem): the problem's controller model, an entry of
 * the table installed with ampc_ilqr_plan_set_models -- results are those of a plan built on that model. */
int ampc_ilqr_solve_queue_var(ampc_ilqr_plan* p, int n_problems, const double* x0, const double* uguess,
                              const int* cost_index, const int* horizon, const int* model_index, int max_iter,
                              double* states, double* ctrls, double* Ks, double* ks, int* converged, int* iters,
                              int* status, double* objective);
/* Controller models per problem.  The tuner's eval_cfg builds the controller with pipeline(cfg, task, trajs),
 * which instantiates and trains a model PER CONFIGURATION when the pipeline has a model factory
 * (pipeline.py:138-145; tuning/pipeline_tuner.py:213-215): candidates of one batch may carry different models.
 * models[n_models]: handles holding MLPs of the plan's shape (same dimensions, hidden layers, activation,
 * precision, device) with their own weights and normalisers; the plan keeps a device table of their
 * descriptors (and the handles alive).  Staging new weights into one of them afterwards needs another call.
 * n_models = 0 removes the table.  Cost blocks, bounds and the surrogate remain the plan handle's. */
int ampc_ilqr_plan_set_models(ampc_ilqr_plan* p, int n_models, ampc_handle* const* models);
/* ... for an MPPI plan: model_index[B] names the table entry of each of the plan's problems; every rollout of
 * problem b then runs on models[model_index[b]] (MLP plans: the sixteen-row and the four-row rollout). */
int ampc_mppi_plan_set_models(ampc_mppi_plan* p, int n_models, ampc_handle* const* models,
                              const int* model_index);
/* MLP models of ANY mix of depth, widths and activation in one f64 MPPI plan: the rollout of every problem b runs on
 * entry model_index[b] of a device table, in 16-row tiles of one kernel for the whole plan (csrc/mppi_table_kernels.hpp).
 * The model arguments are those of ampc_kstep_errors_mlp (below): host-resident parameters are packed and uploaded
 * once by this call, on_device parameters are read in place (memory of the plan's device; the caller keeps it alive
 * and orders its own writes before the call).  The plan keeps the table until it is destroyed or n_models = 0 removes
 * it.  The call rebuilds the plan's geometry (as ampc_mppi_plan_set_geometry(p, 16, horizon cap) does: call it before
 * uploads); ampc_mppi_plan_set_geometry afterwards keeps the table and takes tile_rows 0 or 16 only.
 * Refused with a message: an f32 plan; a handle whose model is not an MLP, that has indicator cost terms (again at
 * solve time if they are set later), a state lift, per-problem models of one shape (ampc_mppi_plan_set_models);
 * models whose nx / nu are not the handle's, obs_dim != nx, anything over ampc_kstep_errors_mlp's limits; a
 * model_index out of range; and -- return code -3 instead of -1 -- an LDS map of more than 160 KB for the plan's
 * states, controls, horizon cap and cost block.
 * Deterministic: a problem's controls are the same bits alone, in any plan, at any position of it.  (Added without a
 * version bump: callers detect it by its symbol.) */
int ampc_mppi_plan_set_model_table(ampc_mppi_plan* p, int n_models, const int* n_hidden, const int* dims,
                                   const int* activations, const double* const* weights,
                                   const double* const* biases, const double* const* norms, const int* on_device,
                                   const int* model_index);
/* SINDy models of ANY mix of feature libraries (trig basis and frequency, interaction terms, polynomial degree, cross
 * terms), coefficients and time modes in one MPPI plan, f64 or f32: the rollout of every problem b runs on
 * models[model_index[b]], one launch per solve for the whole plan (csrc/mppi_sindy_table_kernels.hpp).  models[n_models]:
 * handles staged with ampc_set_sindy; the plan keeps a device table of their descriptors (and the handles alive) and
 * waits for their streams.  Staging a new library or new coefficients into one of them afterwards needs another call.
 * n_models = 0 removes the table: the plan runs on its handle's own model again.  Cost blocks (indicator terms
 * included), bounds and the surrogate remain the plan handle's; ampc_mppi_solve, ampc_mppi_closed_loop and
 * ampc_mppi_closed_loop_scored work on such a plan unchanged.  Per entry the kernel spreads the features over sixteen
 * lanes per sample (entries staged in LDS with a product table and at most eight states; AMPC_SINDY_FP=0 at the time of
 * this call switches it off) or runs one thread per sample; ampc_mppi_plan_set_geometry afterwards keeps the table.
 * Refused with a message: a plan handle or a model handle without a SINDy model; models whose nx, nu, precision or device
 * are not the plan handle's; a state lift on the plan (again at solve time if it is set later); a plan that holds
 * per-problem models of one shape (ampc_mppi_plan_set_models) or a table of MLP models (ampc_mppi_plan_set_model_table)
 * -- and those two calls on a plan that holds this table; a model_index out of range; and -- return code -3 instead of
 * -1 -- an entry whose LDS need exceeds 160 KB for the plan's horizon cap and cost block.
 * Deterministic: a problem's costs, clipped noise and controls are the same bits alone, in any plan of the same
 * geometry, at any position of it -- the bits of a single-model plan on that model under AMPC_SINDY_G=16.  (Added
 * without a version bump: callers detect it by its symbol.) */
int ampc_mppi_plan_set_sindy_models(ampc_mppi_plan* p, int n_models, ampc_handle* const* models, const int* model_index);
/* Linear models x' = A x + B u of ANY mix of state dimensions (ARX histories, Koopman lifts; 1..256 states) in one MPPI
 * plan, f64 or f32: the rollout of every problem b runs on models[model_index[b]], one launch per solve for the whole
 * plan (linear_table_rollout_kernel, csrc/mppi_linear_table_kernels.hpp: 16 samples x 8 waves per workgroup, the K-tiled
 * MFMA step of the wide linear models).  models[n_models]: handles staged with ampc_set_linear, in either staging form;
 * the call packs every entry's fragment-order [A | B] and a plain copy in the plan's precision from the handle's exact f64
 * matrices, keeps them in the plan and keeps the handles alive.  Staging new matrices into one of them afterwards needs
 * another call.  rules / n_basis / lift_kinds / lift_params are PER MODEL and have the meaning of ampc_lqr_plan_set_loop:
 * rules[k] 0 the state is the observation, 1 the ARX shift (A s + B u_prev, then the observation slot overwritten), 2 a
 * lift of the observation with n_basis[k] functions, whose (kind, parameter) pairs follow each other in lift_kinds /
 * lift_params in model order (kinds as ampc_mppi_plan_set_state_lift).  n_basis and lift_* may be NULL without rule 2;
 * rules may be NULL: plain solves only, ampc_mppi_closed_loop_linear is refused.
 * The call rebuilds the plan's geometry to 16-row tiles and makes x0 RAGGED: problem b owns nx[model_index[b]] values, in
 * plan order, and ampc_mppi_upload's x0 is that concatenation.  ampc_mppi_solve and ampc_mppi_download are unchanged.
 * Cost blocks (indicator terms included) and bounds remain the plan handle's.  n_models = 0 removes the table: the plan
 * runs on its handle's own model and the automatic geometry again.  A replacing call takes the old table out first and
 * installs the new one only once it is complete.
 * Refused with a message: NULL arguments; a plan handle or a model handle without a linear model; models whose nu,
 * precision or device are not the plan handle's; an entry with nx < obs_dim; rule 0 with nx != obs_dim; rule 2 with
 * n_basis * obs_dim != nx or a bad kind or power; a plan with a state lift, per-problem models of one shape
 * (ampc_mppi_plan_set_models), a table of MLP models or a table of SINDy models -- and those calls on a plan that holds
 * this table; ampc_mppi_plan_set_geometry with tile_rows other than 0 or 16 afterwards; ampc_mppi_run, _run_legacy,
 * ampc_mppi_set_x0_dev, ampc_mppi_closed_loop and _closed_loop_scored on such a plan (they assume x0 [B][nx]); a
 * model_index out of range; and -- return code -3 instead of -1 -- a widest entry whose LDS map (2 x 16 rows of [x | u],
 * cost block, shifted sequence) exceeds 160 KB for the plan's horizon cap.
 * Deterministic: a problem's costs, clipped noise, sequence and control are the same bits alone, in any plan of the same
 * horizon cap and update mode (fused or not), at any position of it -- the bits of a single-model plan on
 * linear_rollout_kernel for that model (one staged with more than 64 states or under AMPC_LINEAR_WIDE=1).  (Added without
 * a version bump: callers detect it by its symbol.) */
int ampc_mppi_plan_set_linear_models(ampc_mppi_plan* p, int n_models, ampc_handle* const* models,
                                     const int* model_index, const int* rules, const int* n_basis,
                                     const int* lift_kinds, const double* lift_params);
/* simulate() with MPPI.run for every problem of a plan that holds a table of linear models with rules.  Per control step:
 * state_b <- rule_b(state_b, u_prev_b, sim_b[:obs_dim]) before every solve, the first included; the noise (eps_all
 * [n_steps][sum N H nu], or Philox(seed, step offset + step) when NULL; ampc_mppi_plan_set_step_offset is honoured and
 * reset); one rollout launch and the update; sim <- surrogate.pred(sim, u); the step is recorded.  init_state
 * [sum_b nx_b]: each model's state of the one-row trajectory; init_sim [B][surrogate nx]; u_prev starts at 0.
 * init_state == init_sim == NULL continues from the states, u_prev and sim the plan kept from its previous call (an
 * episode in segments).  surrogate: any model with the plan's controls, precision and device whose state starts with the
 * observation.  traj_obs [B][n_steps+1][surrogate nx] (row 0: the sim states the call starts from), traj_ctrls
 * [B][n_steps+1][nu] (last row zero) -- either may be NULL; n_terms / kinds / params / scores as
 * ampc_mppi_closed_loop_scored, n_terms = 0 or scores = NULL skips scoring.  (Added without a version bump.) */
int ampc_mppi_closed_loop_linear(ampc_mppi_plan* p, ampc_handle* surrogate, const double* init_state,
                                 const double* init_sim, int n_steps, uint64_t seed, const double* eps_all,
                                 int n_terms, const int* kinds, const double* params, double* scores,
                                 double* traj_obs, double* traj_ctrls);

/* MLP models of ANY mix of depth, widths and activation in one f64 iLQR plan: the slot of a problem / episode runs on
 * the entry of a device table that model_index[n] of ampc_ilqr_solve_queue_var / ampc_ilqr_closed_loop_var names (range-
 * checked against the table; NULL, and the entries without that argument -- ampc_ilqr_solve, _solve_queue,
 * _closed_loop -- run entry 0).  The line search, the forward pass and the Jacobian chain of an iteration are the
 * kernels of csrc/ilqr_table_kernels.hpp (16-row tiles, one kernel each for the whole plan), the sweep is the plan's
 * run-time-shape sweep; refill / compaction / chains, the surrogate step, harvest, stats, timing, set_constants and
 * set_terminal_goal are the plan's own.  The model arguments are those of ampc_kstep_errors_mlp (below): host-
 * resident parameters are packed and uploaded once by this call, on_device parameters are read in place (memory of the
 * plan's device; the caller keeps it alive and orders its own writes before the call).  The plan keeps the table until
 * it is destroyed or n_models = 0 removes it.
 * Refused with a message: a NULL plan / argument; an f32 plan; a handle whose model is not an MLP (SINDy and linear
 * models included); obs_dim != nx; models whose nx / nu are not the handle's; anything over ampc_kstep_errors_mlp's
 * limits; nx + nu > 63; a plan that holds ampc_ilqr_plan_set_models handles (and that call on a plan with a table);
 * and -- return code -3 instead of -1 -- an LDS map of more than 160 KB for the plan's states, controls and cost block.
 * Deterministic: a problem's results are the same bits alone, in any plan, in any slot, at any position of the table.
 * (Added without a version bump: callers detect it by its symbol.) */
int ampc_ilqr_plan_set_model_table(ampc_ilqr_plan* p, int n_models, const int* n_hidden, const int* dims,
                                   const int* activations, const double* const* weights,
                                   const double* const* biases, const double* const* norms, const int* on_device);

/* SINDy models of ANY mix of feature libraries, coefficients and time modes in one f64 iLQR plan: the slot of a problem /
 * episode runs on models[model_index[n]] of ampc_ilqr_solve_queue_var / ampc_ilqr_closed_loop_var (range-checked against
 * this table; NULL, and the entries without that argument, run models[0]).  models[n_models]: handles staged with
 * ampc_set_sindy; the call waits for their streams, builds a device array of their descriptors (pointers into the
 * handles' buffers) and keeps the handles alive until n_models = 0 removes the table or the plan is destroyed.  The
 * plan keeps its run-time-shape sweep; the line search and the Jacobians are csrc/ilqr_sindy_table_kernels.hpp's: per
 * entry a lane-spread body (a product table, <= 8 states, the program staged in LDS) or one thread per line-search
 * row, chosen from the entry alone.
 * Refused with a message: NULL arguments; an f32 plan; a plan handle or a model handle without a SINDy model; models
 * whose state / control dimensions, precision or device are not the plan handle's; an observation dimension other
 * than the state dimension; a plan that holds ampc_ilqr_plan_set_models handles or an MLP table (and those two calls
 * on a plan that holds this table); a model_index past the table; and -- return code -3 instead of -1 -- an entry
 * whose LDS need exceeds 160 KB.  A call that replaces a table takes the old one out first and installs the new one
 * only once it is complete.  Deterministic: a problem's results are the same bits alone, in any plan, in any slot, at
 * any position of the table.  (Added without a version bump: callers detect it by its symbol.) */
int ampc_ilqr_plan_set_sindy_models(ampc_ilqr_plan* p, int n_models, ampc_handle* const* models);

/* Linear models x' = A x + B u of MIXED state dimension (ARX histories, Koopman lifts) in one f64 iLQR plan: the slot of
 * a problem / episode runs on models[model_index[n]] of ampc_ilqr_solve_queue_var / ampc_ilqr_closed_loop_linear (range-
 * checked; NULL runs models[0]).  models[n_models]: handles staged with ampc_set_linear, either staging form; every
 * entry is packed from the handle's exact f64 [A | B].  The plan handle -- a linear model as well -- supplies nu,
 * obs_dim, the cost blocks, the bounds and the stream.  rules / n_basis / lift_kinds / lift_params: exactly
 * ampc_mppi_plan_set_linear_models' (rule 0 the observation, 1 the ARX shift, 2 a lift); rules == NULL: a table for
 * solves only, ampc_ilqr_closed_loop_linear is then refused.  n_models == 0 removes the table and restores the plan as it
 * was built.  The sweep and the line search are csrc/ilqr_linear_table_kernels.hpp's.
 * Layout with a table: every per-problem region of x0-independent outputs keeps the stride of the plan's horizon and of
 * the WIDEST entry (nxw = max nx); inside its region a problem's rows are packed at its OWN nx, the rest is zero:
 *   x0 of ampc_ilqr_solve_queue_var is ragged, problem j's own nx values, concatenated;
 *   states [P][(H+1) * nxw], Ks [P][H * nu * nxw] hold (H_j+1) x nx_j and H_j x nu x nx_j packed values each.
 * Refused with a message: NULL arguments; an f32 plan or model; a plan handle or a model handle without a linear model;
 * models of another control dimension or device; nx < obs_dim; more than 128 states; nu not one of 1, 2, 3, 4, 6, 8; a
 * plan that holds ampc_ilqr_plan_set_models handles, an MLP table or a SINDy table (and those calls on a plan that holds
 * this table); ampc_ilqr_solve and ampc_ilqr_closed_loop[_var] on a plan that holds this table; and -- return code -3
 * instead of -1 -- an LDS need above 160 KB for the widest entry.  A replacing call installs the new table only once
 * it is complete; a refused one leaves the old table working.  Deterministic: a problem's results are the same bits
 * alone, in any batch, in any slot, at any table position, and the bits of a single-model plan on the wide linear path.
 * (Added without a version bump: callers detect it by its symbol.) */
int ampc_ilqr_plan_set_linear_models(ampc_ilqr_plan* p, int n_models, ampc_handle* const* models, const int* rules,
                                     const int* n_basis, const int* lift_kinds, const double* lift_params);

/* The layout ampc_ilqr_plan_set_linear_models packs and reserves by, without a device call: for models of nx[n_models]
 * states and nu controls in a plan of B slots, horizon H and ls_n line-search step sizes,
 *   entry_off [n_models][3]: offsets (in values) of every entry's fragments, plain rows and padded Jacobian in the
 *     table buffer;
 *   strides [10]: values per slot of states, ctrls, Ks, ks, ls_states, ls_ctrls and vj -- those of the plan's horizon
 *     and of the widest entry --, the values in the table buffer, and the LDS bytes of the sweep and of the line search
 *     for the widest entry with a cost block of obs_dim observations (above 160 KB the table is refused with -3). */
int ampc_ilqr_linear_table_layout(int n_models, const int* nx, int nu, int obs_dim, int B, int H, int ls_n,
                                  long long* entry_off, long long* strides);

/* simulate() with IterativeLQR controllers on a plan that holds a table of linear models WITH rules, any surrogate,
 * device resident: as ampc_ilqr_closed_loop_var, with a slot carrying its episode's surrogate state (surrogate nx wide)
 * beside the controller state.  Per control step: solve from a zero guess, u = ubar_0, sim <- surrogate.pred(sim, u),
 * controller state <- rule(state, u, sim[:obs_dim]); the first solve of an episode runs on rule(init state, 0,
 * init_sim[:obs_dim]), as IterativeLQR.run does.  init_states: ragged, episode c's own nx values (its model's
 * traj_to_state of the one-row trajectory), concatenated; init_sim [C][surrogate nx]; surrogate: any model with the
 * plan's controls, precision and device whose state starts with the observation (NULL: the plan handle's own model).
 * traj_obs [C][n_steps+1][surrogate nx] (row 0: init_sim), traj_ctrls [C][n_steps+1][nu] (last row zero); failed,
 * steps_done, iterations as ampc_ilqr_closed_loop.  Any output may be NULL.  (Added without a version bump.) */
int ampc_ilqr_closed_loop_linear(ampc_ilqr_plan* p, ampc_handle* surrogate, int n_chains, const double* init_states,
                                 const double* init_sim, const int* cost_index, const int* horizon,
                                 const int* model_index, int n_steps, int max_iter, double* traj_obs,
                                 double* traj_ctrls, int* failed, int* steps_done, long long* iterations);

/* simulate() with IterativeLQR controllers, device resident (utils/simulation.py:44-63 as eval_cfg drives it,
 * pipeline_tuner.py:222-231; IterativeLQR.run, ilqr.py:267-295: every control step is a full solve from a zero
 * guess, u = ubar_0, then obs <- surrogate.pred(obs, u)).  n_chains episodes of n_steps control steps stream
 * through the plan's B slots: a slot keeps its episode -- solve, surrogate step, next solve, with no host round
 * trip -- until it ends, then takes the next episode; slots whose solve has converged do not wait for the
 * others (continuous batching as in ampc_ilqr_solve_queue).  The model state must be the observation.
 *   init_obs [n][nx];  cost_index [n] or NULL (block 0);  surrogate: NULL = the plan's own model;
 *   traj_obs [n][n_steps+1][nx], traj_ctrls [n][n_steps+1][nu] (last control row zero, as simulate() returns);
 *   failed [n]: 1 = a solve hit a singular Quu (the reference's LinAlgError, which eval_cfg scores inf,
 *   pipeline_tuner.py:236-239) -- the episode stops there, steps_done [n] tells after how many control steps;
 *   iterations [n]: iLQR iterations over the episode.  Any output may be NULL. */
int ampc_ilqr_closed_loop(ampc_ilqr_plan* p, ampc_handle* surrogate, int n_chains, const double* init_obs,
                          const int* cost_index, int n_steps, int max_iter, double* traj_obs,
                          double* traj_ctrls, int* failed, int* steps_done, long long* iterations);
/* ... with an iLQR horizon per episode: horizon[n] in [1, the plan's horizon] (NULL: the plan's), and a
 * controller model per episode: model_index[n] (NULL: the plan's own), as ampc_ilqr_solve_queue_var;
 * everything else as ampc_ilqr_closed_loop (the surrogate is shared). */
int ampc_ilqr_closed_loop_var(ampc_ilqr_plan* p, ampc_handle* surrogate, int n_chains, const double* init_obs,
                              const int* cost_index, const int* horizon, const int* model_index, int n_steps,
                              int max_iter, double* traj_obs, double* traj_ctrls, int* failed, int* steps_done,
                              long long* iterations);

/* ---- model accuracy ---------------------------------------------------------------------- */
/* k-step prediction error sums (evaluation/model_metrics.py:12-43 get_model_rmse, :45-111 get_model_rmsmens, for
 * every horizon 1..kmax in one pass).  models[n_models]: handles of one shape (ampc_*_plan_set_models rules; MLP
 * models and linear models of at most 64 states -- SINDy and wide linear models are refused).
 * traj_len[n_traj]; obs [sum len][obs_dim], ctrls [sum len][nu] (row-major, trajectories concatenated);
 * init_states: NULL (model state = observation) or [n_models][sum len][state_dim] (traj_to_states rows);
 * inv_std [obs_dim] (needed only for sq_delta_err); outputs sq_err / sq_delta_err [n_models][kmax]
 * = sums over counted rows and obs dims (sq_delta_err may be NULL).  A start point (trajectory i, time t) counts
 * towards horizon h when t + h <= len_i - 1.  Deterministic (fixed-order f64 sums).  Synchronises. */
int ampc_kstep_errors(ampc_handle* const* models, int n_models, int n_traj, const int* traj_len,
                      int obs_dim, const double* obs, const double* ctrls, const double* init_states,
                      int kmax, const double* inv_std, double* sq_err, double* sq_delta_err);

/* ... of WIDE linear models (handles staged with ampc_set_linear, 65..256 states, at most 16 controls), any mix of
 * state dimensions in ONE launch (csrc/kstep_linear_kernels.hpp).  The models share precision, device, ctrl_dim and
 * the data (traj_len, obs, ctrls, kmax, inv_std, outputs: as ampc_kstep_errors); obs_dim <= every state dim.
 * Initial states are formed on the device by a state rule per model, the rules of ampc_lqr_plan_set_loop:
 *   rules [n_models]: 0 = rows supplied by the caller, init_rows[i] [sum len][state_dim_i] (traj_to_states rows;
 *     init_rows or init_rows[i] may be NULL when the model state is the observation, state_dim_i == obs_dim);
 *   1 = ARX (arx.py:47-76): state [obs_t, (obs_t-1, ctrl_t-1), .., (obs_t-k+1, ctrl_t-k+1), 1] with k =
 *     arx_history[i], rows before the trajectory's first repeated as the first (a pure gather: bit-identical to
 *     ARX.traj_to_states); 1 + k (obs_dim + ctrl_dim) - ctrl_dim must equal state_dim_i;
 *   2 = Koopman lift (koopman.py:105-122) with n_basis[i] basis functions (kind, parameter) taken in order from
 *     lift_kinds / lift_params (kinds of ampc_mppi_plan_set_state_lift; rule-2 models only consume entries);
 *     n_basis[i] * obs_dim must equal state_dim_i.
 *   arx_history / n_basis [n_models] are read for their rule's models only and may be NULL without that rule.
 * Refused: MLP, SINDy and narrow linear handles, mixed precision / device / ctrl_dim, a rule whose state size is not
 * the handle's.  Deterministic: a model's sums do not depend on the other models of the call or on their order
 * (fixed 16-row tiles, fixed-order f64 sums).  Synchronises. */
int ampc_kstep_errors_linear(ampc_handle* const* models, int n_models, int n_traj, const int* traj_len,
                             int obs_dim, const double* obs, const double* ctrls, const int* rules,
                             const int* arx_history, const int* n_basis, const int* lift_kinds,
                             const double* lift_params, const double* const* init_rows, int kmax,
                             const double* inv_std, double* sq_err, double* sq_delta_err);

/* ... of SINDy models (handles staged with ampc_set_sindy), any mix of feature libraries, coefficients and time
 * modes in ONE launch (csrc/kstep_sindy_kernels.hpp): one thread per start point, 64-row tiles, grid (tiles, models).
 * The models share precision, device, state dim and ctrl_dim; the state is the observation (obs_dim == state dim, no
 * initial-state rows); data and outputs as ampc_kstep_errors.  Refused: handles without a SINDy model, mixed
 * precision / device / state dim / ctrl_dim, obs_dim != state dim, and a model whose per-thread LDS columns
 * ((2 nx + nu + table entries) x 64 rows) do not fit LDS with the error block.  A diverging model yields non-finite
 * sums for itself only.  Deterministic: a model's sums do not depend on the other models of the call or on their
 * order (fixed 64-row tiles, fixed-order f64 sums).  Synchronises. */
int ampc_kstep_errors_sindy(ampc_handle* const* models, int n_models, int n_traj, const int* traj_len, int obs_dim,
                            const double* obs, const double* ctrls, int kmax, const double* inv_std, double* sq_err,
                            double* sq_delta_err);

/* ... of MLP models of ANY mix of depth, widths and activation in ONE launch (csrc/kstep_mlp_kernels.hpp; f64 only).  No
 * handle is involved and nothing is packed per shape: a model is its plain parameters, read through a device table.
 *   device: the GPU everything runs on;
 *   n_hidden [n_models] in 1..4; dims [n_models][6]: nx + nu, the hidden widths (1..256), nx, the rest ignored;
 *   activations [n_models] as ampc_set_mlp;
 *   weights / biases [n_models][5]: per linear layer (hidden layers, then the output layer; entries past a model's
 *   layers are ignored) the address of the weight [out][in], row-major as torch.nn.Linear keeps it, and of the bias
 *   [out]; norms [n_models][4]: xu_means [nx + nu], xu_std [nx + nu], dy_means [nx], dy_std [nx] (float64);
 *   on_device [n_models]: nonzero -- ALL of that model's addresses are memory of `device` (e.g. views of the flat buffer
 *   ampc_mlpfit_* trained, or separate torch tensors); they are read in place, complete when this is called, with no
 *   copy and no packing kernel (each address is checked to be memory of `device`; the extents are the caller's).
 *   Zero -- host memory: packed and uploaded once by the call.
 *   nx (1..64), nu (1..16), nx + nu <= 80: every model of a call takes nx + nu inputs and gives nx outputs.
 * The step is MLP.pred_batch's (autompc/sysid/mlp.py:229-236): x' = x + (net(([x, u] - xu_means) / xu_std) dy_std +
 * dy_means), normalisers applied as written (not folded into the weights).  The state is the observation (obs_dim ==
 * nx, no initial-state rows); data and outputs as ampc_kstep_errors.  Grid (16-row tiles, models), 256 threads.
 * Refused: depths, widths or dimensions over the limits, a model of other input / output width, obs_dim != nx, NULL
 * addresses, an address flagged as device memory that is not memory of `device`.  A diverging model yields non-finite
 * sums for itself only.  Deterministic: every sum runs in a fixed order that depends on the model's own layer widths
 * and the 16-row tile only -- a model's sums do not depend on the other models of the call or on their order.
 * Synchronises. */
int ampc_kstep_errors_mlp(int device, int n_models, const int* n_hidden, const int* dims, const int* activations,
                          const double* const* weights, const double* const* biases, const double* const* norms,
                          const int* on_device, int nx, int nu, int n_traj, const int* traj_len, int obs_dim,
                          const double* obs, const double* ctrls, int kmax, const double* inv_std, double* sq_err,
                          double* sq_delta_err);

/* ---- least-squares model fits (f64 only) ---------------------------------------------------- */
/* Fits ARX models (sysid/arx.py:62-116) and Koopman models of method "lstsq" (sysid/koopman.py:141-154) of ONE data
 * set in one call.  traj_len[n_traj]; obs [sum len][obs_dim], ctrls [sum len][ctrl_dim] (row-major, trajectories
 * concatenated, as ampc_kstep_errors takes them).  Row t of a trajectory with a successor is one design row with
 * target obs[t + 1]; trajectories of one row contribute nothing.
 * arx_history[n_arx]: one ARX configuration each (state 1 + history (obs_dim + ctrl_dim) - ctrl_dim <= 256).
 * koopman_n_basis[n_koopman] and the concatenated koopman_kinds / koopman_params (as ampc_mppi_plan_set_state_lift:
 * 0 identity, 1 power, 2 sin, 3 cos): one Koopman configuration each, state n_basis * obs_dim <= 256, basis-major;
 * configurations with the same basis share one Gram pass.
 * Outputs, ARX configurations first, each group in the order given: coeffs, packed: ARX [obs_dim][1 + history
 * (obs_dim + ctrl_dim)] in ARX's feature order, Koopman [n][n + ctrl_dim] = [A | B]; status[n_arx + n_koopman]:
 * 0 fitted, 1 not fitted here (the scaled normal equations are singular or too ill conditioned for a Cholesky
 * solve: smallest squared pivot below n_features * 2^-26; fit that model on the host); min_pivot: the smallest
 * squared pivot of the unit-diagonal Gram's factor.  Deterministic: a configuration's result does not depend on
 * the other configurations of the call or on their order.  Synchronises. */
int ampc_linfit_fit(int device, int n_traj, const int* traj_len, int obs_dim, int ctrl_dim, const double* obs,
                    const double* ctrls, int n_arx, const int* arx_history, int n_koopman,
                    const int* koopman_n_basis, const int* koopman_kinds, const double* koopman_params,
                    double* coeffs, int* status, double* min_pivot);

/* Sequentially-thresholded least-squares (STLSQ) fits of SINDy configurations of ONE data set in one call: what
 * sysid/sindy.py SINDy.train does per model (ridge normal equations on the kept features, features with
 * |coefficient| < threshold dropped, at most max_iter solves per target).  Data as ampc_linfit_fit (obs_dim 1..64,
 * ctrl_dim 1..16); a design row is row t of a trajectory with a successor, its variables [obs[t], ctrls[t]].
 * ycont: NULL or [sum len][obs_dim], the continuous-mode targets by data row (row t's derivative; rows without a
 * successor are not read as targets); the discrete target of row t is obs[t + 1].
 * Designs (distinct feature libraries): design d owns features feat_off[d] .. feat_off[d + 1] of kind / a0 / a1 / par
 * (the arrays of ampc_set_sindy: kinds 0 identity, 1 sin, 2 cos, 3 x sin(f y), 4 x cos(f y), 5 power, 6 monomial; at
 * most 272 features) and pairs pair_off[d] .. pair_off[d + 1] of pair_var / pair_exp; a monomial's a0 counts from
 * its own design's first pair.  feat_off / pair_off hold n_designs + 1 entries and start at 0.
 * Configurations: cfg_design, cfg_continuous (0: discrete targets, 1: ycont), cfg_threshold [n_configs]; alpha (the
 * ridge term) and max_iter (>= 1) hold for the call.  All Grams Theta'[Theta | Y] are formed by one launch, each
 * (configuration, target) is then solved by one workgroup on sub-matrices of its design's Gram.
 * Outputs per configuration, in order: coeffs packed [obs_dim][n_features of its design]; status: 0 fitted, 1 not
 * fitted here (in some solve of some target a diagonal entry or pivot of the unit-diagonal matrix was not positive
 * and finite, a coefficient was not finite, or the smallest squared pivot was below n_kept * 2^-26), 2 threshold tie
 * (some kept coefficient of some solve had | |coef| - threshold | / threshold < 2^-20: keep / drop could go either
 * way at rounding level; fit that model on the host); min_pivot: smallest squared pivot of all its solves;
 * min_margin: smallest such threshold margin; iterations: the largest number of solves any of its targets took.
 * Refused: sizes over the limits, max_iter < 1, a continuous configuration with ycont == NULL.  Deterministic: a
 * configuration's result does not depend on the other configurations or designs of the call or on their order.
 * Synchronises. */
int ampc_sindy_fit(int device, int n_traj, const int* traj_len, int obs_dim, int ctrl_dim, const double* obs,
                   const double* ctrls, const double* ycont, int n_designs, const int* feat_off, const int* pair_off,
                   const int* kind, const int* a0, const int* a1, const double* par, const int* pair_var,
                   const int* pair_exp, int n_configs, const int* cfg_design, const int* cfg_continuous,
                   const double* cfg_threshold, double alpha, int max_iter, double* coeffs, int* status,
                   double* min_pivot, double* min_margin, int* iterations);

/* ampc_sindy_fit for feature libraries of up to 2048 features: the same arguments, outputs, statistics and status
 * rules on a second pair of kernels (every design of the call runs on them, also those of at most 272 features; the
 * results need not be bit-equal to ampc_sindy_fit's, the order of summation differs).  Refused: a design outside
 * 1..2048 features, obs_dim outside 1..64, ctrl_dim outside 1..16, and what ampc_sindy_fit refuses.  The Grams, the
 * materialised design rows of one wave of the Gram pass and the workspaces of one wave of solves stay under a memory
 * budget of AMPC_SINDY_WIDE_BUDGET_MB MiB (environment, default 8192; one row split of one design and one pair at the
 * least); a configuration's result does not depend on how the waves were cut.  Deterministic as ampc_sindy_fit.
 * Synchronises.  (Detected by its symbol: ampc_version() stays 114.) */
int ampc_sindy_fit_wide(int device, int n_traj, const int* traj_len, int obs_dim, int ctrl_dim, const double* obs,
                        const double* ctrls, const double* ycont, int n_designs, const int* feat_off,
                        const int* pair_off, const int* kind, const int* a0, const int* a1, const double* par,
                        const int* pair_var, const int* pair_exp, int n_configs, const int* cfg_design,
                        const int* cfg_continuous, const double* cfg_threshold, double alpha, int max_iter,
                        double* coeffs, int* status, double* min_pivot, double* min_margin, int* iterations);

/* Lasso fits of Koopman models (sysid/koopman.py:150-156: sklearn's Lasso(alpha).fit with its defaults -- intercept
 * fitted and dropped, max_iter 1000, tol 1e-4, cyclic coordinate descent) of ONE data set in one call, by the same
 * descent run on the Gram.  Data as ampc_linfit_fit (obs_dim 1..256, ctrl_dim 1..16).  Bases: basis_n[n_bases] and the
 * concatenated basis_kinds / basis_params (kinds of ampc_linfit_fit; n_basis * obs_dim <= 256; duplicate functions
 * are allowed); configurations: cfg_basis, cfg_alpha [n_configs] (alpha finite, >= 0).  Per basis that a
 * configuration names, one Gram pass (the MFMA pass of ampc_linfit_fit) over the design [1 | F | Y], F = [lift(obs[t]),
 * ctrls[t]], Y = lift(obs[t + 1]); with m rows, mu = sum F / m, ybar = sum Y / m:
 *   G = F'F - m mu mu',  Q = F'Y - m mu ybar',  yy_t = Y_t'Y_t - m ybar_t^2,  a = alpha m,  tol_t = 1e-4 yy_t.
 * One wave per (configuration, target) then runs, from w = 0 and H = G w = 0, sweeps it = 0..999 over the features in
 * order: skip i if G_ii == 0; tmp = Q_it - H_i + w_i G_ii; w_new = sign(tmp) max(|tmp| - a, 0) / G_ii; if w_new != w_i:
 * H += (w_new - w_i) G[:, i]; d_w_max = max |w_new - w_i|, w_max = max |w_new|.  After a sweep with w_max == 0 or
 * d_w_max / w_max < 1e-4 or it == 999 the duality gap: dn = max |Q_t - H|, R2 = yy_t - 2 w.Q_t + w.H, Ry = yy_t - w.Q_t;
 * dn > a: c = a / dn, gap = (R2 + R2 c^2) / 2, else c = 1, gap = R2; gap += a |w|_1 - c Ry; stop when gap < tol_t.  A
 * target that reaches sweep 1000 keeps its w; a sweep that moves nothing and does not stop counts as 1000.
 * Outputs per configuration, in order: coeffs packed [n][n + ctrl_dim] = [A | B]; status: 0 fitted, 1 not fitted here
 * (a value is not finite, or the centring took half the digits of a column: G_ii < 2^-26 (F'F)_ii or
 * yy_t < 2^-26 Y_t'Y_t with the raw value non-zero; an all-zero column is skipped and keeps coefficient 0), 2 a stopping
 * decision too close to call (|gap - tol_t| <= tie tol_t at some gap check, or |d_w_max / w_max - 1e-4| <= ratio_tie 1e-4
 * at some sweep: fit that model on the host); min_margin [n_configs][2]: the smallest such gap margin and sweep-test
 * margin; sweeps: the largest sweep count of its targets.  Refused: sizes over the limits, alpha < 0 or not finite.
 * Deterministic (fixed-order sums, no atomics): a configuration's result does not depend on the other configurations
 * or bases of the call or on their order.  Synchronises. */
int ampc_lasso_fit(int device, int n_traj, const int* traj_len, int obs_dim, int ctrl_dim, const double* obs,
                   const double* ctrls, int n_bases, const int* basis_n, const int* basis_kinds,
                   const double* basis_params, int n_configs, const int* cfg_basis, const double* cfg_alpha,
                   double tie, double ratio_tie, double* coeffs, int* status, double* min_margin, int* sweeps);

/* Stable fits of Koopman configurations (f64), one per basis, of one data set in one call (reference:
 * autompc/sysid/stable_koopman.py:47-167 stabilize_discrete with its default initialisation): A = S^-1 U B S with S
 * positive definite, U orthogonal, B symmetric with eigenvalues in [0, 1] -- Schur stable by construction -- fitted by
 * the projected fast-gradient method, run on the Gram of the design [F | Y] (F = [lift(obs[t]), ctrls[t]], Y =
 * lift(obs[t + 1]); one shared Gram pass per basis, the least-squares start by the scaled Cholesky of ampc_linfit_fit),
 * one workgroup per basis: a line-search trial costs O(n^3) whatever the number of rows.  Data and bases as
 * ampc_lasso_fit; lifted states n = basis_n * obs_dim <= 64, ctrl_dim <= 16.
 *   tie: a line-search decision |e_next - e| <= tie e (or the convergence test that close to its threshold) is a tie;
 *   coeffs: per basis [n][n + ctrl_dim] = [A | B], bases in order;
 *   status [n_bases]: 0 fitted; 1 not fitted here (a Cholesky pivot under ampc_linfit_fit's rule, a polar factor of a
 *   matrix whose Gram has min eig <= 2^-40 max eig, an eigen-iteration at its 30-sweep cap, a non-finite value: coeffs
 *   NaN); 2 a decision was a tie (coeffs are the fit that followed);
 *   error [n_bases]: the final |Y - A Xs - B Xu|_F; iterations, trials [n_bases]: outer iterations and line-search
 *   trials run; min_margin [n_bases]: the smallest relative distance of a decision from its threshold.
 * Refused: sizes over the limits, no trajectory with two rows.  Deterministic (fixed-order sums, no atomics): a basis's
 * result does not depend on the other bases of the call or on their order.  Synchronises. */
int ampc_stable_fit(int device, int n_traj, const int* traj_len, int obs_dim, int ctrl_dim, const double* obs,
                    const double* ctrls, int n_bases, const int* basis_n, const int* basis_kinds,
                    const double* basis_params, double tie, double* coeffs, int* status, double* error,
                    int* iterations, int* trials, double* min_margin);

/* ---- MLP training (f64 only) ---------------------------------------------------------------------
 * MLP.train's loop (autompc/sysid/mlp.py:192-217: DataLoader(shuffle=True) mini-batches, SmoothL1Loss, Adam(lr)) for
 * n_models networks of ANY mix of depth, widths, activation and learning rate over one normalised data set, every
 * model exactly as its own training would run.  One optimiser step is one launch per layer forward and one per layer
 * backward for all models together (csrc/mlpfit_kernels.hpp); all ordering comes from kernel boundaries on `stream`.
 *   stream: the hipStream_t everything is enqueued on (e.g. torch's current stream; NULL: the default stream);
 *   n_hidden [n_models] in 1..4; dims [n_models][6]: nx + nu (<= 80), the hidden widths (<= 256), nx (<= 64), the
 *   rest ignored -- every model has the data's input and output width; activations as ampc_set_mlp; lrs: Adam's lr;
 *   feed_dev [n_rows][nx + nu], target_dev [n_rows][nx]: the normalised inputs and targets (mlp.py:179-190);
 *   n_batch in 1..4096 (mlp.py:194); the ragged last batch of an epoch is kept and averaged over its own rows;
 *   params_dev [n_params]: every model's parameters, model k from param_offsets[k] (in doubles): per layer the
 *   weight, row-major [out][in] (torch.nn.Linear's layout), then the bias [out] -- a layer's two addresses are what
 *   ampc_set_mlp_dev takes.  Models must not overlap.  Trained in place.
 * feed, target, params (and idx below) are DEVICE memory of `device`, owned by the caller and alive as long as the
 * plan; host pointers are refused.  The plan owns Adam's moments (zero at creation), the step count and the
 * activation buffers.  Refused: shapes over the limits.  Deterministic: no atomics, every sum in a fixed order that
 * depends on the model's own dimensions and the batch's row count only -- a model's result does not depend on the
 * other models of the plan. */
int ampc_mlpfit_create(int device, void* stream, int n_models, const int* n_hidden, const int* dims,
                       const int* activations, const double* lrs, const long long* param_offsets,
                       const double* feed_dev, const double* target_dev, int n_rows, int n_batch, double* params_dev,
                       long long n_params, ampc_mlpfit_plan** out);
/* One epoch (mlp.py:201-214): ceil(n_rows / n_batch) optimiser steps, step s on rows idx[k][s n_batch ..] of model k.
 * idx_dev [n_models][n_rows] int32, device memory: each model's row order of this epoch (what its DataLoader would
 * draw; entries outside 0..n_rows-1 are clamped into the data).  Only enqueues: idx_dev must stay valid until the
 * stream has run the epoch.  A later call continues the same optimisation (moments and step count persist). */
int ampc_mlpfit_run_epoch(ampc_mlpfit_plan* p, const int* idx_dev);
/* Optimiser steps enqueued so far (Adam's t). */
int ampc_mlpfit_steps(const ampc_mlpfit_plan* p, long long* steps);
/* Waits for the stream, then frees what the plan owns (mlp.py has no counterpart: the optimiser is garbage collected). */
int ampc_mlpfit_destroy(ampc_mlpfit_plan* p);

/* ---- LQR, finite and infinite horizon (f64 only) --------------------------------------------- */
/* A plan of n_problems LQR controllers (reference: autompc/control/lqr.py:139-192 FiniteHorizonLQR) that keeps
 * their gains on the device between ampc_lqr_gains and the closed loop.  obs_dim 1..256, ctrl_dim 1..16. */
int ampc_lqr_plan_create(int device, int n_problems, int obs_dim, int ctrl_dim, ampc_lqr_plan** out);
int ampc_lqr_plan_destroy(ampc_lqr_plan* p);
/* models[n_problems]: one controller model per problem, handles staged with ampc_set_linear (the reference's
 * is_compatible requires a linear model, lqr.py:161-168), f64, on the plan's device, ctrl_dim controls and
 * obs_dim..256 states; state dimensions may differ between problems.  The plan holds a reference on each.  A model
 * re-staged afterwards makes every later call on the plan fail until the models are set again. */
int ampc_lqr_plan_set_models(ampc_lqr_plan* p, ampc_handle* const* models);
/* Gains of every problem in ONE launch (_finite_horz_dt_lqr, lqr.py:35-47, with N = 0): from P = F, horizon[i] + 1
 * Riccati steps P <- A'PA - (A'PB)(R + B'PB)^-1 (B'PA) + Q, then K = -(R + B'PB)^-1 B'PA of the last P.
 *   horizons [n] in 1..1000 (LQRFactory's range, lqr.py:214-224); Q [n][obs_dim][obs_dim], R [n][nu][nu], F [n][obs_dim][obs_dim] (FiniteHorizonLQR.__init__ pads
 *   Q and F with zeros to the model state, lqr.py:146-151: so does the device);
 *   K [sum_i nu * n_i] (NULL: keep on the device only): problem i's K [nu][n_i] row-major, problems in order;
 *   status [n] (may be NULL): 0 ok, 1 R + B'PB singular (an exact zero pivot of the partial-pivot elimination) or
 *   a non-finite value -- the reference's LinAlgError / NaN; that problem's K is NaN.
 * A problem's result does not depend on the other problems of the call (fixed-order sums).  Synchronises. */
int ampc_lqr_gains(ampc_lqr_plan* p, const int* horizons, const double* Q, const double* R, const double* F,
                   double* K, int* status);
/* ampc_lqr_gains with infinite-horizon problems in the same launch (_inf_horz_dt_lqr, lqr.py:22-33, with N = 0).
 *   horizons [n]: 1..1000 a finite problem, exactly as ampc_lqr_gains computes it; 0 an infinite one: from P = Q
 *   (padded; F is not read) the same Riccati step until max|P_new - P_old| over the n_i x n_i entries is
 *   <= thresholds[i], then K of that P as above;
 *   thresholds [n]: finite and > 0 where horizons[i] == 0 (the reference's default is 1e-3), not read elsewhere;
 *   max_iters [n]: 1..100000 where horizons[i] == 0, not read elsewhere.  The reference's loop has no cap and does
 *   not return when P keeps moving (an ARX model with a bias column: its constant state adds a constant to P every
 *   step); here such a problem stops after max_iters[i] steps.  A step of a 256-state model takes about a millisecond,
 *   so the bound of 100000 keeps a workgroup that never converges to a couple of minutes;
 *   status [n] (may be NULL): 0 and 1 as ampc_lqr_gains (a NaN in max|P_new - P_old| is 1); 2 = not converged after
 *   max_iters[i] steps; K is NaN for 1 and 2;
 *   iters [n] (may be NULL): Riccati steps performed; horizons[i] + 1 for a finite problem.
 * The maximum is order-independent, so a problem's K and iters do not depend on the rest of the call either.
 * (Added without a version bump: callers detect it by its symbol.) */
int ampc_lqr_gains_ex(ampc_lqr_plan* p, const int* horizons, const double* thresholds, const int* max_iters,
                      const double* Q, const double* R, const double* F, double* K, int* status, int* iters);
/* How each problem's controller updates its model state in the closed loop (model.update_state, lqr.py:176-177):
 *   rules [n]: 0 = the observation (model state == observation), 1 = ARX shift A s + B u_prev with the
 *   observation slot overwritten (arx.py:94-99), 2 = lift of the observation (koopman.py:105-122, 166-168)
 *   with n_basis[i] basis functions (kind, parameter) taken in order from lift_kinds / lift_params (kinds of
 *   ampc_mppi_plan_set_state_lift; n_basis[i] * obs_dim = n_i); n_basis / lift_* may be NULL without rule 2;
 *   goal [n][obs_dim]: the cost's goal (state0 = goal zero-padded to the model state, lqr.py:178-182);
 *   ctrl_lo / ctrl_hi [nu]: control bounds (u is clipped, lqr.py:184-185; +-inf for none). */
int ampc_lqr_plan_set_loop(ampc_lqr_plan* p, const int* rules, const int* n_basis, const int* lift_kinds,
                           const double* lift_params, const double* goal, const double* ctrl_lo,
                           const double* ctrl_hi);
/* ampc_lqr_plan_set_loop with clip [n] (NULL: every problem clips, as ampc_lqr_plan_set_loop): clip[i] == 0 leaves
 * problem i's u = K (s - state0) as it is, whatever the bounds -- InfiniteHorizonLQR.run (lqr.py:126-136), which also
 * subtracts no goal: pass a zero goal for such a problem.  (Added without a version bump.) */
int ampc_lqr_plan_set_loop_ex(ampc_lqr_plan* p, const int* rules, const int* n_basis, const int* lift_kinds,
                              const double* lift_params, const double* goal, const double* ctrl_lo,
                              const double* ctrl_hi, const int* clip);
/* simulate(controller, init_obs, sim_model=surrogate, max_steps=n_steps) for every problem at once, on the device
 * (utils/simulation.py:44-63; FiniteHorizonLQR.run, lqr.py:174-192): per control step the controller state update,
 * u = clip(K (s - state0)), simstate = surrogate.pred(simstate, u).  Needs ampc_lqr_gains and ampc_lqr_plan_set_loop.
 *   surrogate: f64 handle with any model (MLP, SINDy, linear) whose state starts with the observation;
 *   init_state [sum_i n_i]: each problem's model.traj_to_state of the one-row trajectory (the previous control is 0);
 *   init_sim [n][surrogate state dim]: sim_model.traj_to_state of that trajectory;
 *   traj_obs [n][n_steps+1][obs_dim], traj_ctrls [n][n_steps+1][nu] (last control row zero); either may be NULL. */
int ampc_lqr_closed_loop(ampc_lqr_plan* p, ampc_handle* surrogate, const double* init_state, const double* init_sim,
                         int n_steps, double* traj_obs, double* traj_ctrls);
/* ... ending in the task-cost score of every trajectory (cost terms as ampc_score_trajectories): scores [n]. */
int ampc_lqr_closed_loop_scored(ampc_lqr_plan* p, ampc_handle* surrogate, const double* init_state,
                                const double* init_sim, int n_steps, int n_terms, const int* kinds,
                                const double* params, double* scores, double* traj_obs, double* traj_ctrls);

/* ---- Bayesian-optimisation proposal (f64) ------------------------------------------------------------------ */
/* One proposal of a model-based tuner (autompc_amd/tuning/proposer.py states the algorithm), stateless: a zero-mean
 * GP with the Matern-5/2 kernel k(a, b) = (1 + s + s^2 / 3) exp(-s), s = sqrt(5) |(a - b) o w|, of unit signal
 * variance is fitted to the n observations X [n][d] (points of the unit cube), z [n] (targets) once per row (w [d],
 * noise) of the hyperparameter table: K = k(X, X) + noise I = L L', L t = z, lml = -t't / 2 - sum log L_ii; a row whose
 * factorisation meets a pivot that is not positive and finite is declined (hyper_status 1, lml -inf).  chosen: the
 * accepted row of largest lml, lowest index on ties (-1: every row declined; picks are -1 and pick_ei, pick_margin, mu,
 * var NaN then, and the call succeeds).  For the chosen row the posterior over pool [m][d]: V = L^-1 k(X, pool),
 * mu = V't, var = max(1 - colsum V^2, 1e-12) (mu, var: before the first pick), expected improvement for minimisation
 * against min z, and q greedy picks: the unpicked point of largest EI (lowest index on ties; a NaN EI counts as
 * -inf), then the "believer" update c = k(pool, p_j) - V'V[:, j], row r = c / sqrt(max(c_j + noise, 1e-12)) appended
 * to V, var = max(var - r^2, 1e-12), the mean kept, EI recomputed.  pick_ei [q]: the pick's EI; pick_margin [q]:
 * (EI_best - EI_second) / EI_best over the unpicked points (second taken as 0 when the pick was the last unpicked
 * point; 0 when EI_best <= 0).
 * Refused before any launch: n outside 1..2048, d outside 1..64, n_hyper outside 1..64, m outside 1..65536, q outside
 * 1..min(m, 256).  Deterministic (fixed-order sums, no atomics): the same inputs give the same bits.  Synchronises. */
int ampc_bo_propose(int device, int n, int d, const double* X, const double* z, int n_hyper,
                    const double* hyper_w /*[n_hyper][d]*/, const double* hyper_noise /*[n_hyper]*/, int m,
                    const double* pool, int q, double* lml /*[n_hyper]*/, int* hyper_status /*[n_hyper]*/,
                    int* chosen, int* picks /*[q]*/, double* pick_ei, double* pick_margin, double* mu /*[m]*/,
                    double* var /*[m]*/);

#ifdef __cplusplus
}
#endif
#endif /* AUTOMPC_HIP_H */
