"""ctypes binding of libautompc_hip.so (C ABI: include/autompc_hip.h).

There is deliberately no CPU fallback: if the HIP library is missing or no
MI355X is visible, everything that computes raises ``AmpcError``.
"""
import atexit
import ctypes
import os
import weakref
from ctypes import POINTER, c_char_p, c_double, c_int, c_uint32, c_uint64, c_void_p

import numpy as np

F64, F32 = 0, 1
ACTIVATIONS = {"relu": 0, "tanh": 1, "sigmoid": 2, "selu": 3}
TERM_REFERENCE, TERM_PER_PARTICLE = 0, 1

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AMPC_LIB") or os.path.join(_HERE, "libautompc_hip.so")


class AmpcError(RuntimeError):
    code = -1          # the library call's return code


MPPI_TABLE_NO_FIT = -3     # ampc_mppi_plan_set_model_table: the table kernel's LDS map exceeds 160 KB for this plan
#                            (ampc_mppi_plan_set_sindy_models: an entry's LDS need does;
#                             ampc_mppi_plan_set_linear_models: the widest entry's does)
ILQR_TABLE_NO_FIT = -3     # ampc_ilqr_plan_set_model_table: the same for the table iteration kernel
#                            (ampc_ilqr_plan_set_sindy_models: an entry's LDS need does;
#                             ampc_ilqr_plan_set_linear_models: the widest entry's does)


_lib = None
_dp = POINTER(c_double)
_ip = POINTER(c_int)

# name -> (restype, argtypes); must list every symbol include/autompc_hip.h declares
SIGNATURES = {
    "ampc_last_error": (c_char_p, []),
    "ampc_version": (c_int, []),
    "ampc_device_count": (c_int, []),
    "ampc_create": (c_int, [c_int, c_int, c_void_p, POINTER(c_void_p)]),
    "ampc_destroy": (c_int, [c_void_p]),
    "ampc_synchronize": (c_int, [c_void_p]),
    "ampc_precision": (c_int, [c_void_p]),
    "ampc_set_mlp": (c_int, [c_void_p, c_int, c_int, c_int, _ip, c_int, POINTER(_dp),
                             POINTER(_dp), _dp, _dp, _dp, _dp]),
    "ampc_set_mlp_dev": (c_int, [c_void_p, c_int, c_int, c_int, _ip, c_int, POINTER(c_void_p),
                                 POINTER(c_void_p), c_void_p, c_void_p, c_void_p, c_void_p]),
    "ampc_jit_status": (c_int, [c_void_p, c_char_p, c_int]),
    "ampc_handle_set_jit": (c_int, [c_void_p, c_int]),
    "ampc_jit_wait": (c_int, [c_void_p]),
    "ampc_plan_kernel_kind": (c_int, [c_void_p, c_void_p]),
    "ampc_set_linear": (c_int, [c_void_p, c_int, c_int, _dp, _dp]),
    "ampc_mlp_pred_batch": (c_int, [c_void_p, _dp, _dp, _dp, c_int]),
    "ampc_mlp_pred_diff_batch": (c_int, [c_void_p, _dp, _dp, _dp, _dp, _dp, c_int]),
    "ampc_set_sindy": (c_int, [c_void_p, c_int, c_int, c_int, _ip, _ip, _ip, _dp, _dp, c_int, c_double,
                               c_int, c_int, _ip, _ip]),
    "ampc_sindy_pred_batch": (c_int, [c_void_p, _dp, _dp, _dp, c_int]),
    "ampc_sindy_pred_diff_batch": (c_int, [c_void_p, _dp, _dp, _dp, _dp, _dp, c_int]),
    "ampc_set_program": (c_int, [c_void_p, c_int, c_int, c_int, c_int, _ip, c_int, _dp, _ip]),
    "ampc_program_rollout": (c_int, [c_void_p, c_int, c_int, _dp, _dp, _dp]),
    "ampc_set_program_jvp": (c_int, [c_void_p, c_int, c_int, _ip, c_int, _dp, _ip]),
    "ampc_program_pred_diff_batch": (c_int, [c_void_p, _dp, _dp, _dp, _dp, _dp, c_int]),
    "ampc_program_set_ilqr": (c_int, [c_void_p, c_int]),
    "ampc_ilqr_plan_jacobians": (c_int, [c_void_p, _dp, _dp, c_int]),
    "ampc_set_quad_costs": (c_int, [c_void_p, c_int, c_int, _dp, _dp, _dp, _dp]),
    "ampc_set_indicator_costs": (c_int, [c_void_p, c_int, _ip, _dp]),
    "ampc_set_affine_quad_costs": (c_int, [c_void_p, c_int, c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "ampc_set_ctrl_bounds": (c_int, [c_void_p, _dp, _dp]),
    "ampc_mppi_plan_create": (c_int, [c_void_p, c_int, _ip, _ip, _dp, _dp, _ip, c_int,
                                      POINTER(c_void_p)]),
    "ampc_mppi_plan_destroy": (c_int, [c_void_p]),
    "ampc_mppi_upload": (c_int, [c_void_p, _dp, _dp, _dp]),
    "ampc_mppi_generate_eps": (c_int, [c_void_p, c_uint64, c_uint64]),
    "ampc_mppi_plan_legacy_redraws": (c_int, [c_void_p, POINTER(ctypes.c_longlong)]),
    "ampc_mppi_plan_set_noise_ids": (c_int, [c_void_p, POINTER(c_uint32)]),
    "ampc_set_mt_jump_table": (c_int, [POINTER(c_uint32), c_int, c_int]),
    "ampc_legacy_log_mode": (c_int, []),
    "ampc_mppi_legacy_normal": (c_int, [c_void_p, POINTER(c_uint32), c_int, c_int, c_double,
                                        POINTER(c_uint32), _ip, _ip, _dp]),
    "ampc_mppi_plan_set_geometry": (c_int, [c_void_p, c_int, c_int]),
    "ampc_mppi_plan_set_step_offset": (c_int, [c_void_p, c_uint64]),
    "ampc_mppi_plan_set_state_lift": (c_int, [c_void_p, c_int, _ip, _dp]),
    "ampc_mppi_solve": (c_int, [c_void_p]),
    "ampc_mppi_download": (c_int, [c_void_p, _dp, _dp, _dp, _dp]),
    "ampc_mppi_set_x0_dev": (c_int, [c_void_p, c_void_p]),
    "ampc_mppi_run": (c_int, [c_void_p, _dp, _dp, c_int, c_uint64, c_uint64, _dp]),
    "ampc_mppi_run_legacy": (c_int, [c_void_p, _dp, _dp, POINTER(c_uint32), c_int, c_int, c_double,
                                     POINTER(c_uint32), _ip, _ip, _dp, _dp]),
    "ampc_mppi_plan_info": (c_int, [c_void_p, _ip, _ip, _dp, _dp]),
    "ampc_mppi_plan_sindy_launch": (c_int, [c_void_p, _ip, _ip, _ip, _ip]),
    "ampc_mppi_sindy_launch_choice": (c_int, [c_int] * 11 + [ctypes.c_longlong, c_int, c_int, _ip, _ip, _ip, _ip]),
    "ampc_sindy_pred_lds": (c_int, [c_int] * 9 + [_ip, _ip]),
    "ampc_mppi_plan_set_outputs": (c_int, [c_void_p, c_int]),
    "ampc_mppi_plan_set_timing": (c_int, [c_void_p, c_int]),
    "ampc_mppi_plan_timing": (c_int, [c_void_p, _dp, _dp, _ip]),
    "ampc_mppi_closed_loop": (c_int, [c_void_p, c_void_p, _dp, c_int, c_uint64, _dp, _dp, _dp]),
    "ampc_score_trajectories": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, _dp, _dp, c_int,
                                        _ip, _dp, _dp]),
    "ampc_mppi_closed_loop_scored": (c_int, [c_void_p, c_void_p, _dp, c_int, c_uint64, _dp, c_int,
                                             _ip, _dp, _dp, _dp, _dp]),
    "ampc_ilqr_plan_create": (c_int, [c_void_p, c_int, c_int, c_double, _ip, c_int,
                                      POINTER(c_void_p)]),
    "ampc_ilqr_plan_destroy": (c_int, [c_void_p]),
    "ampc_ilqr_plan_set_constants": (c_int, [c_void_p, c_double, c_int, c_double, c_double]),
    "ampc_ilqr_plan_set_terminal_goal": (c_int, [c_void_p, c_int]),
    "ampc_ilqr_plan_set_timing": (c_int, [c_void_p, c_int]),
    "ampc_ilqr_plan_timing": (c_int, [c_void_p, _dp, _ip]),
    "ampc_ilqr_plan_stats": (c_int, [c_void_p, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)]),
    "ampc_ilqr_solve": (c_int, [c_void_p, _dp, _dp, c_int, _dp, _dp, _dp, _dp, _ip, _ip, _ip, _dp]),
    "ampc_ilqr_closed_loop": (c_int, [c_void_p, c_void_p, c_int, _dp, _ip, c_int, c_int, _dp, _dp, _ip, _ip,
                                      POINTER(ctypes.c_longlong)]),
    "ampc_ilqr_solve_queue": (c_int, [c_void_p, c_int, _dp, _dp, _ip, c_int, _dp, _dp, _dp, _dp, _ip, _ip, _ip,
                                      _dp]),
    "ampc_ilqr_solve_queue_var": (c_int, [c_void_p, c_int, _dp, _dp, _ip, _ip, _ip, c_int, _dp, _dp, _dp, _dp, _ip, _ip,
                                          _ip, _dp]),
    "ampc_ilqr_closed_loop_var": (c_int, [c_void_p, c_void_p, c_int, _dp, _ip, _ip, _ip, c_int, c_int, _dp, _dp, _ip,
                                          _ip, POINTER(ctypes.c_longlong)]),
    "ampc_ilqr_plan_set_models": (c_int, [c_void_p, c_int, POINTER(c_void_p)]),
    "ampc_mppi_plan_set_models": (c_int, [c_void_p, c_int, POINTER(c_void_p), _ip]),
    "ampc_mppi_plan_set_sindy_models": (c_int, [c_void_p, c_int, POINTER(c_void_p), _ip]),
    "ampc_mppi_plan_set_linear_models": (c_int, [c_void_p, c_int, POINTER(c_void_p), _ip, _ip, _ip, _ip, _dp]),
    "ampc_mppi_closed_loop_linear": (c_int, [c_void_p, c_void_p, _dp, _dp, c_int, c_uint64, _dp, c_int, _ip, _dp, _dp,
                                             _dp, _dp]),
    "ampc_ilqr_plan_set_sindy_models": (c_int, [c_void_p, c_int, POINTER(c_void_p)]),
    "ampc_ilqr_plan_set_linear_models": (c_int, [c_void_p, c_int, POINTER(c_void_p), _ip, _ip, _ip, _dp]),
    "ampc_ilqr_linear_table_layout": (c_int, [c_int, _ip, c_int, c_int, c_int, c_int, c_int, POINTER(ctypes.c_longlong),
                                              POINTER(ctypes.c_longlong)]),
    "ampc_ilqr_closed_loop_linear": (c_int, [c_void_p, c_void_p, c_int, _dp, _dp, _ip, _ip, _ip, c_int, c_int, _dp, _dp,
                                             _ip, _ip, POINTER(ctypes.c_longlong)]),
    "ampc_mppi_plan_set_model_table": (c_int, [c_void_p, c_int, _ip, _ip, _ip, POINTER(c_void_p), POINTER(c_void_p),
                                               POINTER(c_void_p), _ip, _ip]),
    "ampc_ilqr_plan_set_model_table": (c_int, [c_void_p, c_int, _ip, _ip, _ip, POINTER(c_void_p), POINTER(c_void_p),
                                               POINTER(c_void_p), _ip]),
    "ampc_kstep_errors": (c_int, [POINTER(c_void_p), c_int, c_int, _ip, c_int, _dp, _dp, _dp, c_int, _dp, _dp,
                                  _dp]),
    "ampc_kstep_errors_linear": (c_int, [POINTER(c_void_p), c_int, c_int, _ip, c_int, _dp, _dp, _ip, _ip, _ip, _ip, _dp,
                                         POINTER(c_void_p), c_int, _dp, _dp, _dp]),
    "ampc_kstep_errors_sindy": (c_int, [POINTER(c_void_p), c_int, c_int, _ip, c_int, _dp, _dp, c_int, _dp, _dp, _dp]),
    "ampc_kstep_errors_mlp": (c_int, [c_int, c_int, _ip, _ip, _ip, POINTER(c_void_p), POINTER(c_void_p),
                                      POINTER(c_void_p), _ip, c_int, c_int, c_int, _ip, c_int, _dp, _dp, c_int, _dp, _dp,
                                      _dp]),
    "ampc_lqr_plan_create": (c_int, [c_int, c_int, c_int, c_int, POINTER(c_void_p)]),
    "ampc_lqr_plan_destroy": (c_int, [c_void_p]),
    "ampc_lqr_plan_set_models": (c_int, [c_void_p, POINTER(c_void_p)]),
    "ampc_lqr_gains": (c_int, [c_void_p, _ip, _dp, _dp, _dp, _dp, _ip]),
    "ampc_lqr_gains_ex": (c_int, [c_void_p, _ip, _dp, _ip, _dp, _dp, _dp, _dp, _ip, _ip]),
    "ampc_lqr_plan_set_loop": (c_int, [c_void_p, _ip, _ip, _ip, _dp, _dp, _dp, _dp]),
    "ampc_lqr_plan_set_loop_ex": (c_int, [c_void_p, _ip, _ip, _ip, _dp, _dp, _dp, _dp, _ip]),
    "ampc_lqr_closed_loop": (c_int, [c_void_p, c_void_p, _dp, _dp, c_int, _dp, _dp]),
    "ampc_lqr_closed_loop_scored": (c_int, [c_void_p, c_void_p, _dp, _dp, c_int, c_int, _ip, _dp, _dp, _dp, _dp]),
    "ampc_linfit_fit": (c_int, [c_int, c_int, _ip, c_int, c_int, _dp, _dp, c_int, _ip, c_int, _ip, _ip, _dp, _dp, _ip,
                                _dp]),
    "ampc_sindy_fit": (c_int, [c_int, c_int, _ip, c_int, c_int, _dp, _dp, _dp, c_int, _ip, _ip, _ip, _ip, _ip, _dp, _ip,
                               _ip, c_int, _ip, _ip, _dp, c_double, c_int, _dp, _ip, _dp, _dp, _ip]),
    "ampc_sindy_fit_wide": (c_int, [c_int, c_int, _ip, c_int, c_int, _dp, _dp, _dp, c_int, _ip, _ip, _ip, _ip, _ip, _dp,
                                    _ip, _ip, c_int, _ip, _ip, _dp, c_double, c_int, _dp, _ip, _dp, _dp, _ip]),
    "ampc_lasso_fit": (c_int, [c_int, c_int, _ip, c_int, c_int, _dp, _dp, c_int, _ip, _ip, _dp, c_int, _ip, _dp,
                               c_double, c_double, _dp, _ip, _dp, _ip]),
    "ampc_stable_fit": (c_int, [c_int, c_int, _ip, c_int, c_int, _dp, _dp, c_int, _ip, _ip, _dp, c_double, _dp, _ip,
                                _dp, _ip, _ip, _dp]),
    "ampc_mlpfit_create": (c_int, [c_int, c_void_p, c_int, _ip, _ip, _ip, _dp, POINTER(ctypes.c_longlong), c_void_p,
                                   c_void_p, c_int, c_int, c_void_p, ctypes.c_longlong, POINTER(c_void_p)]),
    "ampc_mlpfit_run_epoch": (c_int, [c_void_p, c_void_p]),
    "ampc_mlpfit_steps": (c_int, [c_void_p, POINTER(ctypes.c_longlong)]),
    "ampc_mlpfit_destroy": (c_int, [c_void_p]),
    "ampc_bo_propose": (c_int, [c_int, c_int, c_int, _dp, _dp, c_int, _dp, _dp, c_int, _dp, c_int, _dp, _ip, _ip, _ip,
                                _dp, _dp, _dp, _dp]),
}


def load():
    """Load the shared library (once) and attach prototypes."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise AmpcError("libautompc_hip.so is not built (%s). Run `python -c 'import "
                        "__graft_entry__ as g; g.build()'` or `make -C autompc_amd/csrc`."
                        % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def legacy_log_mode():
    """ampc_legacy_log_mode(): 1 / 2 when the library reproduces the host C library's log() bit for
    bit (glibc's FMA / non-FMA build) -- the device-generated numpy legacy stream is then numpy's
    own, normals included -- 0 when it does not."""
    return int(load().ampc_legacy_log_mode())


def check(rc):
    if rc != 0:
        msg = load().ampc_last_error()
        err = AmpcError(msg.decode() if msg else "libautompc_hip error %d" % rc)
        err.code = int(rc)
        raise err


def sindy_launch_choice(sizes, nu, cost_stride, max_h, num_path, precision="f64", fp_allowed=True, g_forced=0):
    """ampc_mppi_sindy_launch_choice: MppiPlan.sindy_launch() from sizes alone, without a device.  sizes: (nx, n_feat,
    n_trig, n_pow, n_mon, n_pool, n_tab) of the model's feature program; num_path: the problems' sample counts."""
    nx, n_feat, n_trig, n_pow, n_mon, n_pool, n_tab = (int(v) for v in sizes)
    samples = sum((int(n) + 63) // 64 * 64 for n in np.atleast_1d(num_path))
    v = [c_int() for _ in range(4)]
    check(load().ampc_mppi_sindy_launch_choice(int(precision == "f64"), nx, int(nu), n_feat, n_trig, n_pow, n_mon, n_pool,
                                               n_tab, int(cost_stride), int(max_h), samples, int(bool(fp_allowed)),
                                               int(g_forced), *[ctypes.byref(x) for x in v]))
    return {"spread": bool(v[0].value), "lanes": v[1].value, "staged": bool(v[2].value), "lds_bytes": v[3].value}


def sindy_pred_lds(sizes, nu, precision="f64"):
    """ampc_sindy_pred_lds: (staged, LDS bytes) of the prediction kernel for a feature program of these sizes; raises
    AmpcError where pred_batch refuses the model."""
    nx, n_feat, n_trig, n_pow, n_mon, n_pool, n_tab = (int(v) for v in sizes)
    st, lb = c_int(), c_int()
    check(load().ampc_sindy_pred_lds(int(precision == "f64"), nx, int(nu), n_feat, n_trig, n_pow, n_mon, n_pool, n_tab,
                                     ctypes.byref(st), ctypes.byref(lb)))
    return bool(st.value), lb.value


def as_f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def dptr(a):
    return None if a is None else a.ctypes.data_as(_dp)


def iptr(a):
    return None if a is None else a.ctypes.data_as(_ip)


# Device objects must be destroyed before the HIP runtime's own static teardown: close every live
# plan, then every live handle, from an atexit hook (runs before interpreter/module teardown).
_live_plans = weakref.WeakSet()
_live_handles = weakref.WeakSet()


@atexit.register
def _shutdown():
    for obj in list(_live_plans) + list(_live_handles):
        try:
            obj.close()
        except Exception:
            pass


class Handle:
    """One device context: model + cost blocks + bounds on one MI355X / one stream."""

    def __init__(self, device=0, precision="f64", stream=None, jit=True):
        """jit=False: never start (or wait for) the run-time build of shape-specialised kernels for what this
        handle holds (ampc_handle_set_jit) -- models that live for one evaluation."""
        lib = load()
        if lib.ampc_device_count() <= 0:
            raise AmpcError("no HIP device visible: the MI355X path cannot run here "
                            "(there is no CPU fallback by design)")
        self.lib = lib
        self.precision = {"f64": F64, "f32": F32}[precision]
        self.precision_name = precision
        self._h = c_void_p()
        check(lib.ampc_create(int(device), self.precision, c_void_p(stream) if stream else None,
                              ctypes.byref(self._h)))
        self.device = int(device)
        if not jit:
            check(lib.ampc_handle_set_jit(self._h, 0))
        self.nx = self.nu = None
        self._plans = weakref.WeakSet()      # plans hold raw pointers into this handle
        _live_handles.add(self)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            # garbage collection may finalise a handle before the plans built on it: destroy
            # those first, they dereference the handle
            for plan in list(getattr(self, "_plans", ())):
                plan.close()
            self.lib.ampc_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        check(self.lib.ampc_synchronize(self._h))

    # -- model ---------------------------------------------------------------
    def set_mlp(self, nx, nu, weights, biases, activation, xu_means, xu_std, dy_means, dy_std):
        n_hidden = len(weights) - 1
        Ws = [as_f64(w) for w in weights]
        bs = [as_f64(b) for b in biases]
        hidden = np.array([w.shape[0] for w in Ws[:-1]], dtype=np.int32)
        sizes = [nx + nu] + [int(x) for x in hidden] + [nx]
        for l, w in enumerate(Ws):
            if w.shape != (sizes[l + 1], sizes[l]) or bs[l].shape != (sizes[l + 1],):
                raise ValueError("layer %d has shape %r, expected %r" % (l, w.shape,
                                                                          (sizes[l + 1], sizes[l])))
        wp = (_dp * len(Ws))(*[dptr(w) for w in Ws])
        bp = (_dp * len(bs))(*[dptr(b) for b in bs])
        norm = [as_f64(v) for v in (xu_means, xu_std, dy_means, dy_std)]
        if norm[0].shape != (nx + nu,) or norm[1].shape != (nx + nu,) \
                or norm[2].shape != (nx,) or norm[3].shape != (nx,):
            raise ValueError("normaliser shapes do not match (nx+nu, nx+nu, nx, nx)")
        check(self.lib.ampc_set_mlp(self._h, nx, nu, n_hidden, iptr(hidden), ACTIVATIONS[activation],
                                    wp, bp, dptr(norm[0]), dptr(norm[1]), dptr(norm[2]),
                                    dptr(norm[3])))
        self.nx, self.nu = nx, nu
        self._sindy = False

    def set_mlp_dev(self, nx, nu, hidden, weight_ptrs, bias_ptrs, activation, norm_ptrs):
        """Stage an MLP whose float64 parameters already live in this device's memory (e.g. the tensors a
        PyTorch-ROCm fit produced): `weight_ptrs[l]` / `bias_ptrs[l]` are device addresses of contiguous
        [out_l][in_l] / [out_l] arrays, `norm_ptrs` those of xu_means, xu_std, dy_means, dy_std.  Folding
        and packing run on the device (csrc/api_model.cpp); the caller's arrays are only read, and must
        be complete (their producing stream synchronised) when this is called."""
        hidden = np.array([int(x) for x in hidden], dtype=np.int32)
        if len(weight_ptrs) != len(hidden) + 1 or len(bias_ptrs) != len(hidden) + 1 or len(norm_ptrs) != 4:
            raise ValueError("one weight and one bias pointer per layer (hidden + output), four normaliser pointers")
        wp = (c_void_p * len(weight_ptrs))(*[c_void_p(int(p)) for p in weight_ptrs])
        bp = (c_void_p * len(bias_ptrs))(*[c_void_p(int(p)) for p in bias_ptrs])
        check(self.lib.ampc_set_mlp_dev(self._h, int(nx), int(nu), len(hidden), iptr(hidden), ACTIVATIONS[activation],
                                        wp, bp, *[c_void_p(int(p)) for p in norm_ptrs]))
        self.nx, self.nu = int(nx), int(nu)
        self._sindy = False

    def jit_status(self):
        """(state, message): 0 no run-time compiled kernels involved, 1 the shape plugin of the staged
        model is being compiled, 2 ready, -1 failed."""
        buf = ctypes.create_string_buffer(512)
        st = self.lib.ampc_jit_status(self._h, buf, 512)
        msg = buf.value.decode()
        if st == -1 and not getattr(self, "_jit_warned", False):
            # say it once: the controller keeps working, on the run-time-shape kernels (1.1-1.9x slower)
            import warnings
            self._jit_warned = True
            warnings.warn("autompc_amd: the kernels specialised for this model's shape could not be compiled at run "
                          "time (%s); plans on this model run the run-time-shape kernels, which are 1.1-1.9x slower. "
                          "A box without hipcc can ship a cache built elsewhere ($AMPC_JIT_CACHE)." % (msg or "no log"),
                          RuntimeWarning, stacklevel=3)
        return st, msg

    def jit_wait(self):
        """Block until the kernels specialised for the staged model's shape are compiled; plans
        created afterwards use them."""
        check(self.lib.ampc_jit_wait(self._h))

    def set_linear(self, A, B):
        """x' = A x + B u (ARX / Koopman prediction, arx.py:151-154, koopman.py:170-173)."""
        A, B = as_f64(A), as_f64(B)
        nx = A.shape[0]
        if A.ndim != 2 or A.shape != (nx, nx) or B.ndim != 2 or B.shape[0] != nx:
            raise ValueError("A must be [nx, nx] and B [nx, nu]")
        check(self.lib.ampc_set_linear(self._h, nx, B.shape[1], dptr(A), dptr(B)))
        self.nx, self.nu = nx, B.shape[1]
        self._sindy = False

    def set_sindy(self, nx, nu, kind, arg0, arg1, param, xi, continuous, dt, strict_reference=True,
                  pair_var=None, pair_exp=None):
        """pair_var / pair_exp: the (variable, exponent) pairs monomial features (kind 6) index
        with arg0 (first pair) and arg1 (number of pairs)."""
        kind = np.ascontiguousarray(kind, dtype=np.int32)
        pair_var = np.ascontiguousarray(pair_var if pair_var is not None else [], dtype=np.int32)
        pair_exp = np.ascontiguousarray(pair_exp if pair_exp is not None else [], dtype=np.int32)
        if pair_var.shape != pair_exp.shape or pair_var.ndim != 1:
            raise ValueError("pair_var and pair_exp must be 1-d arrays of equal length")
        arg0 = np.ascontiguousarray(arg0, dtype=np.int32)
        arg1 = np.ascontiguousarray(arg1, dtype=np.int32)
        param, xi = as_f64(param), as_f64(xi)
        nf = kind.shape[0]
        if xi.shape != (nx, nf) or arg0.shape != (nf,) or arg1.shape != (nf,) or param.shape != (nf,):
            raise ValueError("SINDy descriptor shapes are inconsistent")
        check(self.lib.ampc_set_sindy(self._h, nx, nu, nf, iptr(kind), iptr(arg0), iptr(arg1),
                                      dptr(param), dptr(xi), int(bool(continuous)),
                                      float(dt or 0.0), int(bool(strict_reference)),
                                      int(pair_var.shape[0]), iptr(pair_var) if pair_var.size else None,
                                      iptr(pair_exp) if pair_exp.size else None))
        self.nx, self.nu = nx, nu
        self._sindy = True

    def set_program(self, nx, nu, n_slots, code, consts, out_slot):
        """Analytic dynamics as a straight-line program (ampc_set_program; sysid/program.py): code [n_instr][4] rows
        (op, dst, a, b), consts the constant pool, out_slot [nx].  The library validates everything on the host and
        refuses a malformed program with an AmpcError before anything is uploaded.  pred_batch, program_rollout and
        the `surrogate` argument of the closed loops serve such a handle; it has no Jacobians and takes no plans
        until set_program_jvp stages its JVP."""
        code = np.ascontiguousarray(code, dtype=np.int32).reshape(-1, 4)
        consts = as_f64(consts).reshape(-1)
        out_slot = np.ascontiguousarray(out_slot, dtype=np.int32).reshape(-1)
        if out_slot.shape[0] != int(nx):
            raise ValueError("out_slot needs one entry per state")
        check(self.lib.ampc_set_program(self._h, int(nx), int(nu), int(n_slots), code.shape[0], iptr(code),
                                        consts.shape[0], dptr(consts), iptr(out_slot)))
        self.nx, self.nu = int(nx), int(nu)
        self._sindy = False

    def set_program_jvp(self, n_slots, code, consts, out_slot):
        """The JVP program of the staged program (ampc_set_program_jvp; sysid/program.py derives it): 2 (nx + nu)
        inputs [x | u | dx | du], out_slot [2 nx] = [f | J . (dx, du)].  With it the handle has pred_diff_batch and
        takes MPPI plans.  set_program and every other model call drop it."""
        code = np.ascontiguousarray(code, dtype=np.int32).reshape(-1, 4)
        consts = as_f64(consts).reshape(-1)
        out_slot = np.ascontiguousarray(out_slot, dtype=np.int32).reshape(-1)
        if self.nx is not None and out_slot.shape[0] != 2 * self.nx:
            raise ValueError("out_slot needs two entries per state")
        check(self.lib.ampc_set_program_jvp(self._h, int(n_slots), code.shape[0], iptr(code), consts.shape[0],
                                            dptr(consts), iptr(out_slot)))

    def set_program_ilqr(self, enable=True):
        """ampc_program_set_ilqr: the opt-in that lets IlqrPlan take this handle's program (f64; needs the JVP staged).
        set_program, set_program_jvp and every other model call clear it."""
        check(self.lib.ampc_program_set_ilqr(self._h, int(bool(enable))))

    def program_rollout(self, x0, ctrls):
        """ampc_program_rollout: obs [n][T+1][nx] from x0 [n][nx] under ctrls [n][T][nu], one launch."""
        x0, ctrls = as_f64(x0), as_f64(ctrls)
        n = x0.shape[0]
        if self.nx is None:                 # nothing staged: the library says so (it checks before it reads)
            check(self.lib.ampc_program_rollout(self._h, n, 0, dptr(x0), dptr(ctrls), dptr(x0)))
        if x0.shape != (n, self.nx) or ctrls.ndim != 3 or ctrls.shape[0] != n or ctrls.shape[2] != self.nu:
            raise ValueError("program_rollout: x0 %r / ctrls %r do not match (n,%d) / (n,T,%d)"
                             % (x0.shape, ctrls.shape, self.nx, self.nu))
        T = ctrls.shape[1]
        obs = np.empty((n, T + 1, self.nx))
        check(self.lib.ampc_program_rollout(self._h, n, T, dptr(x0), dptr(ctrls), dptr(obs)))
        return obs

    def pred_batch(self, states, ctrls):
        states, ctrls = as_f64(states), as_f64(ctrls)
        n = states.shape[0]
        if states.shape != (n, self.nx) or ctrls.shape != (n, self.nu):
            raise ValueError("pred_batch: states %r / ctrls %r do not match (n,%d)/(n,%d)"
                             % (states.shape, ctrls.shape, self.nx, self.nu))
        out = np.empty((n, self.nx))
        fn = self.lib.ampc_sindy_pred_batch if getattr(self, "_sindy", False) \
            else self.lib.ampc_mlp_pred_batch
        check(fn(self._h, dptr(states), dptr(ctrls), dptr(out), n))
        return out

    def pred_diff_batch(self, states, ctrls):
        states, ctrls = as_f64(states), as_f64(ctrls)
        n = states.shape[0]
        if states.shape != (n, self.nx) or ctrls.shape != (n, self.nu):
            raise ValueError("pred_diff_batch: bad shapes %r %r" % (states.shape, ctrls.shape))
        out = np.empty((n, self.nx))
        jx = np.empty((n, self.nx, self.nx))
        ju = np.empty((n, self.nx, self.nu))
        fn = self.lib.ampc_sindy_pred_diff_batch if getattr(self, "_sindy", False) \
            else self.lib.ampc_mlp_pred_diff_batch
        check(fn(self._h, dptr(states), dptr(ctrls), dptr(out), dptr(jx), dptr(ju), n))
        return out, jx, ju

    # -- cost / bounds ----------------------------------------------------------
    def set_quad_costs(self, Q, R, F, goal):
        """Q [C,no,no], R [C,nu,nu], F [C,no,no], goal [C,no] (or a single block without C)."""
        Q, R, F, goal = as_f64(Q), as_f64(R), as_f64(F), as_f64(goal)
        if Q.ndim == 2:
            Q, R, F, goal = Q[None], R[None], F[None], goal[None]
        C, no = Q.shape[0], Q.shape[1]
        if Q.shape != (C, no, no) or F.shape != (C, no, no) or R.shape != (C, self.nu, self.nu) \
                or goal.shape != (C, no):
            raise ValueError("cost block shapes are inconsistent")
        check(self.lib.ampc_set_quad_costs(self._h, C, no, dptr(Q), dptr(R), dptr(F), dptr(goal)))
        self.obs_dim = no
        self.n_costs = C

    def set_cost_blocks(self, Q, R, F, goal, lin=None, lin_term=None, consts=None):
        """Affine-quadratic cost blocks (ampc_set_affine_quad_costs; autompc_amd.costs.blocks): the
        arrays of set_quad_costs plus lin [C,no], lin_term [C,no], consts [C,2] (None = zeros)."""
        Q, R, F, goal = as_f64(Q), as_f64(R), as_f64(F), as_f64(goal)
        if Q.ndim == 2:
            Q, R, F, goal = Q[None], R[None], F[None], goal[None]
            lin, lin_term, consts = (None if a is None else as_f64(a)[None] for a in (lin, lin_term, consts))
        C, no = Q.shape[0], Q.shape[1]
        if Q.shape != (C, no, no) or F.shape != (C, no, no) or R.shape != (C, self.nu, self.nu) \
                or goal.shape != (C, no):
            raise ValueError("cost block shapes are inconsistent")
        extra = []
        for a, shape in ((lin, (C, no)), (lin_term, (C, no)), (consts, (C, 2))):
            if a is not None:
                a = as_f64(a)
                if a.shape != shape:
                    raise ValueError("cost block shapes are inconsistent")
            extra.append(a)
        check(self.lib.ampc_set_affine_quad_costs(self._h, C, no, dptr(Q), dptr(R), dptr(F), dptr(goal),
                                                  *(dptr(a) if a is not None else None for a in extra)))
        self.obs_dim = no
        self.n_costs = C

    def set_indicator_costs(self, terms=None):
        """Threshold / box terms of an MPPI controller's cost (ampc_set_indicator_costs): `terms` =
        (kinds int32[n], params f64[...]) as autompc_amd.costs.cost_terms lays them out, kinds 1 / 2 only;
        None or empty removes them.  Call after set_quad_costs / set_cost_blocks."""
        if terms is None or len(terms[0]) == 0:
            check(self.lib.ampc_set_indicator_costs(self._h, 0, None, None))
            self.n_ind = 0
            return
        kinds = np.ascontiguousarray(terms[0], dtype=np.int32)
        params = as_f64(terms[1])
        check(self.lib.ampc_set_indicator_costs(self._h, int(kinds.shape[0]), iptr(kinds), dptr(params)))
        self.n_ind = int(kinds.shape[0])

    def set_ctrl_bounds(self, lo, hi):
        lo, hi = as_f64(lo), as_f64(hi)
        check(self.lib.ampc_set_ctrl_bounds(self._h, dptr(lo), dptr(hi)))

    def score_trajectories(self, terms, obs, ctrls, obs_dim=None):
        """Cost.__call__ (cost.py:27-41) of a batch of trajectories obs [B,T,ns], ctrls [B,T,nu]
        under the cost given as `terms` = (kinds int32[n], params f64[...]) -- see
        autompc_amd.costs.cost_terms.  Returns scores [B]."""
        kinds, params = terms
        obs, ctrls = as_f64(obs), as_f64(ctrls)
        if obs.ndim != 3 or ctrls.ndim != 3 or obs.shape[:2] != ctrls.shape[:2]:
            raise ValueError("obs [B,T,ns] and ctrls [B,T,nu] expected")
        B, T, ns = obs.shape
        no = ns if obs_dim is None else int(obs_dim)
        kinds = np.ascontiguousarray(kinds, dtype=np.int32)
        params = as_f64(params)
        out = np.empty(B)
        check(self.lib.ampc_score_trajectories(
            self._h, B, T, ns, no, ctrls.shape[2], dptr(obs), dptr(ctrls), len(kinds),
            kinds.ctypes.data_as(_ip), dptr(params), dptr(out)))
        return out


class MppiPlan:
    """Device buffers + launch geometry for a batch of independent MPPI problems."""

    def __init__(self, handle, num_path, horizon, sigma, lmda, cost_index=None,
                 term_mode=TERM_REFERENCE):
        self.handle = handle
        self.lib = handle.lib
        self.N = np.atleast_1d(np.asarray(num_path, dtype=np.int32)).copy()
        self.B = self.N.shape[0]
        self.H = np.broadcast_to(np.asarray(horizon, dtype=np.int32), (self.B,)).copy()
        self.sigma = np.broadcast_to(as_f64(sigma), (self.B,)).copy()
        self.lmda = np.broadcast_to(as_f64(lmda), (self.B,)).copy()
        ci = None if cost_index is None else \
            np.broadcast_to(np.asarray(cost_index, dtype=np.int32), (self.B,)).copy()
        self._p = c_void_p()
        check(self.lib.ampc_mppi_plan_create(handle._h, self.B, iptr(self.N), iptr(self.H),
                                             dptr(self.sigma), dptr(self.lmda), iptr(ci),
                                             int(term_mode), ctypes.byref(self._p)))
        _live_plans.add(self)
        handle._plans.add(self)
        nu = handle.nu
        self.sum_hnu = int(np.sum(self.H.astype(np.int64) * nu))
        self.sum_n = int(np.sum(self.N.astype(np.int64)))
        self.sum_nhnu = int(np.sum(self.N.astype(np.int64) * self.H * nu))

    def close(self):
        if getattr(self, "_p", None) is not None and self._p:
            self.lib.ampc_mppi_plan_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _flat(self, a, size, name):
        if a is None:
            return None
        a = as_f64(a).reshape(-1)
        if a.size != size:
            raise ValueError("%s has %d elements, expected %d" % (name, a.size, size))
        return a

    def upload(self, x0=None, act_seq=None, eps=None):
        x0 = self._flat(x0, getattr(self, "_linear_x0", None) or self.B * self.handle.nx, "x0")
        act_seq = self._flat(act_seq, self.sum_hnu, "act_seq")
        eps = self._flat(eps, self.sum_nhnu, "eps")
        check(self.lib.ampc_mppi_upload(self._p, dptr(x0), dptr(act_seq), dptr(eps)))

    def generate_eps(self, seed, stream=0):
        check(self.lib.ampc_mppi_generate_eps(self._p, int(seed), int(stream)))

    _jump_table_set = False

    @classmethod
    def _install_jump_table(cls, lib):
        """MT19937 jump polynomials for the block-parallel stream generator (once per process);
        without the data file the library generates the stream sequentially."""
        if cls._jump_table_set:
            return
        cls._jump_table_set = True
        path = os.path.join(_HERE, "data", "mt19937_jump.npz")
        if os.path.exists(path):
            d = np.load(path)
            for j in d["jumps"]:           # one table per segment length
                polys = np.ascontiguousarray(d["polys_%d" % int(j)], dtype=np.uint32)
                check(lib.ampc_set_mt_jump_table(polys.ctypes.data_as(POINTER(c_uint32)), polys.shape[0], int(j)))

    def legacy_normal(self, state):
        """Fill the noise buffer with numpy's legacy normal draw for the generator state `state`
        (the tuple np.random.get_state() returns); returns the state to install afterwards."""
        self._install_jump_table(self.lib)
        name, key, pos, has_gauss, cached = state
        if name != "MT19937":
            raise ValueError("numpy's legacy global generator (MT19937) expected")
        key = np.ascontiguousarray(key, dtype=np.uint32)
        key_out = np.empty(624, dtype=np.uint32)
        pos_out, hg_out, cached_out = c_int(), c_int(), c_double()
        u32p = POINTER(c_uint32)
        check(self.lib.ampc_mppi_legacy_normal(self._p, key.ctypes.data_as(u32p), int(pos), int(has_gauss),
                                               float(cached), key_out.ctypes.data_as(u32p),
                                               ctypes.byref(pos_out), ctypes.byref(hg_out),
                                               ctypes.byref(cached_out)))
        return ("MT19937", key_out, pos_out.value, hg_out.value, cached_out.value)

    def legacy_normal_inplace(self, ls):
        """legacy_normal() on numpy's global generator where it lives (ls: _npstate.LegacyState):
        the library reads the MT19937 key from numpy's memory and writes the state after the draw
        back into it -- no get_state() / set_state() conversions (~100 us of a 450 us call)."""
        self._install_jump_table(self.lib)
        pos_out, hg_out, cached_out = c_int(), c_int(), c_double()
        with ls.lock:
            check(self.lib.ampc_mppi_legacy_normal(self._p, ls.key_ptr, int(ls.key[624]), ls.has_gauss.value,
                                                   ls.gauss.value, ls.key_ptr, ctypes.byref(pos_out),
                                                   ctypes.byref(hg_out), ctypes.byref(cached_out)))
            ls.key[624] = pos_out.value
            ls.has_gauss.value, ls.gauss.value = hg_out.value, cached_out.value

    def set_geometry(self, tile_rows=0, horizon_cap=0):
        """Fix the rollout tile height (0 = automatic, 16/32/64) and the horizon the LDS layout is
        sized for, so results do not depend on what else shares the plan.  Call before upload()."""
        check(self.lib.ampc_mppi_plan_set_geometry(self._p, int(tile_rows), int(horizon_cap)))

    def set_step_offset(self, first_step):
        """Index of the first control step of the next closed loop (its Philox stream key), for
        episodes run in segments."""
        check(self.lib.ampc_mppi_plan_set_step_offset(self._p, int(first_step)))

    def set_noise_ids(self, ids):
        """ids [B]: the key of every problem's device noise stream (default: its index in the
        plan).  With a candidate's global index here its noise is independent of the sharding."""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        if ids.shape != (self.B,):
            raise ValueError("one noise id per problem expected")
        check(self.lib.ampc_mppi_plan_set_noise_ids(self._p, ids.ctypes.data_as(POINTER(c_uint32))))

    def set_models(self, handles, model_index):
        """Controller models per problem (ampc_mppi_plan_set_models): `handles` hold MLPs of the plan's shape,
        model_index [B] names each problem's.  None / empty handles: back to the plan handle's own model."""
        hs = list(handles or [])
        arr = (c_void_p * max(len(hs), 1))(*[h._h for h in hs])
        mi = None if not hs else np.ascontiguousarray(np.broadcast_to(np.asarray(model_index, dtype=np.int32), (self.B,)))
        check(self.lib.ampc_mppi_plan_set_models(self._p, len(hs), arr, iptr(mi)))
        self._models = hs

    def set_model_table(self, models, model_index):
        """MLP models of any mix of depth, widths and activation per problem (ampc_mppi_plan_set_model_table, f64):
        `models` are sysid.MLP models of the plan handle's system, model_index [B] names each problem's.  Device-
        resident fits hand over their tensors' addresses and are read in place; the plan keeps them (and the host
        arrays of the others) alive.  The call fixes the plan's geometry to 16-row tiles: call it before upload().
        None / empty models: removes the table.  A refusal raises AmpcError; its ``code`` is MPPI_TABLE_NO_FIT when
        the plan's states / controls / horizon cap / cost block do not fit the kernel's LDS."""
        ms = list(models or [])
        if not ms:
            check(self.lib.ampc_mppi_plan_set_model_table(self._p, 0, None, None, None, None, None, None, None, None))
            self._table_args = None
            return
        from .evaluation.model_metrics import mlp_batch_args
        args = mlp_batch_args(ms)
        mi = np.ascontiguousarray(np.broadcast_to(np.asarray(model_index, dtype=np.int32), (self.B,)))
        if args["on_device"].any():
            import torch
            # (the fit's kernels have finished before the rollout reads their parameters)
            torch.cuda.current_stream(torch.device("cuda", int(self.handle.device))).synchronize()
        vpp = lambda a: a.ctypes.data_as(POINTER(c_void_p))
        check(self.lib.ampc_mppi_plan_set_model_table(
            self._p, len(ms), iptr(args["n_hidden"]), iptr(args["dims"]), iptr(args["acts"]), vpp(args["weights"]),
            vpp(args["biases"]), vpp(args["norms"]), iptr(args["on_device"]), iptr(mi)))
        self._table_args = args            # (keeps the parameters the table points into alive)

    def set_sindy_models(self, handles, model_index):
        """SINDy models of any mix of feature libraries per problem (ampc_mppi_plan_set_sindy_models): `handles` hold
        SINDy models (Handle.set_sindy) of the plan handle's dimensions, precision and device, model_index [B] names
        each problem's.  The plan keeps the handles alive; re-staging one of them needs another call.  None / empty
        handles: back to the plan handle's own model.  A refusal raises AmpcError; its ``code`` is MPPI_TABLE_NO_FIT when
        an entry's LDS need exceeds 160 KB for the plan's horizon cap and cost block."""
        hs = list(handles or [])
        arr = (c_void_p * max(len(hs), 1))(*[h._h for h in hs])
        mi = None if not hs else np.ascontiguousarray(np.broadcast_to(np.asarray(model_index, dtype=np.int32), (self.B,)))
        check(self.lib.ampc_mppi_plan_set_sindy_models(self._p, len(hs), arr, iptr(mi)))
        self._sindy_models = hs

    def set_linear_models(self, handles, model_index, rules=None, lifts=None):
        """Linear models of mixed state dimension per problem (ampc_mppi_plan_set_linear_models): `handles` hold linear
        models (Handle.set_linear, either staging form) of the plan handle's controls, precision and device,
        model_index [B] names each problem's.  ``upload``'s x0 is then ragged: the concatenation of the problems' states
        (``linear_x0_sizes``), in plan order.  rules [n_models]: the closed loop's controller-state rule per model (0 the
        observation, 1 the ARX shift, 2 a lift -- ``LqrPlan.set_loop``'s meaning); None: plain solves only.  lifts
        [n_models]: None or (kinds, params) for a rule-2 model.  None / empty handles: removes the table.  A refusal
        raises AmpcError; its ``code`` is MPPI_TABLE_NO_FIT when the widest entry's LDS map exceeds 160 KB."""
        hs = list(handles or [])
        arr = (c_void_p * max(len(hs), 1))(*[h._h for h in hs])
        if not hs:
            check(self.lib.ampc_mppi_plan_set_linear_models(self._p, 0, arr, None, None, None, None, None))
            self._linear_models, self._linear_x0, self.linear_x0_sizes = [], None, None
            return
        mi = np.ascontiguousarray(np.broadcast_to(np.asarray(model_index, dtype=np.int32), (self.B,)))
        ru = nb = lk = lp = None
        if rules is not None:
            ru = np.ascontiguousarray(rules, dtype=np.int32)
            if ru.shape != (len(hs),):
                raise ValueError("rules has %d entries, expected one per model (%d)" % (ru.size, len(hs)))
            lifts = list(lifts) if lifts is not None else [None] * len(hs)
            nb = np.zeros(len(hs), dtype=np.int32)
            kinds, params = [], []
            for i, lf in enumerate(lifts):
                if ru[i] == 2:
                    if lf is None:
                        raise ValueError("model %d has rule 2 (lift) and no lift" % i)
                    nb[i] = len(lf[0])
                    kinds.extend(int(k) for k in lf[0])
                    params.extend(float(q) for q in lf[1])
            lk = np.ascontiguousarray(kinds + [0], dtype=np.int32)
            lp = as_f64(params + [0.0])
        check(self.lib.ampc_mppi_plan_set_linear_models(self._p, len(hs), arr, iptr(mi), iptr(ru), iptr(nb), iptr(lk),
                                                        dptr(lp)))
        self._linear_models = hs            # (kept alive on this side as well)
        ok = all(0 <= int(i) < len(hs) for i in mi)
        self.linear_x0_sizes = np.array([hs[int(i)].nx for i in mi], dtype=np.int64) if ok else None
        self._linear_x0 = int(self.linear_x0_sizes.sum())

    def closed_loop_linear(self, surrogate, n_steps, init_states=None, init_sim=None, terms=None, seed=0, eps_all=None,
                           return_trajectories=True):
        """simulate() for every problem of a plan on a table of linear models (ampc_mppi_closed_loop_linear), device
        resident: per control step every controller state follows its model's rule, one rollout launch solves every
        problem, `surrogate` advances.  init_states: the concatenated model states (each model's traj_to_state of the
        one-row trajectory), init_sim [B, surrogate nx]; both None: continue from where the previous call stopped.
        Returns (scores or None, traj_obs [B, n_steps+1, surrogate nx] or None, traj_ctrls or None)."""
        nu, snx = self.handle.nu, surrogate.nx
        if (init_states is None) != (init_sim is None):
            raise ValueError("init_states and init_sim are given together or not at all")
        init_states = self._flat(init_states, getattr(self, "_linear_x0", None) or 0, "init_states")
        init_sim = self._flat(init_sim, self.B * snx, "init_sim")
        eps_all = self._flat(eps_all, n_steps * self.sum_nhnu, "eps_all")
        kinds = params = scores = None
        if terms is not None:
            kinds = np.ascontiguousarray(terms[0], dtype=np.int32)
            params = as_f64(terms[1])
            scores = np.empty(self.B)
        obs = np.empty((self.B, n_steps + 1, snx)) if return_trajectories else None
        ctl = np.empty((self.B, n_steps + 1, nu)) if return_trajectories else None
        check(self.lib.ampc_mppi_closed_loop_linear(
            self._p, surrogate._h, dptr(init_states), dptr(init_sim), int(n_steps), int(seed), dptr(eps_all),
            0 if kinds is None else len(kinds), iptr(kinds), dptr(params), dptr(scores), dptr(obs), dptr(ctl)))
        return scores, obs, ctl

    def solve(self):
        check(self.lib.ampc_mppi_solve(self._p))

    def download(self, act_seq=True, u=True, costs=False, eps_out=False):
        nu = self.handle.nu
        a = np.empty(self.sum_hnu) if act_seq else None
        uu = np.empty((self.B, nu)) if u else None
        c = np.empty(self.sum_n) if costs else None
        e = np.empty(self.sum_nhnu) if eps_out else None
        check(self.lib.ampc_mppi_download(self._p, dptr(a), dptr(uu), dptr(c), dptr(e)))
        return a, uu, c, e

    def run(self, x0, act_seq=None, philox=None):
        """One control step in a single call: x0 (and optionally a new warm start) in, noise (the
        buffer as it is, or fresh Philox noise when philox=(seed, stream)), solve, controls
        [B, nu] out."""
        nx, nu = self.handle.nx, self.handle.nu
        x0 = self._flat(x0, self.B * nx, "x0")
        act_seq = self._flat(act_seq, self.sum_hnu, "act_seq")
        u = np.empty((self.B, nu))
        seed, stream = philox if philox is not None else (0, 0)
        check(self.lib.ampc_mppi_run(self._p, dptr(x0), dptr(act_seq), 0 if philox is None else 1,
                                     int(seed), int(stream), dptr(u)))
        return u

    def legacy_redraws(self):
        """Draws repeated because a bounded wait inside the draw kernel expired (ampc_mppi_plan_legacy_redraws)."""
        n = ctypes.c_longlong()
        check(self.lib.ampc_mppi_plan_legacy_redraws(self._p, ctypes.byref(n)))
        return int(n.value)

    def run_legacy_inplace(self, x0, act_seq, ls):
        """run() with the reference's own noise: numpy's legacy draw from the global generator
        where it lives (ls: _npstate.LegacyState; see legacy_normal_inplace) and the solve, in one
        library call with one synchronisation (ampc_mppi_run_legacy)."""
        self._install_jump_table(self.lib)
        nx, nu = self.handle.nx, self.handle.nu
        x0 = self._flat(x0, self.B * nx, "x0")
        act_seq = self._flat(act_seq, self.sum_hnu, "act_seq")
        u = np.empty((self.B, nu))
        pos_out, hg_out, cached_out = c_int(), c_int(), c_double()
        with ls.lock:
            check(self.lib.ampc_mppi_run_legacy(self._p, dptr(x0), dptr(act_seq), ls.key_ptr, int(ls.key[624]),
                                                ls.has_gauss.value, ls.gauss.value, ls.key_ptr,
                                                ctypes.byref(pos_out), ctypes.byref(hg_out),
                                                ctypes.byref(cached_out), dptr(u)))
            ls.key[624] = pos_out.value
            ls.has_gauss.value, ls.gauss.value = hg_out.value, cached_out.value
        return u

    def set_x0_dev(self, ptr):
        check(self.lib.ampc_mppi_set_x0_dev(self._p, c_void_p(ptr)))

    def set_state_lift(self, kinds, params):
        """The controller model rebuilds its state from every observation (Koopman): x0 = the basis
        functions (kind 0 identity, 1 power, 2 sin, 3 cos; parameter) applied to the observation.  The
        closed loop then carries the simulation model's state: init_obs and the recorded rows have the
        SURROGATE's state width."""
        kinds = np.ascontiguousarray(kinds, dtype=np.int32)
        params = as_f64(params)
        check(self.lib.ampc_mppi_plan_set_state_lift(self._p, len(kinds), iptr(kinds), dptr(params)))
        self._lift = len(kinds) > 0

    def _loop_width(self, surrogate):
        if getattr(self, "_lift", False):
            return (surrogate if surrogate is not None else self.handle).nx
        return self.handle.nx

    def closed_loop(self, init_obs, n_steps, seed=0, eps_all=None, surrogate=None):
        """simulate() for every problem of the plan, device resident.  Returns
        (traj_obs [B, n_steps+1, nx], traj_ctrls [B, n_steps+1, nu])."""
        nx, nu = self._loop_width(surrogate), self.handle.nu
        init_obs = self._flat(init_obs, self.B * nx, "init_obs")
        eps_all = self._flat(eps_all, n_steps * self.sum_nhnu, "eps_all")
        obs = np.empty((self.B, n_steps + 1, nx))
        ctl = np.empty((self.B, n_steps + 1, nu))
        check(self.lib.ampc_mppi_closed_loop(self._p, surrogate._h if surrogate is not None else None,
                                             dptr(init_obs), int(n_steps), int(seed), dptr(eps_all),
                                             dptr(obs), dptr(ctl)))
        return obs, ctl

    def closed_loop_scored(self, init_obs, n_steps, terms, seed=0, eps_all=None, surrogate=None,
                           return_trajectories=False):
        """closed_loop + cost(traj) on the device (eval_cfg's simulate + score,
        pipeline_tuner.py:222-233); only the B scores come back unless return_trajectories."""
        nx, nu = self._loop_width(surrogate), self.handle.nu
        init_obs = self._flat(init_obs, self.B * nx, "init_obs")
        eps_all = self._flat(eps_all, n_steps * self.sum_nhnu, "eps_all")
        kinds = np.ascontiguousarray(terms[0], dtype=np.int32)
        params = as_f64(terms[1])
        scores = np.empty(self.B)
        obs = np.empty((self.B, n_steps + 1, nx)) if return_trajectories else None
        ctl = np.empty((self.B, n_steps + 1, nu)) if return_trajectories else None
        check(self.lib.ampc_mppi_closed_loop_scored(
            self._p, surrogate._h if surrogate is not None else None, dptr(init_obs), int(n_steps),
            int(seed), dptr(eps_all), len(kinds), kinds.ctypes.data_as(_ip), dptr(params),
            dptr(scores), dptr(obs), dptr(ctl)))
        return (scores, obs, ctl) if return_trajectories else scores

    def kernel_kind(self):
        """0 run-time-shape kernels, 1 a shape registered at build time, 2 a run-time compiled plugin."""
        return int(self.lib.ampc_plan_kernel_kind(self._p, None))

    def set_outputs(self, keep_eps_out=True):
        check(self.lib.ampc_mppi_plan_set_outputs(self._p, int(bool(keep_eps_out))))

    def set_timing(self, enable=True, every=1):
        """Bracket the kernels of every `every`-th solve with HIP events (timing())."""
        check(self.lib.ampc_mppi_plan_set_timing(self._p, max(1, int(every)) if enable else 0))

    def timing(self):
        r, u, n = c_double(), c_double(), c_int()
        check(self.lib.ampc_mppi_plan_timing(self._p, ctypes.byref(r), ctypes.byref(u),
                                             ctypes.byref(n)))
        return {"rollout_ms": r.value, "update_ms": u.value, "count": n.value}

    def info(self):
        wg, spw = c_int(), c_int()
        fl, by = c_double(), c_double()
        check(self.lib.ampc_mppi_plan_info(self._p, ctypes.byref(wg), ctypes.byref(spw),
                                           ctypes.byref(fl), ctypes.byref(by)))
        return {"workgroups": wg.value, "samples_per_wg": spw.value, "flops": fl.value,
                "bytes": by.value}

    def sindy_launch(self):
        """The rollout kernel solve() launches for this plan on its handle's SINDy model
        (ampc_mppi_plan_sindy_launch): spread (features over `lanes` lanes per sample) or one thread per sample,
        whether the feature program is staged in LDS, and the launch's LDS bytes."""
        v = [c_int() for _ in range(4)]
        check(self.lib.ampc_mppi_plan_sindy_launch(self._p, *[ctypes.byref(x) for x in v]))
        return {"spread": bool(v[0].value), "lanes": v[1].value, "staged": bool(v[2].value), "lds_bytes": v[3].value}


class IlqrPlan:
    """Device buffers for a batch of B independent iLQR problems of horizon H."""

    def __init__(self, handle, B, horizon, dt, cost_index=None, clip_to_bounds=False,
                 terminal_goal=False):
        self.handle = handle
        self.lib = handle.lib
        self.B, self.H = int(B), int(horizon)
        ci = None if cost_index is None else \
            np.broadcast_to(np.asarray(cost_index, dtype=np.int32), (self.B,)).copy()
        self._p = c_void_p()
        check(self.lib.ampc_ilqr_plan_create(handle._h, self.B, self.H, float(dt), iptr(ci),
                                             int(bool(clip_to_bounds)), ctypes.byref(self._p)))
        _live_plans.add(self)
        handle._plans.add(self)
        if terminal_goal:      # QuadCost(strict_reference=False): terminal gradient about the goal
            check(self.lib.ampc_ilqr_plan_set_terminal_goal(self._p, 1))

    def close(self):
        if getattr(self, "_p", None) is not None and self._p:
            self.lib.ampc_ilqr_plan_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_constants(self, u_threshold=1e-3, ls_max_iter=10, ls_discount=0.2, ls_cost_threshold=0.3):
        """compute_ilqr_default's keyword constants (ilqr.py:100-101) for the solves that follow."""
        check(self.lib.ampc_ilqr_plan_set_constants(self._p, float(u_threshold), int(ls_max_iter), float(ls_discount),
                                                    float(ls_cost_threshold)))

    def set_timing(self, enable=True, every=1):
        """Bracket the kernels of an iteration with HIP events (timing()); every > 1: only every n-th iteration of a
        queue (solve_queue)."""
        check(self.lib.ampc_ilqr_plan_set_timing(self._p, max(1, int(every)) if enable else 0))

    def timing(self):
        ms = np.zeros(4)
        n = c_int()
        check(self.lib.ampc_ilqr_plan_timing(self._p, dptr(ms), ctypes.byref(n)))
        return {"riccati_ms": ms[0], "iter_ms": ms[1], "forward_ms": ms[2], "jacobian_ms": ms[3],
                "launches": n.value}

    def kernel_kind(self):
        return int(self.lib.ampc_plan_kernel_kind(None, self._p))

    def stats(self):
        """Work of the last solve: iterations launched and line-search candidate rows rolled out
        (summed over the plan's problems)."""
        it, rows = ctypes.c_longlong(), ctypes.c_longlong()
        check(self.lib.ampc_ilqr_plan_stats(self._p, ctypes.byref(it), ctypes.byref(rows)))
        return {"iterations": it.value, "candidate_rows": rows.value}

    def jacobians(self):
        """(jx [B][H][nx][nx], ju [B][H][nx][nu]) as the last refresh left them (ampc_ilqr_plan_jacobians)."""
        nx, nu = self.handle.nx, self.handle.nu
        jx, ju = np.empty((self.B, self.H, nx, nx)), np.empty((self.B, self.H, nx, nu))
        check(self.lib.ampc_ilqr_plan_jacobians(self._p, dptr(jx), dptr(ju), 0))
        return jx, ju

    def set_jacobians(self, jx, ju):
        """Overwrite the plan's Jacobian rows (tests: which rows does a refresh leave alone?)."""
        nx, nu = self.handle.nx, self.handle.nu
        jx, ju = as_f64(jx).reshape(self.B, self.H, nx, nx), as_f64(ju).reshape(self.B, self.H, nx, nu)
        check(self.lib.ampc_ilqr_plan_jacobians(self._p, dptr(jx), dptr(ju), 1))

    def solve(self, x0, uguess, max_iter=50):
        nx, nu, B, H = self.handle.nx, self.handle.nu, self.B, self.H
        x0 = as_f64(x0).reshape(B, nx)
        uguess = as_f64(uguess).reshape(B, H, nu)
        out = {"states": np.empty((B, H + 1, nx)), "ctrls": np.empty((B, H, nu)),
               "Ks": np.empty((B, H, nu, nx)), "ks": np.empty((B, H, nu)),
               "converged": np.zeros(B, dtype=np.int32), "iters": np.zeros(B, dtype=np.int32),
               "status": np.zeros(B, dtype=np.int32), "objective": np.empty(B)}
        check(self.lib.ampc_ilqr_solve(self._p, dptr(x0), dptr(uguess), int(max_iter),
                                       dptr(out["states"]), dptr(out["ctrls"]), dptr(out["Ks"]),
                                       dptr(out["ks"]), iptr(out["converged"]), iptr(out["iters"]),
                                       iptr(out["status"]), dptr(out["objective"])))
        return out

    def _horizons(self, horizon, n):
        if horizon is None:
            return None
        hz = np.ascontiguousarray(np.broadcast_to(np.asarray(horizon, dtype=np.int32), (n,)))
        if hz.min() < 1 or hz.max() > self.H:
            raise ValueError("horizons must lie in [1, %d] (the plan's horizon)" % self.H)
        return hz

    def set_models(self, handles):
        """Controller models per problem (ampc_ilqr_plan_set_models): `handles` hold MLPs of the plan's shape;
        solve_queue / closed_loop then take model_index.  None / empty removes the table."""
        hs = list(handles or [])
        arr = (c_void_p * max(len(hs), 1))(*[h._h for h in hs])
        check(self.lib.ampc_ilqr_plan_set_models(self._p, len(hs), arr))
        self._models = hs                   # (kept alive on this side as well)

    def set_model_table(self, models):
        """MLP models of any mix of depth, widths and activation (ampc_ilqr_plan_set_model_table, f64): `models` are
        sysid.MLP models of the plan handle's system; solve_queue / closed_loop then take model_index (entry 0
        without it).  Device-resident fits hand over their tensors' addresses and are read in place; the plan keeps
        them (and the host arrays of the others) alive.  None / empty models: removes the table.  A refusal raises
        AmpcError; its ``code`` is ILQR_TABLE_NO_FIT when the plan's states / controls / cost block do not fit the
        kernel's LDS."""
        ms = list(models or [])
        if not ms:
            check(self.lib.ampc_ilqr_plan_set_model_table(self._p, 0, None, None, None, None, None, None, None))
            self._table_args = None
            return
        from .evaluation.model_metrics import mlp_batch_args
        args = mlp_batch_args(ms)
        if args["on_device"].any():
            import torch
            # (the fit's kernels have finished before the solves read their parameters)
            torch.cuda.current_stream(torch.device("cuda", int(self.handle.device))).synchronize()
        vpp = lambda a: a.ctypes.data_as(POINTER(c_void_p))
        check(self.lib.ampc_ilqr_plan_set_model_table(
            self._p, len(ms), iptr(args["n_hidden"]), iptr(args["dims"]), iptr(args["acts"]), vpp(args["weights"]),
            vpp(args["biases"]), vpp(args["norms"]), iptr(args["on_device"])))
        self._table_args = args            # (keeps the parameters the table points into alive)

    def set_sindy_models(self, handles):
        """SINDy models of any mix of feature libraries (ampc_ilqr_plan_set_sindy_models, f64): `handles` hold SINDy
        models of the plan handle's state and control dimensions; solve_queue / closed_loop then take model_index
        (entry 0 without it).  The plan keeps the handles alive.  None / empty handles: back to the plan handle's own
        model.  A refusal raises AmpcError; its ``code`` is ILQR_TABLE_NO_FIT when an entry's LDS need exceeds 160 KB."""
        hs = list(handles or [])
        arr = (c_void_p * max(len(hs), 1))(*[h._h for h in hs])
        check(self.lib.ampc_ilqr_plan_set_sindy_models(self._p, len(hs), arr))
        self._sindy_models = hs             # (kept alive on this side as well)

    def set_linear_models(self, handles, rules=None, lifts=None):
        """Linear models of mixed state dimension (ampc_ilqr_plan_set_linear_models, f64): `handles` hold linear models
        (Handle.set_linear, either staging form) of the plan handle's controls, precision and device, at most 128
        states each; solve_queue then takes model_index and a ragged x0, closed_loop_linear runs episodes.  rules
        [n_models]: the closed loop's controller-state rule per model (0 the observation, 1 the ARX shift, 2 a lift --
        ``MppiPlan.set_linear_models``' meaning); None: solves only.  lifts [n_models]: None or (kinds, params) for a
        rule-2 model.  None / empty handles: removes the table.  A refusal raises AmpcError; its ``code`` is
        ILQR_TABLE_NO_FIT when the widest entry's LDS need exceeds 160 KB."""
        hs = list(handles or [])
        arr = (c_void_p * max(len(hs), 1))(*[h._h for h in hs])
        if not hs:
            check(self.lib.ampc_ilqr_plan_set_linear_models(self._p, 0, arr, None, None, None, None))
            self._linear_models, self.linear_nx = [], None
            return
        ru = nb = lk = lp = None
        if rules is not None:
            ru = np.ascontiguousarray(rules, dtype=np.int32)
            if ru.shape != (len(hs),):
                raise ValueError("rules has %d entries, expected one per model (%d)" % (ru.size, len(hs)))
            lifts = list(lifts) if lifts is not None else [None] * len(hs)
            nb = np.zeros(len(hs), dtype=np.int32)
            kinds, params = [], []
            for i, lf in enumerate(lifts):
                if ru[i] == 2:
                    if lf is None:
                        raise ValueError("model %d has rule 2 (lift) and no lift" % i)
                    nb[i] = len(lf[0])
                    kinds.extend(int(k) for k in lf[0])
                    params.extend(float(q) for q in lf[1])
            lk = np.ascontiguousarray(kinds + [0], dtype=np.int32)
            lp = as_f64(params + [0.0])
        check(self.lib.ampc_ilqr_plan_set_linear_models(self._p, len(hs), arr, iptr(ru), iptr(nb), iptr(lk), dptr(lp)))
        self._linear_models = hs            # (kept alive on this side as well)
        self.linear_nx = np.array([h.nx for h in hs], dtype=np.int64)

    def _linear_split(self, model_index, n):
        """Per-problem state dimensions of a plan that holds a table of linear models."""
        mi = np.zeros(n, dtype=np.int32) if model_index is None else self._model_index(model_index, n)
        if mi.min() < 0 or mi.max() >= len(self.linear_nx):
            raise ValueError("model_index out of range")
        return mi, self.linear_nx[mi]

    def _linear_ragged(self, rows, sizes, name):
        """A list of per-problem vectors (or their concatenation) -> the ragged f64 array the library reads."""
        if isinstance(rows, (list, tuple)):
            rows = np.concatenate([as_f64(r).ravel() for r in rows])
        flat = as_f64(rows).ravel()
        if flat.size != int(sizes.sum()):
            raise ValueError("%s has %d values, expected %d (the problems' own state dimensions)"
                             % (name, flat.size, int(sizes.sum())))
        return flat

    def closed_loop_linear(self, surrogate, init_states, init_sim, n_steps, cost_index=None, max_iter=50, horizon=None,
                           model_index=None):
        """simulate() with IterativeLQR controllers on a table of linear models with rules (ampc_ilqr_closed_loop_linear),
        device resident, any surrogate: init_states: per episode its model's traj_to_state of the one-row trajectory (a
        list, or the concatenation); init_sim [C, surrogate nx].  Returns dict(obs [C, n_steps+1, surrogate nx], ctrls
        [C, n_steps+1, nu], failed [C], steps [C], iterations [C])."""
        if not getattr(self, "_linear_models", None):
            raise ValueError("the plan holds no table of linear models (set_linear_models)")
        sur = surrogate if surrogate is not None else self.handle
        nu, snx = self.handle.nu, sur.nx
        init_sim = as_f64(init_sim).reshape(-1, snx)
        C = init_sim.shape[0]
        mi, sizes = self._linear_split(model_index, C)
        x0 = self._linear_ragged(init_states, sizes, "init_states")
        ci = None if cost_index is None else np.ascontiguousarray(np.broadcast_to(
            np.asarray(cost_index, dtype=np.int32), (C,)))
        hz = self._horizons(horizon, C)
        out = {"obs": np.empty((C, n_steps + 1, snx)), "ctrls": np.empty((C, n_steps + 1, nu)),
               "failed": np.zeros(C, dtype=np.int32), "steps": np.zeros(C, dtype=np.int32),
               "iterations": np.zeros(C, dtype=np.int64)}
        check(self.lib.ampc_ilqr_closed_loop_linear(
            self._p, surrogate._h if surrogate is not None else None, C, dptr(x0), dptr(init_sim), iptr(ci), iptr(hz),
            iptr(mi), int(n_steps), int(max_iter), dptr(out["obs"]), dptr(out["ctrls"]), iptr(out["failed"]),
            iptr(out["steps"]), out["iterations"].ctypes.data_as(POINTER(ctypes.c_longlong))))
        return out

    def _solve_queue_linear(self, x0, uguess, cost_index, max_iter, gains, trajectories, horizon, model_index):
        """solve_queue on a table of linear models: ragged x0, per-problem arrays back."""
        nu, H = self.handle.nu, self.H
        P = len(x0) if isinstance(x0, (list, tuple)) else len(np.atleast_1d(model_index))
        mi, sizes = self._linear_split(model_index, P)
        x0 = self._linear_ragged(x0, sizes, "x0")
        nxw = int(self.linear_nx.max())
        ug = None if uguess is None else as_f64(uguess).reshape(P, H, nu)
        ci = None if cost_index is None else np.ascontiguousarray(np.broadcast_to(
            np.asarray(cost_index, dtype=np.int32), (P,)))
        hz = self._horizons(horizon, P)
        out = {"converged": np.zeros(P, dtype=np.int32), "iters": np.zeros(P, dtype=np.int32),
               "status": np.zeros(P, dtype=np.int32), "objective": np.empty(P)}
        st = ct = Kb = kb = None
        if trajectories:
            st, ct = np.empty((P, (H + 1) * nxw)), np.empty((P, H, nu))
        if gains:
            Kb, kb = np.empty((P, H * nu * nxw)), np.empty((P, H, nu))
        check(self.lib.ampc_ilqr_solve_queue_var(self._p, P, dptr(x0), dptr(ug), iptr(ci), iptr(hz), iptr(mi), int(max_iter),
                                                 dptr(st), dptr(ct), dptr(Kb), dptr(kb), iptr(out["converged"]),
                                                 iptr(out["iters"]), iptr(out["status"]), dptr(out["objective"])))
        # a problem's region keeps the widest entry's stride; its rows are packed at its own nx, the rest is zero
        if trajectories:
            out["states"] = [st[j, :(H + 1) * n].reshape(H + 1, n) for j, n in enumerate(sizes)]
            out["ctrls"] = ct
            out["states_tail"] = [st[j, (H + 1) * n:] for j, n in enumerate(sizes)]
        if gains:
            out["Ks"] = [Kb[j, :H * nu * n].reshape(H, nu, n) for j, n in enumerate(sizes)]
            out["ks"] = kb
            out["Ks_tail"] = [Kb[j, H * nu * n:] for j, n in enumerate(sizes)]
        return out

    def _model_index(self, model_index, n):
        if model_index is None:
            return None
        return np.ascontiguousarray(np.broadcast_to(np.asarray(model_index, dtype=np.int32), (n,)))

    def closed_loop(self, init_obs, n_steps, cost_index=None, max_iter=50, surrogate=None, horizon=None,
                    model_index=None):
        """simulate() with IterativeLQR controllers for C episodes, device resident (ampc_ilqr_closed_loop):
        init_obs [C, nx]; returns dict(obs [C, n_steps+1, nx], ctrls [C, n_steps+1, nu], failed [C],
        steps [C], iterations [C]).  horizon [C] (optional): each episode's iLQR horizon, at most the
        plan's (ampc_ilqr_closed_loop_var)."""
        nx, nu = self.handle.nx, self.handle.nu
        init_obs = as_f64(init_obs).reshape(-1, nx)
        C = init_obs.shape[0]
        ci = None if cost_index is None else np.ascontiguousarray(np.broadcast_to(
            np.asarray(cost_index, dtype=np.int32), (C,)))
        hz = self._horizons(horizon, C)
        mi = self._model_index(model_index, C)
        out = {"obs": np.empty((C, n_steps + 1, nx)), "ctrls": np.empty((C, n_steps + 1, nu)),
               "failed": np.zeros(C, dtype=np.int32), "steps": np.zeros(C, dtype=np.int32),
               "iterations": np.zeros(C, dtype=np.int64)}
        check(self.lib.ampc_ilqr_closed_loop_var(
            self._p, surrogate._h if surrogate is not None else None, C, dptr(init_obs), iptr(ci), iptr(hz), iptr(mi),
            int(n_steps), int(max_iter), dptr(out["obs"]), dptr(out["ctrls"]), iptr(out["failed"]),
            iptr(out["steps"]), out["iterations"].ctypes.data_as(POINTER(ctypes.c_longlong))))
        return out

    def solve_queue(self, x0, uguess=None, cost_index=None, max_iter=50, gains=True, trajectories=True,
                    horizon=None, model_index=None):
        """P problems streamed through the plan's B slots (ampc_ilqr_solve_queue): a slot whose problem
        is finished takes the next one at the following iteration boundary, on the device.  x0 [P, nx];
        uguess [P, H, nu] or None (zeros); cost_index [P] or None (block 0).  Per-problem results are
        bit-identical to one-problem solves.  gains / trajectories = False skip those downloads.
        horizon [P] (optional): each problem's own horizon, at most the plan's (ampc_ilqr_solve_queue_var):
        arrays keep the plan's H as their stride, rows past a problem's horizon come back zero.
        On a table of linear models (set_linear_models): x0 is a list of the problems' own states (or their
        concatenation, with model_index of length P); "states" and "Ks" come back as lists of per-problem arrays
        [H+1, nx_j] and [H, nu, nx_j] ("states_tail" / "Ks_tail": what lies behind them in the problem's region: zeros)."""
        if getattr(self, "_linear_models", None):
            return self._solve_queue_linear(x0, uguess, cost_index, max_iter, gains, trajectories, horizon, model_index)
        nx, nu, H = self.handle.nx, self.handle.nu, self.H
        x0 = as_f64(x0).reshape(-1, nx)
        P = x0.shape[0]
        ug = None if uguess is None else as_f64(uguess).reshape(P, H, nu)
        ci = None if cost_index is None else np.ascontiguousarray(np.broadcast_to(
            np.asarray(cost_index, dtype=np.int32), (P,)))
        out = {"converged": np.zeros(P, dtype=np.int32), "iters": np.zeros(P, dtype=np.int32),
               "status": np.zeros(P, dtype=np.int32), "objective": np.empty(P)}
        if trajectories:
            out["states"], out["ctrls"] = np.empty((P, H + 1, nx)), np.empty((P, H, nu))
        if gains:
            out["Ks"], out["ks"] = np.empty((P, H, nu, nx)), np.empty((P, H, nu))
        hz = self._horizons(horizon, P)
        mi = self._model_index(model_index, P)
        check(self.lib.ampc_ilqr_solve_queue_var(self._p, P, dptr(x0), dptr(ug), iptr(ci), iptr(hz), iptr(mi), int(max_iter),
                                                 dptr(out.get("states")), dptr(out.get("ctrls")), dptr(out.get("Ks")),
                                                 dptr(out.get("ks")), iptr(out["converged"]), iptr(out["iters"]),
                                                 iptr(out["status"]), dptr(out["objective"])))
        return out


def ilqr_linear_table_layout(nx, nu, obs_dim, B, H, ls_n=10):
    """(entry_off [n, 3], strides dict) of ampc_ilqr_plan_set_linear_models for models of nx[n] states
    (ampc_ilqr_linear_table_layout: no device needed)."""
    nx = np.ascontiguousarray(nx, dtype=np.int32)
    off = np.zeros((len(nx), 3), dtype=np.int64)
    st = np.zeros(10, dtype=np.int64)
    ll = POINTER(ctypes.c_longlong)
    check(load().ampc_ilqr_linear_table_layout(len(nx), iptr(nx), int(nu), int(obs_dim), int(B), int(H), int(ls_n),
                                               off.ctypes.data_as(ll), st.ctypes.data_as(ll)))
    names = ("states", "ctrls", "Ks", "ks", "ls_states", "ls_ctrls", "vj", "table_values", "sweep_lds_bytes", "ls_lds_bytes")
    return off, {k: int(v) for k, v in zip(names, st)}


class LqrPlan:
    """LQR controllers of B problems, finite and infinite horizon (ampc_lqr_*): linear controller models of any state
    dimension up to 256 in one plan, gains kept on the device for the closed loop.  f64 only."""

    def __init__(self, models, obs_dim, ctrl_dim, device=0):
        """models: B f64 Handles staged with set_linear (one per problem; the same handle may repeat)."""
        lib = load()
        if lib.ampc_device_count() <= 0:
            raise AmpcError("no HIP device visible: the MI355X path cannot run here "
                            "(there is no CPU fallback by design)")
        self.lib, self.models = lib, list(models)
        self.B, self.no, self.nu = len(self.models), int(obs_dim), int(ctrl_dim)
        self._p = c_void_p()
        check(lib.ampc_lqr_plan_create(int(device), self.B, self.no, self.nu, ctypes.byref(self._p)))
        _live_plans.add(self)
        for h in set(self.models):
            h._plans.add(self)
        arr = (c_void_p * self.B)(*[h._h for h in self.models])
        check(lib.ampc_lqr_plan_set_models(self._p, arr))
        self.n = np.array([int(h.nx) for h in self.models])
        self.k_off = np.concatenate([[0], np.cumsum(self.nu * self.n)])

    def close(self):
        if getattr(self, "_p", None) is not None and self._p:
            self.lib.ampc_lqr_plan_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def gains(self, horizons, Q, R, F):
        """K of every problem (list of [nu][n_i] arrays) and status [B] (0 ok, 1 singular / non-finite)."""
        B, no, nu = self.B, self.no, self.nu
        hz = np.broadcast_to(np.asarray(horizons, dtype=np.int32), (B,)).copy()
        Q = as_f64(np.broadcast_to(Q, (B, no, no)))
        R = as_f64(np.broadcast_to(R, (B, nu, nu)))
        F = as_f64(np.broadcast_to(F, (B, no, no)))
        K = np.empty(int(self.k_off[-1]))
        status = np.zeros(B, dtype=np.int32)
        check(self.lib.ampc_lqr_gains(self._p, iptr(hz), dptr(Q), dptr(R), dptr(F), dptr(K), iptr(status)))
        return [K[self.k_off[i]:self.k_off[i + 1]].reshape(nu, self.n[i]) for i in range(B)], status

    def gains_ex(self, horizons, Q, R, F, thresholds=1e-3, max_iters=10000):
        """gains() with infinite-horizon problems in the same launch (ampc_lqr_gains_ex): horizons[i] == 0 iterates
        the Riccati step from P = Q until max|dP| <= thresholds[i] (F is not read), at most max_iters[i] steps (up to
        100000; a step of a 256-state model takes about a millisecond, so lower it where models may not converge).
        Returns (K list, status [B], iters [B]): status 0 ok, 1 singular / non-finite, 2 not converged (K NaN for 1
        and 2); iters the Riccati steps performed (horizon + 1 for a finite problem)."""
        B, no, nu = self.B, self.no, self.nu
        hz = np.broadcast_to(np.asarray(horizons, dtype=np.int32), (B,)).copy()
        th = as_f64(np.broadcast_to(np.asarray(thresholds, dtype=np.float64), (B,)))
        mi = np.broadcast_to(np.asarray(max_iters, dtype=np.int32), (B,)).copy()
        Q = as_f64(np.broadcast_to(Q, (B, no, no)))
        R = as_f64(np.broadcast_to(R, (B, nu, nu)))
        F = as_f64(np.broadcast_to(F, (B, no, no)))
        K = np.empty(int(self.k_off[-1]))
        status = np.zeros(B, dtype=np.int32)
        iters = np.zeros(B, dtype=np.int32)
        check(self.lib.ampc_lqr_gains_ex(self._p, iptr(hz), dptr(th), iptr(mi), dptr(Q), dptr(R), dptr(F), dptr(K),
                                         iptr(status), iptr(iters)))
        return [K[self.k_off[i]:self.k_off[i + 1]].reshape(nu, self.n[i]) for i in range(B)], status, iters

    def set_loop(self, rules, goal, ctrl_lo, ctrl_hi, lifts=None, clip=None):
        """rules [B]: 0 observation, 1 ARX shift, 2 lift; lifts: per problem None or (kinds, params); goal [B][no]
        (or [no]); ctrl_lo / ctrl_hi [nu]; clip [B] (None: every problem clips): 0 leaves that problem's control
        unclipped (InfiniteHorizonLQR.run, which also subtracts no goal: give it a zero goal)."""
        B = self.B
        rules = np.asarray(rules, dtype=np.int32).reshape(B).copy()
        nb = np.zeros(B, dtype=np.int32)
        kinds, params = [], []
        for i in range(B):
            if rules[i] == 2:
                k, p = lifts[i]
                nb[i] = len(k)
                kinds += [int(v) for v in k]
                params += [float(v) for v in p]
        kinds = np.array(kinds + [0], dtype=np.int32)
        params = np.array(params + [0.0])
        goal = as_f64(np.broadcast_to(goal, (B, self.no)))
        if clip is None:
            check(self.lib.ampc_lqr_plan_set_loop(self._p, iptr(rules), iptr(nb), iptr(kinds), dptr(params),
                                                  dptr(goal), dptr(as_f64(ctrl_lo)), dptr(as_f64(ctrl_hi))))
            return
        clip = np.asarray(clip, dtype=np.int32).reshape(B).copy()
        check(self.lib.ampc_lqr_plan_set_loop_ex(self._p, iptr(rules), iptr(nb), iptr(kinds), dptr(params), dptr(goal),
                                                 dptr(as_f64(ctrl_lo)), dptr(as_f64(ctrl_hi)), iptr(clip)))

    def closed_loop(self, surrogate, init_states, init_sim, n_steps, terms=None, trajectories=True):
        """Episodes of n_steps control steps against `surrogate` (a Handle).  init_states: list of each problem's
        initial model state; init_sim [B][surrogate state dim].  Returns (obs [B][T+1][no], ctrls [B][T+1][nu])
        or, with cost `terms` ((kinds, params) of ampc_score_trajectories), (scores, obs, ctrls)."""
        B, T1 = self.B, int(n_steps) + 1
        st = as_f64(np.concatenate([np.asarray(s, dtype=np.float64).ravel() for s in init_states]))
        sim = as_f64(init_sim).reshape(B, -1)
        obs = np.empty((B, T1, self.no)) if trajectories else None
        ctl = np.empty((B, T1, self.nu)) if trajectories else None
        if terms is None:
            check(self.lib.ampc_lqr_closed_loop(self._p, surrogate._h, dptr(st), dptr(sim), int(n_steps), dptr(obs),
                                                dptr(ctl)))
            return obs, ctl
        kinds, params = terms
        kinds = np.ascontiguousarray(kinds, dtype=np.int32)
        params = as_f64(params)
        scores = np.empty(B)
        check(self.lib.ampc_lqr_closed_loop_scored(self._p, surrogate._h, dptr(st), dptr(sim), int(n_steps),
                                                   len(kinds), iptr(kinds), dptr(params), dptr(scores), dptr(obs),
                                                   dptr(ctl)))
        return scores, obs, ctl


class MlpFitPlan:
    """ampc_mlpfit_*: the MLP training loop for a table of models over one data set.  Every array is DEVICE memory the
    caller owns and keeps alive (addresses, e.g. ``tensor.data_ptr()``); the plan owns Adam's state."""

    MAX_HIDDEN, MAX_WIDTH, MAX_IN, MAX_OUT, MAX_BATCH = 4, 256, 80, 64, 4096

    def __init__(self, n_hidden, dims, activations, lrs, param_offsets, feed_ptr, target_ptr, n_rows, n_batch,
                 params_ptr, n_params, device=0, stream=None):
        """dims [K][6] int32 (input, hidden widths, output, padding), param_offsets [K] int64 (doubles)."""
        lib = load()
        if lib.ampc_device_count() <= 0:
            raise AmpcError("no HIP device visible: the MI355X path cannot run here "
                            "(there is no CPU fallback by design)")
        self.lib = lib
        nh = np.ascontiguousarray(n_hidden, dtype=np.int32)
        K = self.K = len(nh)
        dims = np.ascontiguousarray(dims, dtype=np.int32).reshape(K, 6)
        acts = np.array([ACTIVATIONS[a] for a in activations], dtype=np.int32)
        lrs = as_f64(lrs).reshape(K)
        offs = np.ascontiguousarray(param_offsets, dtype=np.int64).reshape(K)
        self._p = c_void_p()
        check(lib.ampc_mlpfit_create(int(device), c_void_p(stream) if stream else None, K, iptr(nh), iptr(dims),
                                     iptr(acts), dptr(lrs), offs.ctypes.data_as(POINTER(ctypes.c_longlong)),
                                     c_void_p(feed_ptr), c_void_p(target_ptr), int(n_rows), int(n_batch),
                                     c_void_p(params_ptr), int(n_params), ctypes.byref(self._p)))
        _live_plans.add(self)

    def run_epoch(self, idx_ptr):
        """One epoch on the row orders idx [K][n_rows] int32 (device address); only enqueues."""
        check(self.lib.ampc_mlpfit_run_epoch(self._p, c_void_p(idx_ptr)))

    @property
    def steps(self):
        n = ctypes.c_longlong(0)
        check(self.lib.ampc_mlpfit_steps(self._p, ctypes.byref(n)))
        return int(n.value)

    def close(self):
        if getattr(self, "_p", None) is not None and self._p:
            self.lib.ampc_mlpfit_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _fit_data(traj_len, obs, ctrls):
    """The library and the data set of a fit call, coerced and checked: (lib, lens, obs, ctrls, obs_dim, ctrl_dim)."""
    lib = load()
    if lib.ampc_device_count() <= 0:
        raise AmpcError("no HIP device visible: the MI355X path cannot run here "
                        "(there is no CPU fallback by design)")
    obs, ctrls = as_f64(obs), as_f64(ctrls)
    lens = np.ascontiguousarray(traj_len, dtype=np.int32)
    if int(lens.sum()) != obs.shape[0] or obs.shape[0] != ctrls.shape[0]:
        raise ValueError("traj_len does not add up to the rows of obs / ctrls")
    return lib, lens, obs, ctrls, obs.shape[1], ctrls.shape[1]


def linfit_fit(traj_len, obs, ctrls, arx_histories=(), koopman_bases=(), device=0):
    """ampc_linfit_fit: least-squares fits of ARX histories and Koopman bases ((kinds, params) pairs) of one data set.
    obs [R][no], ctrls [R][nu]: the trajectories concatenated, traj_len their lengths.  Returns (coeffs, status,
    min_pivot): a list of coefficient matrices -- ARX [no][1 + k (no + nu)], Koopman [n][n + nu] -- ARX configurations
    first, and the two per-configuration arrays."""
    lib, lens, obs, ctrls, no, nu = _fit_data(traj_len, obs, ctrls)
    hist = np.ascontiguousarray(list(arx_histories) + [0], dtype=np.int32)
    n_arx, n_koop = len(hist) - 1, len(koopman_bases)
    nb = np.array([len(k) for k, _ in koopman_bases] + [0], dtype=np.int32)
    kinds = np.array([int(v) for k, _ in koopman_bases for v in k] + [0], dtype=np.int32)
    params = np.array([float(v) for _, p in koopman_bases for v in p] + [0.0])
    shapes = [(no, 1 + int(k) * (no + nu)) for k in hist[:-1]] + [(int(b) * no, int(b) * no + nu) for b in nb[:-1]]
    off = np.concatenate([[0], np.cumsum([r * c for r, c in shapes])]).astype(np.int64)
    coeffs = np.empty(int(off[-1]))
    status = np.zeros(n_arx + n_koop, dtype=np.int32)
    pivot = np.empty(n_arx + n_koop)
    check(lib.ampc_linfit_fit(int(device), len(lens), iptr(lens), no, nu, dptr(obs), dptr(ctrls), n_arx, iptr(hist),
                              n_koop, iptr(nb), iptr(kinds), dptr(params), dptr(coeffs), iptr(status), dptr(pivot)))
    return [coeffs[off[i]:off[i + 1]].reshape(shapes[i]) for i in range(len(shapes))], status, pivot


def sindy_fit_wide(traj_len, obs, ctrls, designs, configs, ycont=None, alpha=0.05, max_iter=20, device=0):
    """ampc_sindy_fit_wide: ``sindy_fit`` for feature libraries of up to 2048 features, on the wide kernels (the
    same arguments and results; every design of the call runs on them)."""
    return _sindy_fit_entry("ampc_sindy_fit_wide", traj_len, obs, ctrls, designs, configs, ycont, alpha, max_iter,
                            device)


def sindy_fit(traj_len, obs, ctrls, designs, configs, ycont=None, alpha=0.05, max_iter=20, device=0):
    """ampc_sindy_fit: sequentially-thresholded least-squares fits of SINDy configurations of one data set.
    obs [R][nx], ctrls [R][nu]: the trajectories concatenated, traj_len their lengths; ycont: None or [R][nx], the
    continuous-mode targets by data row.  designs: feature libraries, the ``(kind, a0, a1, par, pair_var, pair_exp)``
    tuples of ``sysid.sindy.build_library``; configs: ``(design index, continuous, threshold)`` triples.  Returns
    (coeffs, status, min_pivot, min_margin, iterations): a list of [nx][n_features] matrices and four
    per-configuration arrays (status 0 fitted, 1 pivot rule, 2 threshold tie)."""
    return _sindy_fit_entry("ampc_sindy_fit", traj_len, obs, ctrls, designs, configs, ycont, alpha, max_iter, device)


def _sindy_fit_entry(_entry, traj_len, obs, ctrls, designs, configs, ycont, alpha, max_iter, device):
    lib, lens, obs, ctrls, nx, nu = _fit_data(traj_len, obs, ctrls)
    if ycont is not None:
        ycont = as_f64(ycont)
        if ycont.shape != obs.shape:
            raise ValueError("ycont must have the shape of obs")
    i32 = lambda parts: np.ascontiguousarray(np.concatenate([np.asarray(p, dtype=np.int32).ravel() for p in parts]
                                                            + [np.zeros(1, dtype=np.int32)]))
    feat_off = np.concatenate([[0], np.cumsum([len(d[0]) for d in designs])]).astype(np.int32)
    pair_off = np.concatenate([[0], np.cumsum([len(d[4]) for d in designs])]).astype(np.int32)
    kind, a0, a1 = (i32([d[k] for d in designs]) for k in (0, 1, 2))
    pvar, pexp = (i32([d[k] for d in designs]) for k in (4, 5))
    par = as_f64(np.concatenate([np.asarray(d[3], dtype=np.float64).ravel() for d in designs] + [np.zeros(1)]))
    cd = np.ascontiguousarray([c[0] for c in configs] + [0], dtype=np.int32)
    cc = np.ascontiguousarray([1 if c[1] else 0 for c in configs] + [0], dtype=np.int32)
    ct = as_f64([float(c[2]) for c in configs] + [0.0])
    C = len(configs)
    if C and (cd[:C].min() < 0 or cd[:C].max() >= len(designs)):
        raise ValueError("a configuration names no design")
    shapes = [(nx, int(feat_off[cd[i] + 1] - feat_off[cd[i]])) for i in range(C)]
    off = np.concatenate([[0], np.cumsum([r * c for r, c in shapes])]).astype(np.int64)
    coeffs = np.empty(int(off[-1]))
    status = np.zeros(C, dtype=np.int32)
    pivot, margin = np.empty(C), np.empty(C)
    iters = np.zeros(C, dtype=np.int32)
    check(getattr(lib, _entry)(int(device), len(lens), iptr(lens), nx, nu, dptr(obs), dptr(ctrls), dptr(ycont),
                               len(designs), iptr(feat_off), iptr(pair_off), iptr(kind), iptr(a0), iptr(a1), dptr(par),
                               iptr(pvar), iptr(pexp), C, iptr(cd), iptr(cc), dptr(ct), float(alpha), int(max_iter),
                               dptr(coeffs), iptr(status), dptr(pivot), dptr(margin), iptr(iters)))
    return [coeffs[off[i]:off[i + 1]].reshape(shapes[i]) for i in range(C)], status, pivot, margin, iters


def lasso_fit(traj_len, obs, ctrls, bases, configs, tie=None, ratio_tie=None, device=0):
    """ampc_lasso_fit: lasso fits of Koopman configurations of one data set by coordinate descent on the Gram.
    obs [R][no], ctrls [R][nu]: the trajectories concatenated, traj_len their lengths.  bases: (kinds, params) pairs;
    configs: (basis index, lasso_alpha) pairs.  tie / ratio_tie: the margins below which a stopping decision is a tie
    (None: ``sysid.lasso_fit.TIE`` / ``RATIO_TIE``).  Returns (coeffs, status, min_margin, sweeps): a list of
    [n][n + nu] matrices and three per-configuration arrays (status 0 fitted, 1 not fitted here, 2 tie; min_margin
    [.][2]: gap margin, sweep-test margin; sweeps: the largest over the targets)."""
    from .sysid.lasso_fit import RATIO_TIE, TIE
    lib, lens, obs, ctrls, no, nu = _fit_data(traj_len, obs, ctrls)
    nb = np.array([len(k) for k, _ in bases] + [0], dtype=np.int32)
    kinds = np.array([int(v) for k, _ in bases for v in k] + [0], dtype=np.int32)
    params = np.array([float(v) for _, p in bases for v in p] + [0.0])
    C = len(configs)
    cb = np.ascontiguousarray([int(c[0]) for c in configs] + [0], dtype=np.int32)
    ca = as_f64([float(c[1]) for c in configs] + [0.0])
    if C and (cb[:C].min() < 0 or cb[:C].max() >= len(bases)):
        raise ValueError("a configuration names no basis")
    shapes = [(int(nb[cb[i]]) * no, int(nb[cb[i]]) * no + nu) for i in range(C)]
    off = np.concatenate([[0], np.cumsum([r * c for r, c in shapes])]).astype(np.int64)
    coeffs = np.empty(int(off[-1]))
    status = np.zeros(C, dtype=np.int32)
    margin = np.empty((C, 2))
    sweeps = np.zeros(C, dtype=np.int32)
    check(lib.ampc_lasso_fit(int(device), len(lens), iptr(lens), no, nu, dptr(obs), dptr(ctrls), len(bases), iptr(nb),
                             iptr(kinds), dptr(params), C, iptr(cb), dptr(ca), float(TIE if tie is None else tie),
                             float(RATIO_TIE if ratio_tie is None else ratio_tie), dptr(coeffs), iptr(status),
                             dptr(margin), iptr(sweeps)))
    return [coeffs[off[i]:off[i + 1]].reshape(shapes[i]) for i in range(C)], status, margin, sweeps


def bo_propose(X, z, hyper_w, hyper_noise, pool, q, device=0):
    """ampc_bo_propose: one Bayesian-optimisation proposal (``tuning/proposer.py`` states the algorithm): a Matern-5/2
    GP fitted to X [n][d], z [n] for every row (hyper_w [G][d], hyper_noise [G]) of the hyperparameter table, the
    posterior of the row of largest log marginal likelihood over pool [m][d] and q greedy expected-improvement picks
    with the believer update.  Returns a dict: lml [G], status [G] (1: the row was declined), chosen (-1: every row
    declined; the picks are -1 and the other values NaN then), picks [q], pick_ei [q], pick_margin [q], mu [m],
    var [m] (the posterior before the first pick).  Sizes over the limits are refused (AmpcError)."""
    lib = load()
    X, pool, hw = as_f64(X), as_f64(pool), as_f64(hyper_w)
    z, hn = as_f64(z).ravel(), as_f64(hyper_noise).ravel()
    if X.ndim != 2 or pool.ndim != 2 or hw.ndim != 2:
        raise ValueError("X, pool and hyper_w must be two-dimensional")
    n, d = X.shape
    m, G, q = pool.shape[0], hw.shape[0], int(q)
    if pool.shape[1] != d or hw.shape[1] != d or z.shape[0] != n or hn.shape[0] != G:
        raise ValueError("shapes disagree: X [n][d], z [n], hyper_w [G][d], hyper_noise [G], pool [m][d]")
    lml, mu, var = np.empty(max(G, 1)), np.empty(max(m, 1)), np.empty(max(m, 1))
    status = np.zeros(max(G, 1), dtype=np.int32)
    picks = np.full(max(q, 1), -1, dtype=np.int32)
    pick_ei, pick_margin = np.empty(max(q, 1)), np.empty(max(q, 1))
    chosen = np.full(1, -1, dtype=np.int32)
    check(lib.ampc_bo_propose(int(device), n, d, dptr(X), dptr(z), G, dptr(hw), dptr(hn), m, dptr(pool), q, dptr(lml),
                              iptr(status), iptr(chosen), iptr(picks), dptr(pick_ei), dptr(pick_margin), dptr(mu),
                              dptr(var)))
    return dict(lml=lml[:G], status=status[:G], chosen=int(chosen[0]), picks=picks[:q], pick_ei=pick_ei[:q],
                pick_margin=pick_margin[:q], mu=mu[:m], var=var[:m])


def stable_fit(traj_len, obs, ctrls, bases, tie=None, device=0):
    """ampc_stable_fit: stable fits of Koopman configurations of one data set, the projected fast-gradient method of
    ``sysid/stable_fit.py`` on the Gram.  obs [R][no], ctrls [R][nu]: the trajectories concatenated, traj_len their
    lengths.  bases: (kinds, params) pairs, one configuration each (lifted states <= 64).  tie: the margin below which
    a line-search decision is a tie (None: ``sysid.stable_fit.TIE``).  Returns (coeffs, status, error, iterations,
    trials, min_margin): a list of [n][n + nu] matrices ``[A | B]`` and five per-basis arrays (status 0 fitted, 1 not
    fitted here, 2 tie)."""
    from .sysid.stable_fit import TIE
    lib, lens, obs, ctrls, no, nu = _fit_data(traj_len, obs, ctrls)
    C = len(bases)
    nb = np.array([len(k) for k, _ in bases] + [0], dtype=np.int32)
    kinds = np.array([int(v) for k, _ in bases for v in k] + [0], dtype=np.int32)
    params = np.array([float(v) for _, p in bases for v in p] + [0.0])
    shapes = [(int(nb[i]) * no, int(nb[i]) * no + nu) for i in range(C)]
    off = np.concatenate([[0], np.cumsum([r * c for r, c in shapes])]).astype(np.int64)
    coeffs = np.empty(int(off[-1]))
    status, iters, trials = (np.zeros(C, dtype=np.int32) for _ in range(3))
    error, margin = np.empty(C), np.empty(C)
    check(lib.ampc_stable_fit(int(device), len(lens), iptr(lens), no, nu, dptr(obs), dptr(ctrls), C, iptr(nb),
                              iptr(kinds), dptr(params), float(TIE if tie is None else tie), dptr(coeffs),
                              iptr(status), dptr(error), iptr(iters), iptr(trials), dptr(margin)))
    return [coeffs[off[i]:off[i + 1]].reshape(shapes[i]) for i in range(C)], status, error, iters, trials, margin
