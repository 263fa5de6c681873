"""Model prediction accuracy: k-step RMSE and RMSMENS (reference: autompc/evaluation/model_metrics.py).

What it replaces.  ``get_model_rmse(model, trajs, horizon)`` (model_metrics.py:12-43) rolls the model
``horizon`` steps from every start point of every trajectory with one ``pred_batch`` call per step and
trajectory, and ``get_model_rmsmens(model, trajs, horiz)`` (:45-111) scores the last step's increment against
the observed one, normalised by the element-wise std of the trajectories' increments.  A curve over horizons
1..kmax (``KstepPredAccGraph``, graphs/kstep_graph.py) redoes every step for every horizon.

Here ``model_errors(models, trajs, horizons, metric)`` scores many models at many horizons at once: device
models (``MLP``; ``ARX`` / ``Koopman`` of at most 64 states) are grouped by shape and each group is ONE
``ampc_kstep_errors`` call, which rolls every start point ``max(horizons)`` steps on the GPU and returns the
error sums of every horizon (csrc/kstep_kernels.hpp).  Every other model -- SINDy, wide linear models, any
foreign ``Model`` -- takes the host fallback, the reference's own algorithm over ``model.pred_batch``.

``sindy_kstep="device"`` (opt-in; the default ``"host"`` is the path above, bit for bit) scores ``SINDy`` models on
the GPU: they are grouped by ``(precision, device, obs_dim, ctrl_dim)`` (``sindy_kstep_key``) and each group is ONE
``ampc_kstep_errors_sindy`` call, whatever mix of feature libraries, coefficients and time modes it holds
(csrc/kstep_sindy_kernels.hpp).  The state is the observation; the device step is ``pred_batch``'s own.

``mlp_kstep="batch"`` (opt-in; the default ``"shape"`` is the path above, bit for bit) scores f64 ``MLP`` models of ANY
mix of depth, widths and activation together: they are grouped by ``(device, obs_dim, ctrl_dim)`` (``mlp_batch_key``) and
each group is ONE ``ampc_kstep_errors_mlp`` call -- one launch over (row tiles, models) that reads the plain
``torch.nn.Linear``-layout parameters through a device table (csrc/kstep_mlp_kernels.hpp).  No model of such a call is
staged into a handle: a model whose fit left its parameters on the device (``fit_mlps``, either fit) hands over their
addresses, the others their numpy arrays, uploaded once by the call.  The step applies the normalisers as
``pred_batch`` of the reference does (not folded into the weights), so it agrees with the per-shape path at rounding
level, not bit for bit.  f32 models, subclasses with their own ``pred_batch`` and models over the entry's limits keep
the per-shape path.

``linear_kstep="device"`` (opt-in; the default ``"host"`` is the path above, bit for bit) scores trained
``_LinearModel``s of 65..256 states on the GPU too: they are grouped by ``(precision, device, ctrl_dim)``
(``wide_linear_key``) and each group is ONE ``ampc_kstep_errors_linear`` call, whatever mix of state dimensions it
holds -- ARX histories 4..10 and Koopman lifts side by side (csrc/kstep_linear_kernels.hpp).  Initial states are
formed on the device by the model's state rule (``linear_state_rule``: the ARX lag gather, the Koopman lift, or
``traj_to_states`` rows uploaded for that model only); the ARX gather is bit-identical to ``traj_to_states``, the
lift's powers / sin / cos differ from numpy's at rounding level.  ``model_errors`` fills a ``KstepReport`` (also kept
as ``model_metrics.last_report``): ``host_fallbacks`` counts the models the host loop scored.

Definitions (the reference's, for horizon h; only start points t with t + h <= L_i - 1 count, so a trajectory
of at most h rows contributes nothing):
    RMSE(h)    = sqrt(S_h / N_h),  S_h = sum over counted rows and the first obs_dim state entries of
                 (x_pred - obs[t + h])^2, N_h = number of counted rows  (= the reference's sqrt(mean * obs_dim))
    RMSMENS(h) = sqrt(D_h / (N_h * obs_dim)),  D_h = sum of ((dx_pred - dobs) / std)^2 over the same rows, where
                 dx_pred = x_h - x_{h-1}, dobs = obs[t + h] - obs[t + h - 1] and std is the ddof-0 std of
                 obs[1:] - obs[:-1] over the given trajectories
Models with ``traj_to_states`` (ARX, Koopman) start from those states and compare ``state[:, :obs_dim]``.

Deviations from the reference (bugs not reproduced):
  * the reference's RMSMENS calls ``model.pred_parallel``, which its own models lack; the
    models here have that alias, and the host fallback calls ``pred_batch``;
  * RMSMENS of a model whose state is not the observation raises ``ValueError`` (the reference fails with a
    shape error).
"""
import numpy as np

from .. import _lib

METRICS = ("rmse", "rmsmens")
_DEVICE_MAX_LINEAR_STATES = 64          # wider linear models are refused by ampc_kstep_errors
_WIDE_MAX_LINEAR_STATES = 256           # ampc_set_linear / ampc_kstep_errors_linear
_WIDE_MAX_CTRLS = 16
_LDS_BYTES = 160 * 1024
LINEAR_KSTEP = ("host", "device")
SINDY_KSTEP = ("host", "device")
MLP_KSTEP = ("shape", "batch")
_MLP_BATCH_MAX_HIDDEN, _MLP_BATCH_MAX_WIDTH = 4, 256        # csrc/kstep_mlp_kernels.hpp
_MLP_BATCH_MAX_IN, _MLP_BATCH_MAX_STATES = 80, 64
_MLP_BATCH_LAYERS = _MLP_BATCH_MAX_HIDDEN + 1               # pointer slots per model
_SINDY_MAX_TAB = 160                    # kSindyMaxTab (csrc/sindy_kernels.hpp)
_SINDY_STAGE_BYTES = 48 * 1024          # kSindyStageBytes
_SINDY_ROWS, _SINDY_CHUNK, _SINDY_ERR_STRIDE = 64, 8, 65      # csrc/kstep_sindy_kernels.hpp


class KstepReport:
    """What one ``model_errors`` call did: ``device_models`` scored by ``ampc_kstep_errors``, ``wide_models`` by
    ``ampc_kstep_errors_linear`` in ``wide_calls`` calls, ``sindy_models`` by ``ampc_kstep_errors_sindy`` in
    ``sindy_calls`` calls, ``mlp_batch_models`` by ``ampc_kstep_errors_mlp`` in ``mlp_batch_calls`` calls,
    ``host_fallbacks`` by the host loop over ``pred_batch``."""

    def __init__(self):
        self.device_models = self.wide_models = self.wide_calls = self.host_fallbacks = 0
        self.sindy_models = self.sindy_calls = 0
        self.mlp_batch_models = self.mlp_batch_calls = 0

    def __repr__(self):
        return ("KstepReport(device_models=%d, wide_models=%d, wide_calls=%d, sindy_models=%d, sindy_calls=%d, "
                "mlp_batch_models=%d, mlp_batch_calls=%d, host_fallbacks=%d)"
                % (self.device_models, self.wide_models, self.wide_calls, self.sindy_models, self.sindy_calls,
                   self.mlp_batch_models, self.mlp_batch_calls, self.host_fallbacks))


last_report = KstepReport()


def normalize(means, std, A):
    """(A - means) / std column by column (model_metrics.py:6-10)."""
    At = []
    for i in range(A.shape[1]):
        At.append((A[:, i] - means[i]) / std[i])
    return np.vstack(At).T


def _obs_dim(trajs, model=None):
    if trajs:
        return trajs[0].system.obs_dim
    return model.system.obs_dim


def _increment_stats(trajs):
    """Element-wise mean and ddof-0 std of obs[1:] - obs[:-1] over all trajectories (model_metrics.py:93-95)."""
    dY = np.concatenate([traj.obs[1:, :] - traj.obs[:-1, :] for traj in trajs])
    return np.mean(dY, axis=0), np.std(dY, axis=0)


def _check_rmsmens_model(model, obs_dim):
    if hasattr(model, "traj_to_states") or int(getattr(model, "state_dim", obs_dim)) != obs_dim:
        raise ValueError("RMSMENS compares the model state with the observation: %s's state is not the "
                         "observation" % type(model).__name__)


# ---- host fallback: the reference's algorithm over pred_batch -----------------------------------------
def host_rmse(model, trajs, horizon=1):
    """model_metrics.py:12-43 over ``model.pred_batch`` (trajectories of at most `horizon` rows skipped)."""
    obs_dim = _obs_dim(trajs, model)
    sqerrss = []
    for traj in trajs:
        if len(traj) <= horizon:
            continue
        if hasattr(model, "traj_to_states"):
            state = model.traj_to_states(traj[:-horizon])
        else:
            state = traj.obs[:-horizon, :]
        for k in range(horizon):
            state = model.pred_batch(state, traj.ctrls[k:-(horizon - k), :])
        if hasattr(model, "traj_to_states"):
            state = state[:, :obs_dim]
        actual = traj.obs[horizon:]
        sqerrss.append((state - actual) ** 2)
    if not sqerrss:
        return float("nan")
    sqerrs = np.concatenate(sqerrss)
    return float(np.sqrt(np.mean(sqerrs, axis=None) * obs_dim))


def host_rmsmens(model, trajs, horiz=1):
    """model_metrics.py:45-111 over ``model.pred_batch``."""
    _check_rmsmens_model(model, _obs_dim(trajs, model))
    dy_means, dy_std = _increment_stats(trajs)
    sqerrss = []
    for traj in trajs:
        if len(traj) <= horiz:
            continue
        state = traj.obs[:-horiz, :]
        for k in range(horiz):
            pstate = state
            state = model.pred_batch(state, traj.ctrls[k:-(horiz - k), :])
        pred_deltas = state - pstate
        act_deltas = traj.obs[horiz:] - traj.obs[horiz - 1:-1]
        sqerrs = (normalize(dy_means, dy_std, pred_deltas) - normalize(dy_means, dy_std, act_deltas)) ** 2
        sqerrss.append(sqerrs)
    if not sqerrss:
        return float("nan")
    return float(np.sqrt(np.mean(np.concatenate(sqerrss), axis=None)))


# ---- device path ---------------------------------------------------------------------------------------
def device_shape_key(model):
    """Key of the models that share one ``ampc_kstep_errors`` call, or None when the model is scored on the
    host (SINDy, linear models wider than 64 states, untrained linear models, foreign models)."""
    from ..sysid.linear import _LinearModel
    from ..sysid.mlp import MLP
    s = model.system
    if type(model).pred_batch is not MLP.pred_batch and type(model).pred_batch is not _LinearModel.pred_batch:
        return None
    if isinstance(model, MLP):
        return ("mlp", model.precision, int(model.device), s.obs_dim, s.ctrl_dim, tuple(model.hidden_sizes),
                model.nonlintype)
    if isinstance(model, _LinearModel):
        if getattr(model, "A", None) is None or model.state_dim > _DEVICE_MAX_LINEAR_STATES:
            return None
        return ("linear", model.precision, int(model.device), model.state_dim, s.ctrl_dim)
    return None


# ---- wide linear models: state rules and the one-launch entry ------------------------------------------
def linear_state_rule(model, obs_dim=None):
    """How ``ampc_kstep_errors_linear`` forms the model's initial states, as plain values:
    ``{"rule": 1, "history": k}`` (ARX: the lag gather), ``{"rule": 2, "kinds": int32[], "params": float64[]}``
    (Koopman without product terms: the lift) or ``{"rule": 0}`` (rows from ``traj_to_states``, or the observation
    itself for a model without it).  Rules 1 and 2 are given only when the class's own ``traj_to_states`` is in
    use and the rule's state size is the width of the trained ``A``."""
    from ..sysid.linear import ARX, Koopman
    cls = type(model)
    no = model.system.obs_dim if obs_dim is None else int(obs_dim)
    nu = model.system.ctrl_dim
    width = None if getattr(model, "A", None) is None else int(np.shape(model.A)[0])
    if (isinstance(model, ARX) and cls.traj_to_states is ARX.traj_to_states
            and cls._get_all_feature_vectors is ARX._get_all_feature_vectors
            and width in (None, 1 + model.k * (no + nu) - nu)):
        return {"rule": 1, "history": int(model.k)}
    if (isinstance(model, Koopman) and cls.traj_to_states is Koopman.traj_to_states
            and cls._transform_observations is Koopman._transform_observations
            and cls._apply_basis is Koopman._apply_basis):
        lift = model.device_lift()
        if lift is not None and width in (None, len(lift[0]) * no):
            return {"rule": 2, "kinds": np.asarray(lift[0], dtype=np.int32),
                    "params": np.asarray(lift[1], dtype=np.float64)}
    return {"rule": 0}


def rule_states(rule, obs, ctrls):
    """The states of ONE trajectory (obs [T][obs_dim], ctrls [T][ctrl_dim]) by a ``linear_state_rule`` of kind 1
    or 2, evaluated in numpy the way the device evaluates it: column by column, row ``max(t - lag, 0)``."""
    obs, ctrls = np.asarray(obs, dtype=np.float64), np.asarray(ctrls, dtype=np.float64)
    T = obs.shape[0]
    if rule["rule"] == 1:
        cols = [obs]
        for lag in range(1, int(rule["history"])):
            idx = np.maximum(np.arange(T) - lag, 0)
            cols += [obs[idx], ctrls[idx]]
        cols.append(np.ones((T, 1)))
        return np.concatenate(cols, axis=1)
    if rule["rule"] == 2:
        parts = []
        for kind, p in zip(rule["kinds"], rule["params"]):
            parts.append(obs if kind == 0 else obs ** int(p) if kind == 1
                         else np.sin(p * obs) if kind == 2 else np.cos(p * obs))
        return np.concatenate(parts, axis=1)
    raise ValueError("rule 0 has no formula: its rows are the model's traj_to_states")


def _wide_lds_bytes(obs_dim, delta, width, ctrl_dim, esz):
    """kstep_lin_lds_bytes (csrc/kstep_linear_kernels.hpp)."""
    kp = (width + ctrl_dim + 3) // 4 * 4
    xs = (kp | 1) if esz == 8 else ((kp + 2) | 2)
    return (4 if delta else 2) * 16 * obs_dim * 8 + 128 + 2 * 16 * xs * esz


def wide_linear_key(model, obs_dim=None, delta=False):
    """Key of the wide linear models that share one ``ampc_kstep_errors_linear`` call -- (precision, device,
    ctrl_dim): state dimensions may differ -- or None: not a trained ``_LinearModel`` of 65..256 states and at most
    16 controls with the class's own ``pred_batch`` (or, with the delta sums of an observation of more than ~200
    entries, error blocks that do not fit LDS)."""
    from ..sysid.linear import _LinearModel
    if not isinstance(model, _LinearModel) or type(model).pred_batch is not _LinearModel.pred_batch:
        return None
    if getattr(model, "A", None) is None:
        return None
    s = model.system
    no = s.obs_dim if obs_dim is None else int(obs_dim)
    width = int(np.shape(model.A)[0])
    if not (_DEVICE_MAX_LINEAR_STATES < width <= _WIDE_MAX_LINEAR_STATES) or not (1 <= s.ctrl_dim <= _WIDE_MAX_CTRLS):
        return None
    if np.shape(model.A) != (width, width) or np.shape(model.B) != (width, s.ctrl_dim) or no > width:
        return None
    if not hasattr(model, "traj_to_states") and width != no:
        return None
    if _wide_lds_bytes(no, delta, width, s.ctrl_dim, 8 if model.precision == "f64" else 4) > _LDS_BYTES:
        return None
    return ("wide-linear", model.precision, int(model.device), s.ctrl_dim)


def kstep_sums_linear(models, trajs, kmax, delta=False):
    """(S [n_models][kmax], D or None) of wide linear models of ONE ``wide_linear_key``: one
    ``ampc_kstep_errors_linear`` call."""
    import ctypes
    obs_dim = _obs_dim(trajs, models[0])
    lens, obs, ctrls = _concat(trajs)
    n = len(models)
    handles = [m._dev() for m in models]
    hp = (ctypes.c_void_p * n)(*[h._h.value for h in handles])
    rules = np.zeros(n, dtype=np.int32)
    history = np.zeros(n, dtype=np.int32)
    n_basis = np.zeros(n, dtype=np.int32)
    kinds, params, keep = [], [], []
    rows = (ctypes.c_void_p * n)()
    for i, m in enumerate(models):
        r = linear_state_rule(m, obs_dim)
        rules[i] = r["rule"]
        if r["rule"] == 1:
            history[i] = r["history"]
        elif r["rule"] == 2:
            n_basis[i] = len(r["kinds"])
            kinds.append(r["kinds"])
            params.append(r["params"])
        elif hasattr(m, "traj_to_states"):
            a = np.ascontiguousarray(np.concatenate([m.traj_to_states(t) for t in trajs]), dtype=np.float64)
            keep.append(a)
            rows[i] = a.ctypes.data
    kinds = np.ascontiguousarray(np.concatenate(kinds), dtype=np.int32) if kinds else None
    params = np.ascontiguousarray(np.concatenate(params), dtype=np.float64) if params else None
    inv_std = None
    if delta:
        _, std = _increment_stats(trajs)
        with np.errstate(divide="ignore"):
            inv_std = np.ascontiguousarray(1.0 / std)
    S = np.empty((n, kmax))
    D = np.empty((n, kmax)) if delta else None
    lib = handles[0].lib
    _lib.check(lib.ampc_kstep_errors_linear(hp, n, len(trajs), _lib.iptr(lens), obs_dim, _lib.dptr(obs),
                                            _lib.dptr(ctrls), _lib.iptr(rules), _lib.iptr(history),
                                            _lib.iptr(n_basis), _lib.iptr(kinds), _lib.dptr(params), rows, int(kmax),
                                            _lib.dptr(inv_std), _lib.dptr(S), _lib.dptr(D)))
    return S, D


# ---- SINDy models: the one-launch entry ------------------------------------------------------------------
def sindy_program_sizes(model):
    """(n_feat, n_trig, n_pow, n_mon, n_pool, n_tab) of the feature program ``ampc_set_sindy`` builds from the
    model's library: the distinct sin / cos arguments and powers, one table entry per monomial and a constant 1;
    ``n_tab == 0`` (and no table arrays) when the table would exceed ``kSindyMaxTab``: direct evaluation."""
    kind, a0, a1, par, pair_var, _ = model.library
    trig, pows, n_mon = set(), set(), 0
    for k, a, b, p in zip(kind.tolist(), a0.tolist(), a1.tolist(), par.tolist()):
        if 1 <= k <= 4:
            trig.add((a if k <= 2 else b, p))
        elif k == 5:
            pows.add((a, p))
        elif k == 6:
            n_mon += 1
    n_tab = 2 * len(trig) + len(pows) + n_mon + 1
    if n_tab > _SINDY_MAX_TAB:
        return len(kind), 0, 0, 0, len(pair_var), 0
    return len(kind), len(trig), len(pows), n_mon, len(pair_var), n_tab


def _sindy_lds_bytes(model, nx, nu, delta):
    """kstep_sindy_lds_bytes (csrc/kstep_sindy_kernels.hpp) with sindy_stage_bytes (csrc/host_common.hpp)."""
    esz = 8 if model.precision == "f64" else 4
    n_feat, n_trig, n_pow, n_mon, n_pool, n_tab = sindy_program_sizes(model)
    stage = 0
    if n_tab > 0:
        ints = 2 * n_feat + n_trig + n_pow + 2 * n_mon + 2 * n_pool
        elems = n_feat * nx + n_trig + n_pow + (ints * 4 + esz - 1) // esz + 2
        stage = elems * esz + 2 * esz if elems * esz <= _SINDY_STAGE_BYTES else 0
    err = (2 if delta else 1) * _SINDY_CHUNK * _SINDY_ERR_STRIDE * 8
    return (2 * nx + nu + n_tab) * _SINDY_ROWS * esz + err + stage


def sindy_kstep_key(model, obs_dim=None, delta=False):
    """Key of the SINDy models that share one ``ampc_kstep_errors_sindy`` call -- ("sindy", precision, device,
    obs_dim, ctrl_dim): libraries, coefficients and time modes may differ -- or None: not a ``SINDy`` with the
    class's own ``pred_batch`` and device staging, a system the entry does not take (``obs_dim`` is not the model's,
    more than 64 states or 16 controls, a coefficient matrix of another shape), or per-thread columns that do not
    fit LDS.  Needs no GPU."""
    from ..sysid.sindy import SINDy
    cls = type(model)
    if not isinstance(model, SINDy) or cls.pred_batch is not SINDy.pred_batch:
        return None
    if cls._dev is not SINDy._dev or cls.stage_into is not SINDy.stage_into:
        return None
    s = model.system
    no = s.obs_dim if obs_dim is None else int(obs_dim)
    if no != s.obs_dim or not (1 <= no <= 64) or not (1 <= s.ctrl_dim <= _WIDE_MAX_CTRLS):
        return None
    n_feat = len(model.library[0])
    if not (1 <= n_feat <= 4096) or np.shape(model.coefficients) != (no, n_feat):
        return None
    if model.precision not in ("f64", "f32"):
        return None
    if _sindy_lds_bytes(model, no, s.ctrl_dim, delta) > _LDS_BYTES:
        return None
    return ("sindy", model.precision, int(model.device), no, s.ctrl_dim)


def kstep_sums_sindy(models, trajs, kmax, delta=False):
    """(S [n_models][kmax], D or None) of SINDy models of ONE ``sindy_kstep_key``: one ``ampc_kstep_errors_sindy``
    call."""
    import ctypes
    obs_dim = _obs_dim(trajs, models[0])
    lens, obs, ctrls = _concat(trajs)
    n = len(models)
    handles = [m._dev() for m in models]
    hp = (ctypes.c_void_p * n)(*[h._h.value for h in handles])
    inv_std = None
    if delta:
        _, std = _increment_stats(trajs)
        with np.errstate(divide="ignore"):
            inv_std = np.ascontiguousarray(1.0 / std)
    S = np.empty((n, kmax))
    D = np.empty((n, kmax)) if delta else None
    lib = handles[0].lib
    _lib.check(lib.ampc_kstep_errors_sindy(hp, n, len(trajs), _lib.iptr(lens), obs_dim, _lib.dptr(obs),
                                           _lib.dptr(ctrls), int(kmax), _lib.dptr(inv_std), _lib.dptr(S),
                                           _lib.dptr(D)))
    return S, D


# ---- MLP models of any mix of shapes: the one-launch entry ------------------------------------------------
def mlp_batch_key(model, obs_dim=None):
    """Key of the MLP models that share one ``ampc_kstep_errors_mlp`` call -- ("mlp-batch", device, obs_dim, ctrl_dim):
    depth, widths and activation may differ -- or None: not an f64 ``MLP`` with the class's own ``pred_batch``, a
    system the entry does not take (``obs_dim`` is not the model's, more than 64 states, 16 controls or 80 inputs), or
    a network over its limits (1..4 hidden layers of 1..256 units).  Needs no GPU."""
    from ..sysid.mlp import MLP
    if not isinstance(model, MLP) or type(model).pred_batch is not MLP.pred_batch:
        return None
    if model.precision != "f64" or model.nonlintype not in _lib.ACTIVATIONS:
        return None
    s = model.system
    no = s.obs_dim if obs_dim is None else int(obs_dim)
    if no != s.obs_dim or not (1 <= no <= _MLP_BATCH_MAX_STATES) or not (1 <= s.ctrl_dim <= _WIDE_MAX_CTRLS):
        return None
    if no + s.ctrl_dim > _MLP_BATCH_MAX_IN:
        return None
    hidden = [int(h) for h in model.hidden_sizes]
    if not (1 <= len(hidden) <= _MLP_BATCH_MAX_HIDDEN) or any(not (1 <= h <= _MLP_BATCH_MAX_WIDTH) for h in hidden):
        return None
    return ("mlp-batch", int(model.device), no, s.ctrl_dim)


def _device_resident(model):
    """The fit's device tensors of `model` when they stand for it on its own GPU (float64, contiguous, the fit's
    normalisers still in place), else None."""
    dp = getattr(model, "_dev_params", None)
    if dp is None:
        return None
    tensors = list(dp["w"]) + list(dp["b"]) + list(dp["norm_dev"])
    for t in tensors:
        if not (t.is_cuda and t.device.index == int(model.device) and t.is_contiguous()
                and str(t.dtype) == "torch.float64"):
            return None
    return dp if model._normalisers_are_the_fit() else None


def mlp_batch_args(models):
    """What ``ampc_kstep_errors_mlp`` takes for `models`, as plain arrays (no GPU, no library call): ``n_hidden`` [n],
    ``dims`` [n][6] (nx + nu, hidden widths, nx, zero padded), ``acts`` [n], ``weights`` / ``biases`` [n][5] and
    ``norms`` [n][4] (addresses as uint64, 0 past a model's layers), ``on_device`` [n] and ``keep``: the objects the
    addresses point into.  A model whose ``_dev_params`` holds the fit's device tensors hands over their
    ``data_ptr()``s (``on_device`` 1), the others contiguous float64 numpy copies of ``weights`` / ``biases`` and of the
    normalisers."""
    n, L = len(models), _MLP_BATCH_LAYERS
    n_hidden = np.zeros(n, dtype=np.int32)
    dims = np.zeros((n, L + 1), dtype=np.int32)
    acts = np.zeros(n, dtype=np.int32)
    weights = np.zeros((n, L), dtype=np.uint64)
    biases = np.zeros((n, L), dtype=np.uint64)
    norms = np.zeros((n, 4), dtype=np.uint64)
    on_device = np.zeros(n, dtype=np.int32)
    keep = []
    for k, m in enumerate(models):
        s = m.system
        hidden = [int(h) for h in m.hidden_sizes]
        if not 1 <= len(hidden) <= _MLP_BATCH_MAX_HIDDEN:
            raise ValueError("ampc_kstep_errors_mlp takes models of 1..%d hidden layers, not %d"
                             % (_MLP_BATCH_MAX_HIDDEN, len(hidden)))
        if m.precision != "f64":
            raise ValueError("ampc_kstep_errors_mlp takes f64 models only")
        d = [s.obs_dim + s.ctrl_dim] + hidden + [s.obs_dim]
        n_hidden[k] = len(hidden)
        dims[k, :len(d)] = d
        acts[k] = _lib.ACTIVATIONS[m.nonlintype]
        dp = _device_resident(m)
        if dp is not None:
            on_device[k] = 1
            ws, bs, nm = dp["w"], dp["b"], dp["norm_dev"]
            ptr = lambda t: t.data_ptr()
        else:
            ws, bs = [_lib.as_f64(w) for w in m.weights], [_lib.as_f64(b) for b in m.biases]
            nm = [_lib.as_f64(v) for v in (m.xu_means, m.xu_std, m.dy_means, m.dy_std)]
            ptr = lambda a: a.ctypes.data
        if len(ws) != len(d) - 1 or len(bs) != len(d) - 1:
            raise ValueError("one weight and one bias per layer (hidden + output) expected")
        for l, (w, b) in enumerate(zip(ws, bs)):
            if tuple(w.shape) != (d[l + 1], d[l]) or tuple(b.shape) != (d[l + 1],):
                raise ValueError("layer %d has shape %r, expected %r" % (l, tuple(w.shape), (d[l + 1], d[l])))
            weights[k, l], biases[k, l] = ptr(w), ptr(b)
        for i, v in enumerate(nm):
            if tuple(v.shape) != ((d[0],) if i < 2 else (d[-1],)):
                raise ValueError("normaliser shapes do not match (nx+nu, nx+nu, nx, nx)")
            norms[k, i] = ptr(v)
        keep.append((ws, bs, nm))
    return {"n_hidden": n_hidden, "dims": dims, "acts": acts, "weights": weights, "biases": biases, "norms": norms,
            "on_device": on_device, "keep": keep}


def kstep_sums_mlp(models, trajs, kmax, delta=False):
    """(S [n_models][kmax], D or None) of MLP models of ONE ``mlp_batch_key``: one ``ampc_kstep_errors_mlp`` call.  No
    model is staged into a handle."""
    import ctypes
    lib = _lib.load()
    obs_dim = _obs_dim(trajs, models[0])
    s = models[0].system
    lens, obs, ctrls = _concat(trajs)
    n = len(models)
    args = mlp_batch_args(models)
    device = int(models[0].device)
    if any(int(m.device) != device for m in models):
        raise ValueError("the models of one ampc_kstep_errors_mlp call live on one device")
    if args["on_device"].any():
        import torch
        torch.cuda.current_stream(torch.device("cuda", device)).synchronize()    # the fit's kernels have finished
    inv_std = None
    if delta:
        _, std = _increment_stats(trajs)
        with np.errstate(divide="ignore"):
            inv_std = np.ascontiguousarray(1.0 / std)
    S = np.empty((n, kmax))
    D = np.empty((n, kmax)) if delta else None
    vpp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_void_p))
    _lib.check(lib.ampc_kstep_errors_mlp(device, n, _lib.iptr(args["n_hidden"]), _lib.iptr(args["dims"]),
                                         _lib.iptr(args["acts"]), vpp(args["weights"]), vpp(args["biases"]),
                                         vpp(args["norms"]), _lib.iptr(args["on_device"]), s.obs_dim, s.ctrl_dim,
                                         len(trajs), _lib.iptr(lens), obs_dim, _lib.dptr(obs), _lib.dptr(ctrls),
                                         int(kmax), _lib.dptr(inv_std), _lib.dptr(S), _lib.dptr(D)))
    del args
    return S, D


def _concat(trajs):
    lens = np.array([len(t) for t in trajs], dtype=np.int32)
    obs = np.ascontiguousarray(np.concatenate([np.asarray(t.obs, dtype=np.float64) for t in trajs]))
    ctrls = np.ascontiguousarray(np.concatenate([np.asarray(t.ctrls, dtype=np.float64) for t in trajs]))
    return lens, obs, ctrls


def kstep_sums(models, trajs, kmax, delta=False):
    """(S [n_models][kmax], D [n_models][kmax] or None): the sums ``ampc_kstep_errors`` returns, for models
    of ONE device shape (device_shape_key)."""
    import ctypes
    obs_dim = _obs_dim(trajs, models[0])
    lens, obs, ctrls = _concat(trajs)
    n = len(models)
    handles = [m._dev() for m in models]
    hp = (ctypes.c_void_p * n)(*[h._h.value for h in handles])
    init = None
    if hasattr(models[0], "traj_to_states"):
        init = np.ascontiguousarray(np.stack([np.concatenate([m.traj_to_states(t) for t in trajs]) for m in models]),
                                    dtype=np.float64)
    inv_std = None
    if delta:
        _, std = _increment_stats(trajs)
        with np.errstate(divide="ignore"):
            inv_std = np.ascontiguousarray(1.0 / std)
    S = np.empty((n, kmax))
    D = np.empty((n, kmax)) if delta else None
    lib = handles[0].lib
    _lib.check(lib.ampc_kstep_errors(hp, n, len(trajs), _lib.iptr(lens), obs_dim, _lib.dptr(obs), _lib.dptr(ctrls),
                                     _lib.dptr(init), int(kmax), _lib.dptr(inv_std), _lib.dptr(S), _lib.dptr(D)))
    return S, D


def row_counts(trajs, kmax):
    """N_h for h = 1..kmax: start points with t + h <= L_i - 1."""
    lens = np.array([len(t) for t in trajs], dtype=np.int64)
    return np.array([np.maximum(lens - h, 0).sum() for h in range(1, kmax + 1)], dtype=np.float64)


def model_errors(models, trajs, horizons, metric="rmse", linear_kstep="host", report=None, sindy_kstep="host",
                 mlp_kstep="shape"):
    """RMSE or RMSMENS of every model at every horizon: ndarray [len(models), len(horizons)] in input order
    (the data of a ``KstepPredAccGraph`` curve).  Device models are grouped by shape, one ``ampc_kstep_errors``
    call per group covering every horizon; the others take the host fallback (module docstring) -- except, with
    ``linear_kstep="device"``, the wide linear models: one ``ampc_kstep_errors_linear`` call per
    ``wide_linear_key``, and, with ``sindy_kstep="device"``, the SINDy models: one ``ampc_kstep_errors_sindy`` call
    per ``sindy_kstep_key``, and, with ``mlp_kstep="batch"``, the f64 MLPs of any mix of shapes: one
    ``ampc_kstep_errors_mlp`` call per ``mlp_batch_key`` instead of one ``ampc_kstep_errors`` launch per model (MLPs that
    key refuses keep the per-shape path).  ``report``: a ``KstepReport`` to fill (one is made otherwise; either way it becomes
    ``model_metrics.last_report``)."""
    global last_report
    if metric not in METRICS:
        raise ValueError("metric must be one of %s, not %r" % (", ".join(METRICS), metric))
    if linear_kstep not in LINEAR_KSTEP:
        raise ValueError("linear_kstep must be 'host' or 'device'")
    if sindy_kstep not in SINDY_KSTEP:
        raise ValueError("sindy_kstep must be 'host' or 'device'")
    if mlp_kstep not in MLP_KSTEP:
        raise ValueError("mlp_kstep must be 'shape' or 'batch'")
    report = KstepReport() if report is None else report
    last_report = report
    models = list(models)
    horizons = [int(h) for h in np.atleast_1d(horizons)]
    if not horizons or min(horizons) < 1:
        raise ValueError("horizons must be >= 1")
    trajs = list(trajs)
    obs_dim = _obs_dim(trajs, models[0]) if models else 0
    out = np.full((len(models), len(horizons)), np.nan)
    if metric == "rmsmens":
        for m in models:
            _check_rmsmens_model(m, obs_dim)
    delta = metric == "rmsmens"
    groups, wide, sindy, batch = {}, {}, {}, {}
    for i, m in enumerate(models):
        key = mlp_batch_key(m, obs_dim) if mlp_kstep == "batch" and trajs else None
        if key is not None:
            batch.setdefault(key, []).append(i)
            continue
        key = device_shape_key(m) if trajs else None
        if key is not None:
            groups.setdefault(key, []).append(i)
            continue
        if linear_kstep == "device" and trajs:
            key = wide_linear_key(m, obs_dim, delta)
        if key is not None:
            wide.setdefault(key, []).append(i)
            continue
        if sindy_kstep == "device" and trajs:
            key = sindy_kstep_key(m, obs_dim, delta)
        if key is not None:
            sindy.setdefault(key, []).append(i)
        else:
            host = host_rmse if metric == "rmse" else host_rmsmens
            out[i] = [host(m, trajs, h) for h in horizons]
            report.host_fallbacks += 1
    if groups or wide or sindy or batch:
        kmax = max(horizons)
        N = row_counts(trajs, kmax)
        hidx = np.array(horizons) - 1
        for sums, grp in ((kstep_sums, groups), (kstep_sums_linear, wide), (kstep_sums_sindy, sindy),
                          (kstep_sums_mlp, batch)):
            for idx in grp.values():
                S, D = sums([models[i] for i in idx], trajs, kmax, delta=delta)
                with np.errstate(divide="ignore", invalid="ignore"):
                    val = np.sqrt(S / N) if metric == "rmse" else np.sqrt(D / (N * obs_dim))
                out[idx] = val[:, hidx]
                if grp is wide:
                    report.wide_models += len(idx)
                    report.wide_calls += 1
                elif grp is sindy:
                    report.sindy_models += len(idx)
                    report.sindy_calls += 1
                elif grp is batch:
                    report.mlp_batch_models += len(idx)
                    report.mlp_batch_calls += 1
                else:
                    report.device_models += len(idx)
    return out


def get_model_rmse(model, trajs, horizon=1, linear_kstep="host", sindy_kstep="host", mlp_kstep="shape"):
    """Unnormalised RMSE at a fixed horizon (model_metrics.py:12-43); see the module docstring."""
    return float(model_errors([model], trajs, [horizon], "rmse", linear_kstep=linear_kstep,
                              sindy_kstep=sindy_kstep, mlp_kstep=mlp_kstep)[0, 0])


def get_model_rmsmens(model, trajs, horiz=1, linear_kstep="host", sindy_kstep="host", mlp_kstep="shape"):
    """Root mean squared model error, normalised step-wise (model_metrics.py:45-111); see the module
    docstring for the deviations from the reference."""
    return float(model_errors([model], trajs, [horiz], "rmsmens", linear_kstep=linear_kstep,
                              sindy_kstep=sindy_kstep, mlp_kstep=mlp_kstep)[0, 0])
