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


def model_errors(models, trajs, horizons, metric="rmse"):
    """RMSE or RMSMENS of every model at every horizon: ndarray [len(models), len(horizons)] in input order
    (the data of a ``KstepPredAccGraph`` curve).  Device models are grouped by shape, one ``ampc_kstep_errors``
    call per group covering every horizon; the others take the host fallback (module docstring)."""
    if metric not in METRICS:
        raise ValueError("metric must be one of %s, not %r" % (", ".join(METRICS), metric))
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
    groups = {}
    for i, m in enumerate(models):
        key = device_shape_key(m) if trajs else None
        if key is None:
            host = host_rmse if metric == "rmse" else host_rmsmens
            out[i] = [host(m, trajs, h) for h in horizons]
        else:
            groups.setdefault(key, []).append(i)
    if groups:
        kmax = max(horizons)
        N = row_counts(trajs, kmax)
        hidx = np.array(horizons) - 1
        for idx in groups.values():
            S, D = kstep_sums([models[i] for i in idx], trajs, kmax, delta=(metric == "rmsmens"))
            with np.errstate(divide="ignore", invalid="ignore"):
                val = np.sqrt(S / N) if metric == "rmse" else np.sqrt(D / (N * obs_dim))
            out[idx] = val[:, hidx]
    return out


def get_model_rmse(model, trajs, horizon=1):
    """Unnormalised RMSE at a fixed horizon (model_metrics.py:12-43); see the module docstring."""
    return float(model_errors([model], trajs, [horizon], "rmse")[0, 0])


def get_model_rmsmens(model, trajs, horiz=1):
    """Root mean squared model error, normalised step-wise (model_metrics.py:45-111); see the module
    docstring for the deviations from the reference."""
    return float(model_errors([model], trajs, [horiz], "rmsmens")[0, 0])
