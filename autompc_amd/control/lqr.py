"""LQR, finite and infinite horizon, whose gain is computed on MI355X.

Drop-in for the reference's ``autompc.control.LQR`` / ``LQRFactory`` / ``FiniteHorizonLQR`` /
``InfiniteHorizonLQR`` (reference: autompc/control/lqr.py:139-253): same constructors, ``state_dim``,
``traj_to_state``, ``run`` and ``is_compatible``.

The gain K = -(R + B'PB)^-1 B'PA after horizon + 1 Riccati steps from P = F (``_finite_horz_dt_lqr``,
lqr.py:35-47; Q and F zero-padded to the model state, :146-151) comes from a one-problem ``ampc_lqr_gains``
call (csrc/lqr_kernels.hpp).  A singular R + B'PB raises ``numpy.linalg.LinAlgError`` as the reference's
``la.inv`` does.  ``run`` is the reference's host arithmetic (lqr.py:174-192): a nu x n matrix-vector product
per step is cheaper on the host than a device round trip.

Infinite horizon.  The reference's ``InfiniteHorizonLQR.__init__`` calls ``dare``, which it never defines
(lqr.py:104), so by default (``infinite_horizon="refuse"``) the class raises ``NotImplementedError`` here.  With
``infinite_horizon="iterate"`` the gain is the one the reference ships for that class, ``_inf_horz_dt_lqr(A, B, Qp, R,
0, threshold)`` (lqr.py:22-33): the Riccati step from P = Q (padded, :102-103; F is not used) until max|dP| <=
threshold, on the device (``ampc_lqr_gains_ex``), and ``run`` is the reference's (:126-136): u = K modelstate, no goal
offset and no clipping even on a bounded task.

Deviations, on purpose: the reference prints P after every gain (lqr.py:44-45) and the state in every infinite-horizon
``run`` (:131-133) -- not reproduced; the reference's fixed-point loop has no cap and never returns when P keeps
moving (an ARX model with a noticeable bias column: its constant state adds a constant to P every step) -- here it
stops after ``max_iter`` steps (default 10000) and raises ``RiccatiNotConverged``, a ``LinAlgError``, so a tuner scores
the configuration ``inf``; a nonlinear model raises ``TypeError`` (what ``is_compatible`` implies); a horizon outside
LQRFactory's range 1..1000 raises ``ValueError`` (the device refuses longer recursions).
"""
import numpy as np

from .. import _lib
from .controller import Controller, ControllerFactory


# LQRFactory's space (lqr.py:214-224): finite_horizon {"true", "false"} (default "true"); horizon 1..1000
# (default 10), active when finite_horizon == "true"
FINITE_HORIZON_CHOICES = ("true", "false")
HORIZON_RANGE = (1, 1000)
HORIZON_DEFAULT = 10
# what a controller does with finite_horizon false: "refuse" (NotImplementedError, the default) or "iterate"
INFINITE_HORIZON_CHOICES = ("refuse", "iterate")
INF_THRESHOLD_DEFAULT = 1e-3          # _inf_horz_dt_lqr's default (lqr.py:22)
INF_MAX_ITER_DEFAULT = 10000          # ours: the reference has no cap
INF_MAX_ITER_LIMIT = 100000           # ampc_lqr_gains_ex's bound


class RiccatiNotConverged(np.linalg.LinAlgError):
    """The infinite-horizon Riccati iteration still moved P by more than its threshold after max_iter steps."""


def _is_linear(model):
    return bool(getattr(model, "is_linear", False))


def _compatible(task, model):
    # (a task type without constraint support has none)
    eq = getattr(task, "eq_cons_present", lambda: False)()
    ineq = getattr(task, "ineq_cons_present", lambda: False)()
    return _is_linear(model) and task.is_cost_quad() and not task.are_obs_bounded() and not eq and not ineq


def check_horizon(horizon):
    if not HORIZON_RANGE[0] <= int(horizon) <= HORIZON_RANGE[1]:
        raise ValueError("LQR horizon %r is outside LQRFactory's range %d..%d (lqr.py:214-224)"
                         % (horizon, HORIZON_RANGE[0], HORIZON_RANGE[1]))


def check_infinite_horizon(value):
    if value not in INFINITE_HORIZON_CHOICES:
        raise ValueError("infinite_horizon must be one of %r, not %r" % (INFINITE_HORIZON_CHOICES, value))
    return value


def check_inf_params(threshold, max_iter):
    if not (np.isfinite(threshold) and threshold > 0):
        raise ValueError("infinite-horizon LQR threshold must be finite and > 0, not %r" % (threshold,))
    if not 1 <= int(max_iter) <= INF_MAX_ITER_LIMIT:
        raise ValueError("infinite-horizon LQR max_iter must be in 1..%d, not %r" % (INF_MAX_ITER_LIMIT, max_iter))


def check_linear(model):
    if not _is_linear(model):
        raise TypeError("LQR needs a linear model (ARX, Koopman: to_linear()); %s is not one "
                        "(the reference's is_compatible, lqr.py:161-168)" % type(model).__name__)


def lqr_gain_host(A, B, Q, R, F, horizon):
    """K of _finite_horz_dt_lqr(A, B, Q, R, 0, F, horizon) on the host, in the reference's own order of operations
    (lqr.py:15-20, 35-47; Q and F zero-padded to the model state, :146-151).  For models the device cannot take
    (more than 256 states).  Raises LinAlgError where the reference's ``la.inv`` does."""
    check_horizon(horizon)
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    n = A.shape[0]
    Q, F = np.asarray(Q, dtype=np.float64), np.asarray(F, dtype=np.float64)
    Qp, Fp = np.zeros((n, n)), np.zeros((n, n))
    Qp[:Q.shape[0], :Q.shape[1]] = Q
    Fp[:F.shape[0], :F.shape[1]] = F
    R = np.asarray(R, dtype=np.float64)
    N = np.zeros((n, B.shape[1]))

    def riccati(Pk):
        return A.T @ Pk @ A - (A.T @ Pk @ B + N) @ np.linalg.inv(R + B.T @ Pk @ B) @ (B.T @ Pk @ A + N.T) + Qp
    P2 = riccati(Fp)
    for _ in range(int(horizon)):
        P2 = riccati(P2)
    return -np.linalg.inv(R + B.T @ P2 @ B) @ B.T @ P2 @ A


def lqr_gain(A, B, Q, R, F, horizon, device=0):
    """K of _finite_horz_dt_lqr(A, B, Q, R, 0, F, horizon) (lqr.py:35-47) on the device; Q, F of obs_dim
    (padded there).  Raises LinAlgError where the reference's inversion fails."""
    check_horizon(horizon)
    A, B = _lib.as_f64(A), _lib.as_f64(B)
    Q, R, F = _lib.as_f64(Q), _lib.as_f64(R), _lib.as_f64(F)
    h = _lib.Handle(device, "f64", jit=False)
    try:
        h.set_linear(A, B)
        plan = _lib.LqrPlan([h], Q.shape[0], B.shape[1], device=device)
        try:
            K, status = plan.gains([int(horizon)], Q[None], R[None], F[None])
        finally:
            plan.close()
    finally:
        h.close()
    if status[0] != 0:
        raise np.linalg.LinAlgError("LQR: R + B'PB is singular (or the Riccati recursion overflowed)")
    return K[0]


def lqr_gain_inf_host(A, B, Q, R, threshold=INF_THRESHOLD_DEFAULT, max_iter=INF_MAX_ITER_DEFAULT):
    """(K, iters) of _inf_horz_dt_lqr(A, B, Qp, R, 0, threshold) on the host, in the reference's own order of
    operations (lqr.py:15-33; Q zero-padded to the model state, :102-103).  iters: Riccati steps performed, 1 plus the
    passes of the reference's ``while``.  The reference's loop has no cap; this one raises ``RiccatiNotConverged``
    when P still moves by more than `threshold` after `max_iter` steps (an ARX model with a bias column never
    converges).  The default of 10000 is a choice, not a measurement: that many steps of a 235-state model take of
    the order of ten seconds on the device and far longer here, so lower it when tuning ARX models.  Raises
    LinAlgError where the reference's ``la.inv`` does, or where P turns NaN (the reference returns a NaN gain)."""
    check_inf_params(threshold, max_iter)
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    n = A.shape[0]
    Q = np.asarray(Q, dtype=np.float64)
    Qp = np.zeros((n, n))
    Qp[:Q.shape[0], :Q.shape[1]] = Q
    R = np.asarray(R, dtype=np.float64)
    N = np.zeros((n, B.shape[1]))

    def riccati(Pk):
        return A.T @ Pk @ A - (A.T @ Pk @ B + N) @ np.linalg.inv(R + B.T @ Pk @ B) @ (B.T @ Pk @ A + N.T) + Qp
    P1 = Qp
    P2 = riccati(P1)
    iters = 1
    while True:
        d = np.abs(P1 - P2).max()
        if np.isnan(d):
            raise np.linalg.LinAlgError("LQR: the Riccati iteration produced a non-finite P")
        if not d > threshold:
            break
        if iters >= int(max_iter):
            raise RiccatiNotConverged("LQR: P still moves by %.3g > threshold %.3g after max_iter = %d Riccati steps"
                                      % (d, threshold, iters))
        P1 = P2
        P2 = riccati(P1)
        iters += 1
    K = -np.linalg.inv(R + B.T @ P2 @ B) @ B.T @ P2 @ A
    if not np.all(np.isfinite(K)):
        raise np.linalg.LinAlgError("LQR: non-finite gain")
    return K, iters


def lqr_gain_inf(A, B, Q, R, threshold=INF_THRESHOLD_DEFAULT, max_iter=INF_MAX_ITER_DEFAULT, device=0):
    """(K, iters) of _inf_horz_dt_lqr(A, B, Qp, R, 0, threshold) (lqr.py:22-33) on the device; Q of obs_dim (padded
    there).  Raises ``RiccatiNotConverged`` at `max_iter` steps (see ``lqr_gain_inf_host`` on the default) and
    LinAlgError where the reference's inversion fails or P turns non-finite."""
    check_inf_params(threshold, max_iter)
    A, B = _lib.as_f64(A), _lib.as_f64(B)
    Q, R = _lib.as_f64(Q), _lib.as_f64(R)
    h = _lib.Handle(device, "f64", jit=False)
    try:
        h.set_linear(A, B)
        plan = _lib.LqrPlan([h], Q.shape[0], B.shape[1], device=device)
        try:
            K, status, iters = plan.gains_ex([0], Q[None], R[None], Q[None], thresholds=float(threshold),
                                             max_iters=int(max_iter))
        finally:
            plan.close()
    finally:
        h.close()
    if status[0] == 2:
        raise RiccatiNotConverged("LQR: P still moves by more than threshold %.3g after max_iter = %d Riccati steps"
                                  % (threshold, int(max_iter)))
    if status[0] != 0:
        raise np.linalg.LinAlgError("LQR: R + B'PB is singular (or the Riccati iteration overflowed)")
    return K[0], int(iters[0])


class FiniteHorizonLQR(Controller):
    def __init__(self, system, task, model, horizon, device=None):
        super().__init__(system, task, model)
        check_linear(model)
        A, B = model.to_linear()
        self.horizon = horizon
        Q, R, F = task.get_cost().get_cost_matrices()
        self.device = device if device is not None else getattr(model, "device", 0)
        self.K = lqr_gain(A, B, Q, R, F, int(horizon), device=self.device)
        self.model = model
        self.umin = task.get_ctrl_bounds()[:, 0]
        self.umax = task.get_ctrl_bounds()[:, 1]

    @property
    def state_dim(self):
        return self.model.state_dim + self.system.ctrl_dim

    @staticmethod
    def is_compatible(system, task, model):
        return _compatible(task, model)

    def traj_to_state(self, traj):
        return np.concatenate([self.model.traj_to_state(traj), traj[-1].ctrl])

    def run(self, state, new_obs):
        nu = self.system.ctrl_dim
        modelstate = self.model.update_state(state[:-nu], state[-nu:], new_obs)
        x0 = np.asarray(self.task.get_cost().get_goal())
        if x0.size < modelstate.size:
            state0 = np.zeros(modelstate.size)
            state0[:x0.size] = x0
        else:
            state0 = x0
        u = self.K @ (modelstate - state0)
        u = np.minimum(u, self.umax)
        u = np.maximum(u, self.umin)
        return u, np.concatenate([modelstate, u])


class InfiniteHorizonLQR(Controller):
    """infinite_horizon="refuse" (default): raises NotImplementedError, as the reference's undefined ``dare`` makes
    its class unusable.  "iterate": K = _inf_horz_dt_lqr(A, B, Qp, R, 0, threshold) on the device, at most `max_iter`
    Riccati steps (``RiccatiNotConverged`` beyond; the default 10000 is a choice -- about ten seconds for a 235-state
    model -- so lower it when tuning ARX models, whose bias column can keep P moving for ever)."""

    def __init__(self, system, task, model, infinite_horizon="refuse", threshold=INF_THRESHOLD_DEFAULT,
                 max_iter=INF_MAX_ITER_DEFAULT, device=None):
        super().__init__(system, task, model)
        if check_infinite_horizon(infinite_horizon) == "refuse":
            raise NotImplementedError("infinite-horizon LQR: the reference calls dare(), which it never defines "
                                      "(autompc/control/lqr.py:104); use finite_horizon=True, or "
                                      "infinite_horizon='iterate' for the reference's _inf_horz_dt_lqr gain")
        check_linear(model)
        A, B = model.to_linear()
        Q, R, _ = task.get_cost().get_cost_matrices()
        self.threshold, self.max_iter = float(threshold), int(max_iter)
        self.device = device if device is not None else getattr(model, "device", 0)
        self.K, self.iters = self._gain(A, B, Q, R)
        self.model = model

    def _gain(self, A, B, Q, R):
        return lqr_gain_inf(A, B, Q, R, self.threshold, self.max_iter, device=self.device)

    @property
    def state_dim(self):
        return self.model.state_dim + self.system.ctrl_dim

    @staticmethod
    def is_compatible(system, task, model):
        return _compatible(task, model) and not task.are_ctrl_bounded()

    def traj_to_state(self, traj):
        return np.concatenate([self.model.traj_to_state(traj), traj[-1].ctrl])

    def run(self, state, new_obs):
        nu = self.system.ctrl_dim
        modelstate = self.model.update_state(state[:-nu], state[-nu:], new_obs)
        u = np.array(self.K @ modelstate).flatten()
        return u, np.concatenate([modelstate, u])


class LQR(Controller):
    """infinite_horizon / threshold / max_iter: what finite_horizon false does (``InfiniteHorizonLQR``); through the
    factory's keyword merge, ``LQRFactory(system, infinite_horizon="iterate")``."""

    def __init__(self, system, task, model, finite_horizon, horizon=None, device=None, infinite_horizon="refuse",
                 threshold=INF_THRESHOLD_DEFAULT, max_iter=INF_MAX_ITER_DEFAULT):
        super().__init__(system, task, model)
        check_infinite_horizon(infinite_horizon)
        if not isinstance(finite_horizon, bool):
            finite_horizon = finite_horizon == "true"
        if finite_horizon:
            self._controller = FiniteHorizonLQR(system, task, model, horizon, device=device)
        else:
            self._controller = InfiniteHorizonLQR(system, task, model, infinite_horizon=infinite_horizon,
                                                  threshold=threshold, max_iter=max_iter, device=device)

    @property
    def K(self):
        return self._controller.K

    @property
    def iters(self):
        """Riccati steps of an infinite-horizon gain (None for a finite horizon)."""
        return getattr(self._controller, "iters", None)

    @property
    def state_dim(self):
        return self._controller.state_dim

    @staticmethod
    def is_compatible(system, task, model):
        return _compatible(task, model)

    def traj_to_state(self, traj):
        return self._controller.traj_to_state(traj)

    def run(self, state, new_obs):
        return self._controller.run(state, new_obs)


class LQRFactory(ControllerFactory):
    """Hyper-parameters as lqr.py:214-224: finite_horizon {"true", "false"}, horizon int 1..1000 (default 10)
    conditioned on finite_horizon == "true"."""
    Controller = LQR
    name = "LQR"

    def get_configuration_space(self):
        try:
            import ConfigSpace as CS
            import ConfigSpace.conditions as CSC
            import ConfigSpace.hyperparameters as CSH
        except ImportError as e:
            raise ImportError("ConfigSpace is required for get_configuration_space()") from e
        cs = CS.ConfigurationSpace()
        finite = CSH.CategoricalHyperparameter("finite_horizon", choices=list(FINITE_HORIZON_CHOICES),
                                               default_value="true")
        horizon = CSH.UniformIntegerHyperparameter("horizon", lower=HORIZON_RANGE[0], upper=HORIZON_RANGE[1],
                                                   default_value=HORIZON_DEFAULT)
        cs.add_hyperparameters([horizon, finite])
        cs.add_condition(CSC.InCondition(child=horizon, parent=finite, values=["true"]))
        return cs
