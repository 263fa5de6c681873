"""Batched closed-loop scores of LQR pipeline candidates: (ARX | Koopman) x LQR x QuadCost.

What it replaces.  ``PipelineTuner.eval_cfg`` (autompc/tuning/pipeline_tuner.py:213-258) builds the configuration's
model and its ``LQR`` controller (control/lqr.py:139-253), runs ``simulate(controller, init_obs, task.term_cond,
sim_model=surrogate, max_steps=task.get_num_steps())`` and scores the trajectory with ``task.get_cost()``; a
``LinAlgError`` scores ``inf``.  Here every finite-horizon candidate of a batch goes into ONE ``_lib.LqrPlan``:

1. one ``ampc_lqr_gains`` launch computes every gain (state sizes obs_dim..256 and horizons 1..1000 mixed);
2. ``ampc_lqr_plan_set_loop`` gives each candidate the controller update of its model: rule 1 the ARX shift,
   rule 2 the Koopman lift (``Koopman.device_lift()``), rule 0 a model whose state is the observation;
3. one scored closed loop (``ampc_lqr_closed_loop_scored``) runs every episode against the shared surrogate.

Nothing runs on the host per control step, and each distinct model is staged once per call.

Edge cases, on purpose:

* ``finite_horizon`` false scores ``inf`` by default (``infinite_horizon="refuse"``, status 2): the reference's
  ``InfiniteHorizonLQR`` calls ``dare``, which it never defines (lqr.py:104), so such a configuration can never become
  its incumbent.  With ``infinite_horizon="iterate"`` such a candidate gets the gain the reference ships for that class
  (``_inf_horz_dt_lqr``, lqr.py:22-33; ``control.lqr`` has the details) and rides in the same plan as the finite ones:
  horizon 0 in the one ``ampc_lqr_gains_ex`` launch, and in the one ``ampc_lqr_plan_set_loop_ex`` a zero goal and no
  clipping (``InfiniteHorizonLQR.run`` applies neither).  A candidate whose Riccati iteration has not converged after
  ``inf_max_iter`` steps scores ``inf`` with status 3, as ``eval_cfg`` scores a ``LinAlgError``.
* Gain status 1 (singular ``R + B'PB`` or a non-finite recursion) scores ``inf``, as ``eval_cfg``'s
  ``LinAlgError`` branch does.
* A nonlinear model raises ``TypeError`` and a horizon outside 1..1000 ``ValueError``, as the drop-in ``LQR`` does.
* A model the device cannot stage (more than 256 states, or a Koopman lift with product terms) is scored on the host:
  the reference's recursion (``control.lqr.lqr_gain_host``) and ``simulate()``.  ``host_fallbacks`` counts them.
* A user termination condition: nothing in the LQR loop is random and no candidate's rows depend on the rest of the
  batch, so the device runs the whole batch ``term_check_every`` steps, then twice as many, and so on (every run
  starts from the initial state again and repeats the earlier rows bit for bit) until every candidate has met the
  condition or the episode cap is reached.  Each trajectory is then cut at the first row where the host condition
  holds and scored on its own rows.
"""
import numpy as np

from .. import _lib
from ..control.lqr import (INF_MAX_ITER_DEFAULT, INF_THRESHOLD_DEFAULT, FiniteHorizonLQR, InfiniteHorizonLQR,
                           RiccatiNotConverged, check_horizon, check_inf_params, check_infinite_horizon,
                           check_linear, lqr_gain_host, lqr_gain_inf_host)
from ..costs.terms import cost_terms
from .batch_eval import (_as_matrix, _task_goal, default_episode_controls, episode_of, model_handle,
                         score_trajectories)

# what ampc_lqr_plan_create / _set_models take (csrc/api_lqr.cpp)
MAX_DEVICE_STATES = 256
MAX_DEVICE_CTRLS = 16


def is_finite_horizon(v):
    """LQRFactory's ``finite_horizon`` as a bool: "true" / "false" (the categorical's values) or a bool."""
    if isinstance(v, str):
        if v not in ("true", "false"):
            raise ValueError("finite_horizon must be 'true' or 'false', not %r" % v)
        return v == "true"
    return bool(v)


def device_rule(model, obs_dim):
    """(rule, lift) of ``ampc_lqr_plan_set_loop`` for a linear controller model, or None when the device cannot run
    its controller (state outside obs_dim..256, or an update_state it has no rule for)."""
    from ..sysid.linear import ARX
    n = int(model.state_dim)
    if n < obs_dim or n > MAX_DEVICE_STATES:
        return None
    if isinstance(model, ARX):
        return 1, None
    lift = model.device_lift() if hasattr(model, "device_lift") else None
    if lift is None:
        return None
    kinds, params = lift
    if len(kinds) == 1 and int(kinds[0]) == 0:     # the identity lift: the state is the observation
        return 0, None
    return 2, lift


class _HostFiniteHorizonLQR(FiniteHorizonLQR):
    """FiniteHorizonLQR whose gain comes from the host recursion (models the device does not take)."""

    def __init__(self, system, task, model, horizon):
        super(FiniteHorizonLQR, self).__init__(system, task, model)
        check_linear(model)
        A, B = model.to_linear()
        Q, R, F = task.get_cost().get_cost_matrices()
        self.horizon = horizon
        self.K = lqr_gain_host(A, B, Q, R, F, int(horizon))
        self.model = model
        self.umin = task.get_ctrl_bounds()[:, 0]
        self.umax = task.get_ctrl_bounds()[:, 1]


class _HostInfiniteHorizonLQR(InfiniteHorizonLQR):
    """InfiniteHorizonLQR ("iterate") whose gain comes from the host iteration (models the device does not take)."""

    def _gain(self, A, B, Q, R):
        return lqr_gain_inf_host(A, B, Q, R, self.threshold, self.max_iter)


class LqrCandidateEvaluator:
    """Closed-loop surrogate scores of LQR + QuadCost candidates on one GPU (see the module docstring).

    Candidates are dicts: ``controller="lqr"``, ``finite_horizon`` (bool or "true"/"false"), ``horizon`` (1..1000,
    read only when finite), ``Q``, ``R``, ``F`` (diagonals or full matrices about the task cost's goal) and optionally
    ``model`` (a trained ARX / Koopman; else the evaluator's own).  ``model_cfg`` rides along for the tuner."""

    accepts_global_ids = True

    def __init__(self, system, task, model=None, surrogate=None, device=0, term_check_every=64,
                 infinite_horizon="refuse", inf_threshold=INF_THRESHOLD_DEFAULT, inf_max_iter=INF_MAX_ITER_DEFAULT):
        """model: the controller model of candidates that carry none (may be None if every candidate carries one);
        surrogate: the simulation model (default: `model`); term_check_every: with a user termination condition,
        the length of the first device run (doubled until every candidate has ended); infinite_horizon: "refuse"
        scores a ``finite_horizon`` false candidate ``inf`` unrun, "iterate" runs it (module docstring) with
        ``_inf_horz_dt_lqr``'s threshold `inf_threshold` and at most `inf_max_iter` Riccati steps.  The default cap of
        10000 is a choice, not a measurement: that many steps of a 235-state model take of the order of ten seconds,
        and an ARX model with a noticeable bias never converges, so lower it when tuning ARX models."""
        self.infinite_horizon = check_infinite_horizon(infinite_horizon)
        check_inf_params(inf_threshold, inf_max_iter)
        self.inf_threshold, self.inf_max_iter = float(inf_threshold), int(inf_max_iter)
        if surrogate is None:
            surrogate = model
        if surrogate is None:
            raise ValueError("LqrCandidateEvaluator needs a surrogate (or a model to simulate against)")
        if not hasattr(surrogate, "stage_into"):
            raise TypeError("needs a device-stageable surrogate (autompc_amd.sysid models)")
        if system.ctrl_dim > MAX_DEVICE_CTRLS:
            raise ValueError("LQR plans take at most %d controls" % MAX_DEVICE_CTRLS)
        self.system, self.task, self.model, self.surrogate = system, task, model, surrogate
        self.device = device
        self.term_check_every = max(1, int(term_check_every))
        self.precision = "f64"
        b = task.get_ctrl_bounds()
        self.umin, self.umax = b[:, 0].copy(), b[:, 1].copy()
        # QuadCostFactory takes the task cost's goal, NaN entries zeroed (quad_cost_factory.py:64-95)
        self.goal = np.nan_to_num(_task_goal(task.get_cost(), system.obs_dim), nan=0.0)
        self.last_lengths = None
        self.host_fallbacks = 0          # candidates scored on the host (models the device does not take)
        self.last_status = None          # per candidate: 0 scored, 1 singular gain, 2 infinite horizon refused,
        #                                  3 infinite horizon not converged at inf_max_iter
        self.last_iterations = None      # per candidate: Riccati steps of its gain (0: none computed)

    # -- one candidate's pieces --------------------------------------------------------------------------
    def _prepare(self, c):
        """(finite, model, horizon, Q, R, F) of a candidate, with the drop-in's refusals; horizon 0 for an infinite
        horizon that is iterated, and model None for one that is refused."""
        if not isinstance(c, dict):
            raise TypeError("LQR candidates are dicts")
        if c.get("controller", "lqr") != "lqr":
            raise ValueError("LqrCandidateEvaluator scores controller='lqr' candidates, not %r" % c.get("controller"))
        finite = is_finite_horizon(c.get("finite_horizon", True))
        if not finite and self.infinite_horizon == "refuse":
            return False, None, None, None, None, None
        model = c.get("model")
        model = self.model if model is None else model
        if model is None:
            raise ValueError("candidate carries no model and the evaluator has none")
        check_linear(model)
        no, nu = self.system.obs_dim, self.system.ctrl_dim
        if not finite:                     # F is not used (lqr.py:101-104)
            F = _as_matrix(c["F"], no) if c.get("F") is not None else np.zeros((no, no))
            return False, model, 0, _as_matrix(c["Q"], no), _as_matrix(c["R"], nu), F
        horizon = int(c["horizon"])
        check_horizon(horizon)
        return True, model, horizon, _as_matrix(c["Q"], no), _as_matrix(c["R"], nu), _as_matrix(c["F"], no)

    def _controller_task(self, Q, R, F):
        """The task the drop-in LQR of a candidate sees: its QuadCost about the task's goal, the task's bounds."""
        from ..costs import QuadCost
        from ..task import Task
        t = Task(self.system)
        t.set_cost(QuadCost(self.system, Q, R, F, goal=self.goal))
        t.set_ctrl_bounds(self.umin, self.umax)
        return t

    # -- evaluation --------------------------------------------------------------------------------------
    def evaluate(self, candidates, n_steps=None, seed=0, init_obs=None, return_trajectories=False, index_offset=0):
        """``surr_cost`` of every candidate (pipeline_tuner.py:213-258).  Episode as CandidateEvaluator.evaluate:
        eval_cfg's (``task.term_cond``, ``max_steps = task.get_num_steps()``) or exactly ``n_steps`` control steps.
        seed / index_offset are accepted for interface compatibility (nothing here is random).

        return_trajectories: also obs [B, rows, obs_dim], ctrls [B, rows, ctrl_dim], NaN-padded past each
        candidate's ``last_lengths``; a candidate scored ``inf`` keeps only its initial row."""
        from ..trajectory import Trajectory
        B = len(candidates)
        if B == 0:
            return (np.zeros(0), None, None) if return_trajectories else np.zeros(0)
        no, nu = self.system.obs_dim, self.system.ctrl_dim
        prep = [self._prepare(c) for c in candidates]
        if n_steps is not None:
            n_ctl, term_cond = int(n_steps), None
        else:
            max_steps, term_cond = episode_of(self.task)
            n_ctl = default_episode_controls(self.task) if term_cond is None else max_steps
        x0 = np.asarray(self.task.get_init_obs() if init_obs is None else init_obs, dtype=np.float64).reshape(no)
        t0 = Trajectory(self.system, 1, x0[None].copy(), np.zeros((1, nu)))
        try:
            terms = cost_terms(self.task.get_cost(), no, nu)
        except TypeError:
            terms = None                  # a user-defined cost object: scored through its own interface
        obs = np.full((B, n_ctl + 1, no), np.nan)
        ctl = np.full((B, n_ctl + 1, nu), np.nan)
        obs[:, 0], ctl[:, 0] = x0, 0.0
        lengths = np.ones(B, dtype=np.int64)
        scores = np.full(B, np.inf)
        status = np.full(B, 2, dtype=np.int32)
        iterations = np.zeros(B, dtype=np.int64)
        dev, host = [], []
        rules = {}
        for i, (finite, model, *_rest) in enumerate(prep):
            if model is None:              # an infinite horizon, refused
                continue
            r = rules.setdefault(id(model), device_rule(model, no))
            (dev if r is not None else host).append(i)
        if dev:
            self._evaluate_device(prep, dev, rules, x0, t0, n_ctl, term_cond, terms, obs, ctl, lengths, scores,
                                  status, iterations)
        for i in host:
            self._evaluate_host(prep[i], i, x0, n_ctl, term_cond, obs, ctl, lengths, scores, status, iterations)
        self.host_fallbacks += len(host)
        self.last_lengths = lengths
        self.last_status = status
        self.last_iterations = iterations
        if return_trajectories:
            Lmax = int(lengths.max())
            return scores, obs[:, :Lmax], ctl[:, :Lmax]
        return scores

    def _evaluate_device(self, prep, dev, rules, x0, t0, n_ctl, term_cond, terms, obs, ctl, lengths, scores, status,
                         iterations):
        no, nu = self.system.obs_dim, self.system.ctrl_dim
        opened = []
        try:
            sur = _lib.Handle(self.device, "f64")
            opened.append(sur)
            self.surrogate.stage_into(sur)
            handles = {}
            for i in dev:
                m = prep[i][1]
                if id(m) not in handles:               # each distinct model staged once per call
                    handles[id(m)] = model_handle(m, self.device, "f64", opened)
            models = [prep[i][1] for i in dev]
            plan = _lib.LqrPlan([handles[id(m)] for m in models], no, nu, device=self.device)
            opened.append(plan)
            Q = np.array([prep[i][3] for i in dev])
            R = np.array([prep[i][4] for i in dev])
            F = np.array([prep[i][5] for i in dev])
            hz = np.array([prep[i][2] for i in dev])
            inf = hz == 0
            rl = [rules[id(m)] for m in models]
            if inf.any():                      # one launch for finite and infinite problems alike
                _, st, its = plan.gains_ex(hz, Q, R, F, thresholds=self.inf_threshold, max_iters=self.inf_max_iter)
                # InfiniteHorizonLQR.run subtracts no goal and does not clip (lqr.py:126-136)
                goal = np.where(inf[:, None], 0.0, np.tile(self.goal, (len(dev), 1)))
                plan.set_loop([r for r, _ in rl], goal, self.umin, self.umax, lifts=[lift for _, lift in rl],
                              clip=(~inf).astype(np.int32))
            else:
                _, st = plan.gains(hz, Q, R, F)
                its = hz + 1
                plan.set_loop([r for r, _ in rl], np.tile(self.goal, (len(dev), 1)), self.umin, self.umax,
                              lifts=[lift for _, lift in rl])
            init_states = [m.traj_to_state(t0) for m in models]
            init_sim = np.tile(np.asarray(self.surrogate.traj_to_state(t0), dtype=np.float64), (len(dev), 1))
            idx = np.asarray(dev)
            ok = st == 0
            status[idx] = np.where(ok, 0, np.where(st == 2, 3, 1))
            iterations[idx] = its
            if n_ctl == 0:                     # max_steps = 0: the one-row trajectory is scored as is
                o, c = obs[idx, :1].copy(), ctl[idx, :1].copy()
                sc = self._score(sur, terms, o, c)
            elif term_cond is None:
                if terms is not None:
                    sc, o, c = plan.closed_loop(sur, init_states, init_sim, n_ctl, terms=terms)
                else:
                    o, c = plan.closed_loop(sur, init_states, init_sim, n_ctl)
                    sc = self._score(sur, None, o, c)
                obs[idx], ctl[idx] = o, c
                lengths[idx] = n_ctl + 1
            else:
                sc = self._device_until(plan, sur, init_states, init_sim, idx, n_ctl, term_cond, terms, obs, ctl,
                                        lengths)
            scores[idx] = np.where(ok, sc, np.inf)
            bad = idx[~ok]                     # singular or unconverged gain: no trajectory (eval_cfg keeps none)
            obs[bad, 1:], ctl[bad, 1:] = np.nan, np.nan
            ctl[bad, 0] = 0.0
            lengths[bad] = 1
        finally:
            for obj in reversed(opened):
                obj.close()

    def _device_until(self, plan, sur, init_states, init_sim, idx, max_steps, term_cond, terms, obs, ctl, lengths):
        """Episodes that end on a host condition: device runs of growing length from the start, each trajectory cut
        at the first row where ``term_cond`` holds (simulate() asks after appending a row, simulation.py:59-63)."""
        from ..trajectory import Trajectory
        no = self.system.obs_dim
        n = len(idx)
        end = np.zeros(n, dtype=np.int64)      # rows of a finished episode (0: still running)
        asked = np.ones(n, dtype=np.int64)     # rows 0..asked-1 have been asked about
        L = min(self.term_check_every, max_steps)
        while True:
            o, c = plan.closed_loop(sur, init_states, init_sim, L)
            for j in np.nonzero(end == 0)[0]:
                for t in range(int(asked[j]), L + 1):        # rows 0..t exist, control row t is zero
                    rows_c = c[j, :t + 1].copy()
                    rows_c[t] = 0.0
                    if term_cond(Trajectory(self.system, t + 1, o[j, :t + 1, :no].copy(), rows_c)):
                        end[j] = t + 1
                        break
                asked[j] = L + 1
            if L >= max_steps or np.all(end > 0):
                break
            L = min(2 * L, max_steps)
        end[end == 0] = max_steps + 1
        scores = np.empty(n)
        for E in np.unique(end):
            sel = np.nonzero(end == E)[0]
            oc, cc = o[sel, :E].copy(), c[sel, :E].copy()
            cc[:, E - 1] = 0.0                               # simulate()'s trailing zero control row
            scores[sel] = self._score(sur, terms, oc, cc)
            obs[idx[sel], :E], ctl[idx[sel], :E] = oc, cc
        lengths[idx] = end
        return scores

    def _score(self, sur, terms, obs, ctrls):
        no = self.system.obs_dim
        if terms is not None:
            return sur.score_trajectories(terms, obs, ctrls, obs_dim=no)
        return score_trajectories(self.task.get_cost(), obs[:, :, :no], ctrls)

    def _evaluate_host(self, p, i, x0, n_ctl, term_cond, obs, ctl, lengths, scores, status, iterations):
        """A model the device cannot take: the reference's recursion and simulate() on the host."""
        from ..utils import simulate
        finite, model, horizon, Q, R, F = p
        try:
            if finite:
                ctl_i = _HostFiniteHorizonLQR(self.system, self._controller_task(Q, R, F), model, horizon)
                iterations[i] = horizon + 1
            else:
                ctl_i = _HostInfiniteHorizonLQR(self.system, self._controller_task(Q, R, F), model, "iterate",
                                                self.inf_threshold, self.inf_max_iter)
                iterations[i] = ctl_i.iters
        except RiccatiNotConverged:
            iterations[i] = self.inf_max_iter
            status[i] = 3
            return
        except np.linalg.LinAlgError:
            ctl_i = None
        if ctl_i is None or not np.all(np.isfinite(ctl_i.K)):  # (the device's status 1)
            status[i] = 1
            return
        ctl_i.reset()
        traj = simulate(ctl_i, x0, term_cond, sim_model=self.surrogate, max_steps=n_ctl, silent=True)
        L = len(traj)
        obs[i, :L], ctl[i, :L] = traj.obs, traj.ctrls
        lengths[i] = L
        scores[i] = float(self.task.get_cost()(traj))
        status[i] = 0


def random_lqr_candidates(system, n, seed=0):
    """Candidates drawn from LQRFactory's space (control/lqr.py:214-224): finite_horizon uniform over
    {"true", "false"}, horizon uniform in 1..1000 (drawn for every candidate, read only when finite); QuadCost
    diagonal gains log-uniform in [1e-3, 1e4] (quad_cost_factory.py:46-58)."""
    rng = np.random.default_rng(seed)
    no, nu = system.obs_dim, system.ctrl_dim
    out = []
    for _ in range(n):
        finite = bool(rng.integers(2) == 0)
        horizon = int(rng.integers(1, 1001))
        c = dict(controller="lqr", finite_horizon=finite, Q=10 ** rng.uniform(-3, 4, size=no),
                 R=10 ** rng.uniform(-3, 4, size=nu), F=10 ** rng.uniform(-3, 4, size=no))
        if finite:
            c["horizon"] = horizon
        out.append(c)
    return out
