#!/usr/bin/env python3
"""Golden vectors of the infinite-horizon LQR gain and controller, from the REAL reference (williamedwards/autompc).

Run in the build container only (needs the reference checkout that gen_golden.py installs):

    python tests/golden/gen_golden_lqr_inf.py

Writes ``tests/golden/lqrinf_*.npz`` (data only).  The reference's ``InfiniteHorizonLQR.__init__`` calls an undefined
``dare`` (lqr.py:104), so the class cannot be constructed; the gain function it was written around,
``_inf_horz_dt_lqr`` (lqr.py:22-33), can be called.  Per case, on an ARX / Koopman model the reference trained on
seeded trajectories (``gen_golden_lqr.training_trajs``):

* ``K``: ``_inf_horz_dt_lqr(A, B, Qp, R, 0, threshold)`` with Q zero-padded as ``InfiniteHorizonLQR.__init__`` pads it
  (lqr.py:102-103);
* ``dP`` and ``iters``: max|P_new - P_old| after every Riccati step, from a loop over the reference's own
  ``_dynamic_ricatti_equation`` with ``_inf_horz_dt_lqr``'s stopping rule, and the number of steps.  Every entry
  before the last is > threshold (1 + 1e-6) and the last < threshold (1 - 1e-6) (asserted), so one rounding cannot
  change the count;
* ``obs`` / ``ctrls`` / ``cstate0``: the reference's ``simulate()`` driving a small controller object whose ``run`` is
  the body of ``InfiniteHorizonLQR.run`` (lqr.py:126-136, prints left out) -- against the model itself or against a
  seeded MLP surrogate (``oracle.mlp.random_params(seed)`` + ``normalisers(seed)``, weights not stored).

Also stored: the model parameters (``coeffs`` / ``A``, ``B``), Q, R, the task's goal and bounds (neither is applied by
the controller: the ARX-2 case has both, and asserts a control outside the bounds), init_obs, threshold.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G                                        # noqa: E402  (installs the reference)
import gen_golden_lqr as GL                                   # noqa: E402  (training_trajs, make_task, coeffs_of)
from autompc.control import lqr as ref_lqr                    # noqa: E402
from autompc.sysid.arx import ARX                             # noqa: E402
from autompc.sysid.koopman import Koopman                     # noqa: E402

THRESHOLD = 1e-3
MARGIN = 1e-6


class InfLoopController:
    """What simulate() needs of InfiniteHorizonLQR (lqr.py:109-136) around a gain computed elsewhere."""

    def __init__(self, system, model, K):
        self.system, self.model, self.K = system, model, K

    def traj_to_state(self, traj):
        return np.concatenate([self.model.traj_to_state(traj), traj[-1].ctrl])

    def run(self, state, new_obs):
        nu = self.system.ctrl_dim
        modelstate = self.model.update_state(state[:-nu], state[-nu:], new_obs)
        u = np.array(self.K @ modelstate).flatten()
        return u, np.concatenate([modelstate, u])


def dp_sequence(A, B, Qp, R, threshold, limit=100000):
    """max|P_new - P_old| after every step of _inf_horz_dt_lqr's loop (lqr.py:23-29)."""
    N = np.zeros((A.shape[0], B.shape[1]))
    P1 = Qp
    P2 = ref_lqr._dynamic_ricatti_equation(A, B, Qp, R, N, P1)
    out = [np.abs(P1 - P2).max()]
    while out[-1] > threshold:
        assert len(out) < limit, "no convergence"
        P1 = P2
        P2 = ref_lqr._dynamic_ricatti_equation(A, B, Qp, R, N, P1)
        out.append(np.abs(P1 - P2).max())
    return np.array(out)


def run_case(name, system, model, task, n_steps, sim_model=None, init_obs=None, extra=None):
    A, B = model.to_linear()
    n = model.state_dim
    Q, R, _ = task.get_cost().get_cost_matrices()
    Qp = np.zeros((n, n))
    Qp[:Q.shape[0], :Q.shape[1]] = Q
    N = np.zeros((A.shape[0], B.shape[1]))
    K = np.asarray(ref_lqr._inf_horz_dt_lqr(A, B, Qp, R, N, THRESHOLD))
    dP = dp_sequence(A, B, Qp, R, THRESHOLD)
    assert np.all(dP[:-1] > THRESHOLD * (1 + MARGIN)) and dP[-1] < THRESHOLD * (1 - MARGIN), (name, dP)
    margin = min(np.min(dP[:-1] / THRESHOLD - 1), 1 - dP[-1] / THRESHOLD)
    b = task.get_ctrl_bounds()
    out = dict(K=K, dP=dP, iters=len(dP), threshold=THRESHOLD, Q=Q, R=R, umin=b[:, 0].copy(), umax=b[:, 1].copy())
    if n_steps:
        init_obs = np.asarray(init_obs, dtype=np.float64)
        ctl = InfLoopController(system, model, K)
        t0 = G.ampc.zeros(system, 1)
        t0[0].obs[:] = init_obs
        traj = G.quiet(G.simulate, ctl, init_obs, sim_model=sim_model or model, max_steps=n_steps, silent=True)
        out.update(init_obs=init_obs, cstate0=ctl.traj_to_state(t0), obs=np.asarray(traj.obs),
                   ctrls=np.asarray(traj.ctrls))
    out.update(extra or {})
    print("%-12s n = %3d  iters = %3d  margin = %.2f %%" % (name, n, len(dP), 100 * margin))
    G.save("lqrinf_" + name, **out)
    return out


def gen():
    # small ARX: history 2 on 4 obs / 1 ctrl; the task has a non-zero goal and bounds, and the controller applies neither
    s4 = G.make_system(4, 1)
    arx2 = ARX(s4, history=2)
    G.quiet(arx2.train, GL.training_trajs(s4, 1))
    goal = np.array([0.5, -0.3, 0.2, 0.1])
    task = GL.make_task(s4, np.diag([1.0, 2.0, 0.5, 1.5]), 0.1 * np.eye(1), np.diag([3.0, 1.0, 1.0, 2.0]), goal, 0.4)
    o = run_case("arx2", s4, arx2, task, 50, init_obs=[1.0, -1.0, 0.5, 0.0],
                 extra=dict(coeffs=GL.coeffs_of(arx2), goal=goal, history=2))
    assert np.any(np.abs(o["ctrls"][:-1]) > 0.4), "no control outside the bounds"

    # Koopman with a polynomial basis against a seeded MLP surrogate (the lift rule)
    koop = Koopman(s4, method="lstsq", poly_basis="true", poly_degree=3, trig_basis="false", product_terms="false")
    G.quiet(koop.train, GL.training_trajs(s4, 4))
    sur4, _ = G.ref_mlp(s4, [16], "relu", 62)
    task_k = GL.make_task(s4, np.eye(4), 0.1 * np.eye(1), np.eye(4), goal, 0.5)
    run_case("koop_mlp", s4, koop, task_k, 40, sim_model=sur4, init_obs=[0.3, -0.2, 0.1, 0.4],
             extra=dict(A=koop.A, B=koop.B, goal=goal, poly_degree=3, sur_seed=62, sur_hidden=[16]))

    # ARX history 4 at HalfCheetah shape against a seeded MLP surrogate (the ARX-shift rule)
    s17 = G.make_system(17, 6)
    arx4 = ARX(s17, history=4)
    G.quiet(arx4.train, GL.training_trajs(s17, 2))
    sur, _ = G.ref_mlp(s17, [32, 32], "tanh", 61)
    goal17 = np.linspace(-0.2, 0.2, 17)
    task17 = GL.make_task(s17, np.eye(17), 0.5 * np.eye(6), 2.0 * np.eye(17), goal17, 1.0)
    run_case("arx4_mlp", s17, arx4, task17, 30, sim_model=sur,
             init_obs=np.random.default_rng(3).uniform(-0.5, 0.5, size=17),
             extra=dict(coeffs=GL.coeffs_of(arx4), goal=goal17, history=4, sur_seed=61, sur_hidden=[32, 32]))

    # wide ARX: history 10 at HalfCheetah shape (225 states), gain only
    arx10 = ARX(s17, history=10)
    G.quiet(arx10.train, GL.training_trajs(s17, 5, n=8, L=80))
    run_case("arx10_wide", s17, arx10, task17, 0, extra=dict(coeffs=GL.coeffs_of(arx10), goal=goal17, history=10))


if __name__ == "__main__":
    gen()
