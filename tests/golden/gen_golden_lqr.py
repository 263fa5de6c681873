#!/usr/bin/env python3
"""Golden vectors of the LQR controller, from the REAL reference (williamedwards/autompc).

Run in the build container only (needs the reference checkout that gen_golden.py installs):

    python tests/golden/gen_golden_lqr.py

Writes ``tests/golden/lqr_*.npz`` (data only).  Every case builds the reference's ``FiniteHorizonLQR`` directly
(``LQRFactory`` needs ConfigSpace) on an ARX / Koopman model the reference trained on seeded trajectories, records
its gain K and the trajectory of the reference's own ``simulate()`` -- against the controller model itself or
against a seeded MLP surrogate (``oracle.mlp.random_params(seed)`` + ``normalisers(seed)``, as in gen_golden.py,
weights not stored).  Stored per case: the model parameters (``coeffs`` / ``A``, ``B``), Q, R, F, goal, bounds,
init_obs, the controller state simulate() starts from, and per horizon h ``K_h``, ``obs_h``, ``ctrls_h``.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G                                        # noqa: E402  (installs the reference)
from autompc.control.lqr import FiniteHorizonLQR              # noqa: E402
from autompc.costs.sum_cost import SumCost                    # noqa: E402
from autompc.sysid.arx import ARX                             # noqa: E402
from autompc.sysid.koopman import Koopman                     # noqa: E402


def training_trajs(system, seed, n=6, L=60):
    """Trajectories of a seeded stable linear system with noise (what the models are fitted to)."""
    rng = np.random.default_rng(seed)
    no, nu = system.obs_dim, system.ctrl_dim
    A = 0.9 * np.linalg.qr(rng.normal(size=(no, no)))[0]
    B = 0.3 * rng.normal(size=(no, nu))
    out = []
    for _ in range(n):
        t = G.ampc.zeros(system, L)
        x = rng.normal(size=no)
        for i in range(L):
            u = rng.normal(size=nu)
            t.obs[i], t.ctrls[i] = x, u
            x = A @ x + B @ u + 0.01 * rng.normal(size=no)
        out.append(t)
    return out


def coeffs_of(model):
    """ARX regression coefficients [obs_dim][fvec] (the reference keeps only A and B, arx.py:137-143)."""
    n = model.system.obs_dim
    return np.hstack([model.A[:n], model.B[:n]])


def make_task(system, Q, R, F, goal, umax=None, cost=None):
    task = G.Task(system)
    task.set_cost(cost if cost is not None else G.QuadCost(system, Q, R, F, goal=goal))
    if umax is not None:
        task.set_ctrl_bounds(np.full(system.ctrl_dim, -umax), np.full(system.ctrl_dim, umax))
    return task


def run_case(name, system, model, task, horizons, n_steps, sim_model=None, init_obs=None, extra=None):
    init_obs = np.asarray(init_obs, dtype=np.float64)
    out = dict(init_obs=init_obs, horizons=np.array(horizons))
    Q, R, F = task.get_cost().get_cost_matrices()
    out.update(Q=Q, R=R, F=F)
    b = task.get_ctrl_bounds()
    out.update(umin=b[:, 0].copy(), umax=b[:, 1].copy())
    for h in horizons:
        ctl = G.quiet(FiniteHorizonLQR, system, task, model, h)
        out["K_%d" % h] = np.asarray(ctl.K)
        if n_steps:
            t0 = G.ampc.zeros(system, 1)
            t0[0].obs[:] = init_obs
            out["cstate0_%d" % h] = ctl.traj_to_state(t0)
            traj = G.quiet(G.simulate, ctl, init_obs, sim_model=sim_model or model, max_steps=n_steps, silent=True)
            out["obs_%d" % h] = np.asarray(traj.obs)
            out["ctrls_%d" % h] = np.asarray(traj.ctrls)
    out.update(extra or {})
    G.save("lqr_" + name, **out)
    return out


def gen():
    # small ARX: history 2 on 4 obs / 1 ctrl, non-zero goal, bounds the episode hits
    s4 = G.make_system(4, 1)
    arx2 = ARX(s4, history=2)
    G.quiet(arx2.train, training_trajs(s4, 1))
    goal = np.array([0.5, -0.3, 0.2, 0.1])
    task = make_task(s4, np.diag([1.0, 2.0, 0.5, 1.5]), 0.1 * np.eye(1), np.diag([3.0, 1.0, 1.0, 2.0]), goal, 0.4)
    o = run_case("arx2_small", s4, arx2, task, [1, 10, 200, 1000], 50, init_obs=[1.0, -1.0, 0.5, 0.0],
                 extra=dict(coeffs=coeffs_of(arx2), goal=goal, history=2))
    assert any(np.any(np.abs(o["ctrls_%d" % h][:-1]) >= 0.4 - 1e-12) for h in (1, 10, 200, 1000)), "bounds not hit"

    # SumCost of two QuadCosts (get_cost_matrices sums them, sum_cost.py:30-42): gains only (the reference's
    # SumCost.get_goal returns a cost object, so FiniteHorizonLQR.run cannot run on it)
    c1 = G.QuadCost(s4, np.diag([1.0, 0.0, 2.0, 0.0]), 0.05 * np.eye(1), np.eye(4), goal=goal)
    c2 = G.QuadCost(s4, np.diag([0.5, 1.0, 0.0, 1.0]), 0.2 * np.eye(1), np.diag([0.0, 1.0, 2.0, 3.0]), goal=goal)
    task_sum = make_task(s4, None, None, None, None, 0.4, cost=SumCost(s4, [c1, c2]))
    run_case("sumcost", s4, arx2, task_sum, [10, 100], 0, init_obs=np.zeros(4),
             extra=dict(coeffs=coeffs_of(arx2), goal=goal, history=2,
                        Q1=c1.get_cost_matrices()[0], R1=c1.get_cost_matrices()[1], F1=c1.get_cost_matrices()[2],
                        Q2=c2.get_cost_matrices()[0], R2=c2.get_cost_matrices()[1], F2=c2.get_cost_matrices()[2]))

    # ARX history 4 at HalfCheetah shape against a seeded MLP surrogate (the ARX-shift rule, first step included)
    s17 = G.make_system(17, 6)
    arx4 = ARX(s17, history=4)
    G.quiet(arx4.train, training_trajs(s17, 2))
    sur, _ = G.ref_mlp(s17, [32, 32], "tanh", 61)
    goal17 = np.linspace(-0.2, 0.2, 17)
    task17 = make_task(s17, np.eye(17), 0.5 * np.eye(6), 2.0 * np.eye(17), goal17, 1.0)
    run_case("arx4_mlp", s17, arx4, task17, [10, 500], 30, sim_model=sur,
             init_obs=np.random.default_rng(3).uniform(-0.5, 0.5, size=17),
             extra=dict(coeffs=coeffs_of(arx4), goal=goal17, history=4, sur_seed=61, sur_hidden=[32, 32]))

    # Koopman with a polynomial basis against a seeded MLP surrogate (the lift rule)
    koop = Koopman(s4, method="lstsq", poly_basis="true", poly_degree=3, trig_basis="false", product_terms="false")
    G.quiet(koop.train, training_trajs(s4, 4))
    sur4, _ = G.ref_mlp(s4, [16], "relu", 62)
    task_k = make_task(s4, np.eye(4), 0.1 * np.eye(1), np.eye(4), goal, 0.5)
    run_case("koop_mlp", s4, koop, task_k, [20], 40, sim_model=sur4, init_obs=[0.3, -0.2, 0.1, 0.4],
             extra=dict(A=koop.A, B=koop.B, goal=goal, poly_degree=3, sur_seed=62, sur_hidden=[16]))

    # wide ARX: history 10 at HalfCheetah shape (225 states), closed loop on the model itself
    arx10 = ARX(s17, history=10)
    G.quiet(arx10.train, training_trajs(s17, 5, n=8, L=80))
    run_case("arx10_wide", s17, arx10, task17, [50], 10, init_obs=np.full(17, 0.1),
             extra=dict(coeffs=coeffs_of(arx10), goal=goal17, history=10))

    # singular: R = 0 and a control that moves nothing -> R + B'PB singular, the reference raises
    s2 = G.make_system(3, 2)
    arx1 = ARX(s2, history=2)
    G.quiet(arx1.train, training_trajs(s2, 6))
    arx1.B[:, -1] = 0.0
    coeffs = coeffs_of(arx1)
    task_s = make_task(s2, np.eye(3), np.zeros((2, 2)), np.eye(3), np.zeros(3))
    raised = 0
    try:
        G.quiet(FiniteHorizonLQR, s2, task_s, arx1, 5)
    except np.linalg.LinAlgError:
        raised = 1
    assert raised
    G.save("lqr_singular", coeffs=coeffs, history=2, Q=np.eye(3), R=np.zeros((2, 2)), F=np.eye(3), horizon=5,
           raised=raised)


if __name__ == "__main__":
    gen()
