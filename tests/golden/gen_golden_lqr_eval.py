#!/usr/bin/env python3
"""Golden scores of LQR pipeline candidates, from the REAL reference (williamedwards/autompc).

Run in the build container only (needs the reference checkout that gen_golden.py installs):

    python tests/golden/gen_golden_lqr_eval.py

Writes ``tests/golden/lqreval_*.npz`` (data only).  Every case is the surrogate branch of the reference's
``PipelineTuner.eval_cfg`` (tuning/pipeline_tuner.py:213-239) for one (ARX | Koopman) x LQR x QuadCost
configuration: the model comes from the reference's own ``ARXFactory`` / ``KoopmanFactory`` trained on seeded
trajectories, the controller cost from its ``QuadCostFactory`` about the task's goal, the controller is
``FiniteHorizonLQR`` on a copy of the task carrying that cost (what ``Pipeline.__call__`` builds), then
``simulate(controller, init_obs, task.term_cond, sim_model=surrogate, max_steps=task.get_num_steps())`` and
``task.get_cost()(traj)``; a ``LinAlgError`` scores inf.  Surrogates: a seeded MLP (gen_golden.ref_mlp, weights not
stored) or a trained ARX (coefficients stored).  Stored per case: the configuration (JSON), the model parameters,
the task (Q, R, F, goal, bounds, init_obs, num_steps), the score and the trajectory.
"""
import copy
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G                                        # noqa: E402  (installs the reference)
from gen_golden_lqr import coeffs_of, training_trajs          # noqa: E402
from autompc.control.lqr import FiniteHorizonLQR              # noqa: E402
from autompc.costs.quad_cost_factory import QuadCostFactory   # noqa: E402
from autompc.sysid.arx import ARXFactory                      # noqa: E402
from autompc.sysid.koopman import KoopmanFactory              # noqa: E402


class Cfg(dict):
    def get_dictionary(self):
        return dict(self)


def subspace(cfg, prefix):
    return Cfg({k[len(prefix) + 1:]: v for k, v in cfg.items() if k.startswith(prefix + ":")})


def gains(rng, system):
    out = {}
    for n in system.observations:
        out["_cost:%s_Q" % n] = float(10 ** rng.uniform(-1, 1))
    for n in system.observations:
        out["_cost:%s_F" % n] = float(10 ** rng.uniform(-1, 1))
    for n in system.controls:
        out["_cost:%s_R" % n] = float(10 ** rng.uniform(-1, 1))
    return out


def run_case(name, system, cfg, trajs, sur, sur_info, goal, umax, init_obs, num_steps, tweak=None):
    no, nu = system.obs_dim, system.ctrl_dim
    task = G.Task(system)
    Qt, Rt, Ft = np.eye(no), 0.1 * np.eye(nu), 2.0 * np.eye(no)
    task.set_cost(G.QuadCost(system, Qt, Rt, Ft, goal=goal))
    if umax is not None:
        task.set_ctrl_bounds(np.full(nu, -umax), np.full(nu, umax))
    task.set_init_obs(np.asarray(init_obs, dtype=np.float64))
    task.set_num_steps(num_steps)
    mcfg = subspace(cfg, "_model")
    factory = ARXFactory(system) if "history" in mcfg else KoopmanFactory(system)
    model = G.quiet(factory, mcfg, trajs)
    if tweak is not None:
        tweak(model)
    cost = QuadCostFactory(system)(subspace(cfg, "_cost"), task, trajs)
    new_task = copy.deepcopy(task)
    new_task.set_cost(cost)
    ctrl = subspace(cfg, "_ctrlr")
    assert ctrl["finite_horizon"] == "true"
    raised = 0
    try:
        controller = G.quiet(FiniteHorizonLQR, system, new_task, model, int(ctrl["horizon"]))
        controller.reset()
        traj = G.quiet(G.simulate, controller, task.get_init_obs(), task.term_cond, sim_model=sur,
                       max_steps=task.get_num_steps())
        score = float(task.get_cost()(traj))
        obs, ctrls = np.asarray(traj.obs), np.asarray(traj.ctrls)
    except np.linalg.LinAlgError:
        raised, score = 1, np.inf
        obs, ctrls = np.zeros((0, no)), np.zeros((0, nu))
    out = dict(cfg=np.array(json.dumps(cfg, sort_keys=True)), no=no, nu=nu, score=score, raised=raised, obs=obs,
               ctrls=ctrls, Qt=Qt, Rt=Rt, Ft=Ft, goal=np.asarray(goal, dtype=np.float64),
               umax=np.inf if umax is None else float(umax), init_obs=np.asarray(init_obs, dtype=np.float64),
               num_steps=num_steps, **sur_info)
    if "history" in mcfg:
        out.update(model_kind="arx", coeffs=coeffs_of(model))
    else:
        out.update(model_kind="koopman", A=model.A, B=model.B)
    G.save("lqreval_" + name, **out)
    return score


def gen():
    rng = np.random.default_rng(2024)
    s4, s6, s3 = G.make_system(4, 1), G.make_system(6, 2), G.make_system(3, 2)
    tr4, tr6, tr3 = training_trajs(s4, 11), training_trajs(s6, 12, n=8, L=80), training_trajs(s3, 13)
    mlp4, _ = G.ref_mlp(s4, [32], "tanh", 81)
    mlp6, _ = G.ref_mlp(s6, [32, 32], "tanh", 82)
    lin6 = G.quiet(ARXFactory(s6), Cfg(history=2), tr6)
    m4 = dict(sur_kind="mlp", sur_seed=81, sur_hidden=[32], sur_act="tanh")
    m6 = dict(sur_kind="mlp", sur_seed=82, sur_hidden=[32, 32], sur_act="tanh")
    l6 = dict(sur_kind="arx", sur_history=2, sur_coeffs=coeffs_of(lin6))
    g4, g6 = np.array([0.3, -0.2, 0.1, 0.0]), np.linspace(-0.2, 0.2, 6)
    x4, x6 = np.array([0.8, -0.6, 0.4, 0.2]), np.random.default_rng(5).uniform(-0.5, 0.5, 6)

    def cfg(model, horizon, system):
        c = {"_model:%s" % k: v for k, v in model.items()}
        c.update({"_ctrlr:finite_horizon": "true", "_ctrlr:horizon": horizon})
        c.update(gains(rng, system))
        return c

    koop_poly = dict(method="lstsq", poly_basis="true", poly_degree=3, trig_basis="false", product_terms="false")
    koop_trig = dict(method="lstsq", poly_basis="false", trig_basis="true", trig_freq=2, product_terms="false")
    run_case("arx1_h10_mlp_bounded", s4, cfg({"history": 1}, 10, s4), tr4, mlp4, m4, g4, 0.3, x4, 40)
    run_case("koop_poly_h10_mlp", s4, cfg(koop_poly, 10, s4), tr4, mlp4, m4, g4, 0.5, x4, 40)
    run_case("arx4_h1000_mlp", s6, cfg({"history": 4}, 1000, s6), tr6, mlp6, m6, g6, None, x6, 30)
    run_case("arx10_h1_lin", s6, cfg({"history": 10}, 1, s6), tr6, lin6, l6, g6, None, x6, 30)
    run_case("koop_trig_h1000_lin", s6, cfg(koop_trig, 1000, s6), tr6, lin6, l6, g6, 1.0, x6, 30)
    run_case("arx2_h200_lin_bounded", s6, cfg({"history": 2}, 200, s6), tr6, lin6, l6, g6, 0.2, x6, 30)
    run_case("koop_poly_h1_mlp", s6, cfg(dict(koop_poly, poly_degree=2), 1, s6), tr6, mlp6, m6, g6, None, x6, 25)

    # singular: a control the model ignores and R = 0 on it -> R + B'PB singular, the reference raises
    c = cfg({"history": 2}, 5, s3)
    c["_cost:u1_R"] = 0.0
    lin3 = G.quiet(ARXFactory(s3), Cfg(history=2), tr3)

    def zero_u1(model):
        model.B[:, -1] = 0.0
    sc = run_case("singular", s3, c, tr3, lin3, dict(sur_kind="arx", sur_history=2, sur_coeffs=coeffs_of(lin3)),
                  np.zeros(3), None, np.ones(3), 20, tweak=zero_u1)
    assert sc == np.inf


if __name__ == "__main__":
    gen()
