"""LqrCandidateEvaluator on the device against the reference's eval_cfg (tests/golden/gen_golden_lqr_eval.py), the
drop-in LQR under simulate(), itself in other batches, a user termination condition, the host fallback and the
tuner.  Needs MI355X."""
import json
import os

import numpy as np
import pytest

from autompc_amd import ARX, ARXFactory, Koopman, QuadCost, System, Task, simulate
from autompc_amd.control.lqr import LQR
from autompc_amd.tuning import (BatchPipelineTuner, LqrCandidateEvaluator, evaluate_sharded,
                                lqr_candidate_from_config, sample_lqr_pipeline_configs)
from test_gpu_lqr import TRAJ_TOL, _training_trajs, seeded_mlp

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
CASES = ["arx1_h10_mlp_bounded", "koop_poly_h10_mlp", "arx4_h1000_mlp", "arx10_h1_lin", "koop_trig_h1000_lin",
         "arx2_h200_lin_bounded", "koop_poly_h1_mlp", "singular"]


def system(no, nu):
    return System(["x%d" % i for i in range(no)], ["u%d" % i for i in range(nu)], dt=0.05)


def _golden(name):
    g = np.load(os.path.join(GOLD, "lqreval_%s.npz" % name))
    s = system(int(g["no"]), int(g["nu"]))
    cfg = json.loads(str(g["cfg"]))
    mcfg = {k[len("_model:"):]: v for k, v in cfg.items() if k.startswith("_model:")}
    if str(g["model_kind"]) == "arx":
        model = ARX(s, history=int(mcfg["history"]))
        model.set_parameters({"coeffs": g["coeffs"]})
    else:
        model = Koopman(s, **mcfg)
        model.set_parameters({"A": g["A"], "B": g["B"]})
    if str(g["sur_kind"]) == "mlp":
        sur = seeded_mlp(s, [int(v) for v in g["sur_hidden"]], str(g["sur_act"]), int(g["sur_seed"]))
    else:
        sur = ARX(s, history=int(g["sur_history"]))
        sur.set_parameters({"coeffs": g["sur_coeffs"]})
    task = Task(s)
    task.set_cost(QuadCost(s, g["Qt"], g["Rt"], g["Ft"], goal=g["goal"]))
    if np.isfinite(float(g["umax"])):
        u = float(g["umax"])
        task.set_ctrl_bounds(np.full(s.ctrl_dim, -u), np.full(s.ctrl_dim, u))
    task.set_init_obs(g["init_obs"])
    task.set_num_steps(int(g["num_steps"]))
    cand = lqr_candidate_from_config(s, cfg)
    cand["model"] = model
    return g, s, task, model, sur, cand


@pytest.mark.parametrize("name", CASES)
def test_golden_parity(name):
    g, s, task, model, sur, cand = _golden(name)
    ev = LqrCandidateEvaluator(s, task, surrogate=sur)
    sc, obs, ctl = ev.evaluate([cand], return_trajectories=True)
    if int(g["raised"]):
        assert sc[0] == np.inf and ev.last_status[0] == 1
        return
    ref = float(g["score"])
    assert abs(sc[0] - ref) <= 1e-8 * abs(ref), (sc[0], ref)
    L = int(ev.last_lengths[0])
    assert L == g["obs"].shape[0]
    assert np.abs(obs[0, :L] - g["obs"]).max() / np.abs(g["obs"]).max() < TRAJ_TOL
    assert np.abs(ctl[0, :L] - g["ctrls"]).max() / max(np.abs(g["ctrls"]).max(), 1e-12) < TRAJ_TOL


# ---- a mixed batch: ARX histories 1..10, Koopman lifts, horizons 1..1000, some infinite horizons -------------
NO, NU, STEPS = 6, 2, 20


def _mixed(B=64, seed=3):
    s = system(NO, NU)
    models = []
    for k in range(1, 11):
        m = ARX(s, history=k)
        m.train(_training_trajs(s, 40 + k))
        models.append(m)
    for i, kw in enumerate([dict(poly_basis=True, poly_degree=2), dict(poly_basis=True, poly_degree=3),
                            dict(trig_basis=True), dict(poly_basis=True, poly_degree=2, trig_basis=True)]):
        m = Koopman(s, method="lstsq", **kw)
        m.train(_training_trajs(s, 60 + i, n=8, L=80))
        models.append(m)
    sur = seeded_mlp(s, [32], "tanh", 91)
    task = Task(s)
    task.set_cost(QuadCost(s, np.eye(NO), 0.1 * np.eye(NU), 2.0 * np.eye(NO), goal=np.linspace(-0.2, 0.2, NO)))
    task.set_ctrl_bounds(-np.ones(NU), np.ones(NU))
    task.set_init_obs(np.random.default_rng(seed).uniform(-0.5, 0.5, NO))
    task.set_num_steps(STEPS)
    rng = np.random.default_rng(seed)
    cands = []
    for i in range(B):
        c = {"controller": "lqr", "finite_horizon": bool(i % 7 != 3), "model": models[i % len(models)],
             "Q": 10 ** rng.uniform(-1, 1, NO), "R": 10 ** rng.uniform(-1, 1, NU), "F": 10 ** rng.uniform(-1, 1, NO)}
        h = int(rng.integers(1, 1001))
        if c["finite_horizon"]:
            c["horizon"] = [1, 1000][i] if i < 2 else h
        cands.append(c)
    return s, task, sur, cands


def _dropin(s, task, sur, c, term_cond=None, max_steps=None):
    t = Task(s)
    t.set_cost(QuadCost(s, np.diag(c["Q"]), np.diag(c["R"]), np.diag(c["F"]), goal=task.get_cost().get_goal()))
    t.set_ctrl_bounds(task.get_ctrl_bounds()[:, 0], task.get_ctrl_bounds()[:, 1])
    ctl = LQR(s, t, c["model"], "true", c["horizon"])
    ctl.reset()
    return simulate(ctl, task.get_init_obs(), term_cond if term_cond is not None else task.term_cond,
                    sim_model=sur, max_steps=max_steps or task.get_num_steps())


def test_mixed_batch_matches_dropin():
    s, task, sur, cands = _mixed()
    ev = LqrCandidateEvaluator(s, task, surrogate=sur)
    sc, obs, ctl = ev.evaluate(cands, return_trajectories=True)
    assert ev.host_fallbacks == 0
    assert len({c["model"].state_dim for c in cands}) == 13
    for i, c in enumerate(cands):
        if not c["finite_horizon"]:
            assert sc[i] == np.inf
            continue
        traj = _dropin(s, task, sur, c)
        ref = float(task.get_cost()(traj))
        assert abs(sc[i] - ref) <= 1e-10 * abs(ref), (i, sc[i], ref)
        L = len(traj)
        assert ev.last_lengths[i] == L == STEPS
        assert np.abs(obs[i, :L] - traj.obs).max() / np.abs(traj.obs).max() < TRAJ_TOL


def test_batch_independence():
    s, task, sur, cands = _mixed()
    ev = LqrCandidateEvaluator(s, task, surrogate=sur)
    sc, obs, ctl = ev.evaluate(cands, return_trajectories=True)

    def same(x, y):                                    # (an infinite-horizon candidate's rows are NaN)
        return np.array_equal(x, y, equal_nan=True)
    for i in (0, 1, 5, 13, 40, 63):                     # alone
        a, o, c = ev.evaluate([cands[i]], return_trajectories=True)
        assert same(a, sc[i:i + 1]) and same(o[0], obs[i]) and same(c[0], ctl[i])
    perm = np.random.default_rng(9).permutation(len(cands))
    a, o, c = ev.evaluate([cands[i] for i in perm], return_trajectories=True)
    assert same(a, sc[perm]) and same(o, obs[perm]) and same(c, ctl[perm])
    for lo, hi in ((0, 23), (23, 64)):
        a, o, c = ev.evaluate(cands[lo:hi], return_trajectories=True)
        assert same(a, sc[lo:hi]) and same(o, obs[lo:hi]) and same(c, ctl[lo:hi])


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    s, task, sur, cands = _mixed()
    ev = LqrCandidateEvaluator(s, task, surrogate=sur)
    scores = evaluate_sharded(lambda shard, lo: ev.evaluate(shard, index_offset=lo), cands, weights="auto")
    q.put((rank, scores))
    dist.destroy_process_group()


def test_sharded_two_ranks_bit_identical():
    import torch.multiprocessing as mp
    from test_sharded_eval import _free_port
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=600) for _ in range(2))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    s, task, sur, cands = _mixed()
    ref = LqrCandidateEvaluator(s, task, surrogate=sur).evaluate(cands)
    for r in range(2):
        assert np.array_equal(got[r], ref)


def test_user_termination_condition():
    s, task, sur, cands = _mixed(B=24, seed=5)
    x0 = task.get_init_obs()
    max_steps = 60

    def cond(traj):                                      # ends when the first coordinate has moved by 0.05
        return abs(traj[-1].obs[0] - x0[0]) > 0.05
    t2 = Task(s)
    t2.set_cost(task.get_cost())
    t2.set_ctrl_bounds(task.get_ctrl_bounds()[:, 0], task.get_ctrl_bounds()[:, 1])
    t2.set_init_obs(x0)
    t2.set_num_steps(max_steps)
    t2.set_term_cond(cond)
    ev = LqrCandidateEvaluator(s, t2, surrogate=sur, term_check_every=4)
    sc, obs, ctl = ev.evaluate(cands, return_trajectories=True)
    lengths = ev.last_lengths.copy()
    full = LqrCandidateEvaluator(s, t2, surrogate=sur)
    _, fo, fc = full.evaluate(cands, n_steps=max_steps, return_trajectories=True)
    ended = 0
    for i, c in enumerate(cands):
        if not c["finite_horizon"]:
            assert sc[i] == np.inf
            continue
        traj = _dropin(s, t2, sur, c, term_cond=cond, max_steps=max_steps)
        L = len(traj)
        ended += L < max_steps + 1
        assert lengths[i] == L, i
        ref = float(t2.get_cost()(traj))
        assert abs(sc[i] - ref) <= 1e-10 * abs(ref), i
        assert np.array_equal(obs[i, :L], fo[i, :L])         # the rows kept are those of the uncut run
        assert np.array_equal(ctl[i, :L - 1], fc[i, :L - 1]) and np.all(ctl[i, L - 1] == 0.0)
    assert ended > 0


def test_host_fallback_300_states():
    s = system(20, 2)
    koop = Koopman(s, method="lstsq", poly_basis=True, poly_degree=5, trig_basis=True)
    assert koop.state_dim == 300
    koop.train(_training_trajs(s, 71, n=8, L=80))
    arx = ARX(s, history=2)
    arx.train(_training_trajs(s, 72))
    sur = seeded_mlp(s, [32], "tanh", 93)
    task = Task(s)
    task.set_cost(QuadCost(s, np.eye(20), 0.1 * np.eye(2), np.eye(20)))
    task.set_ctrl_bounds(-np.ones(2), np.ones(2))
    task.set_init_obs(np.random.default_rng(1).uniform(-0.3, 0.3, 20))
    task.set_num_steps(8)
    rng = np.random.default_rng(2)
    cands = [{"controller": "lqr", "finite_horizon": True, "horizon": 15, "model": m,
              "Q": 10 ** rng.uniform(-1, 1, 20), "R": 10 ** rng.uniform(-1, 1, 2), "F": 10 ** rng.uniform(-1, 1, 20)}
             for m in (koop, arx)]
    ev = LqrCandidateEvaluator(s, task, surrogate=sur)
    sc = ev.evaluate(cands)
    assert ev.host_fallbacks == 1
    # the host path against a restatement of the reference's controller (lqr.py:35-47, 174-192)
    c = cands[0]
    A, B = koop.to_linear()
    n = A.shape[0]
    Qp, Fp = np.zeros((n, n)), np.zeros((n, n))
    Qp[:20, :20], Fp[:20, :20], R = np.diag(c["Q"]), np.diag(c["F"]), np.diag(c["R"])
    P = Fp
    for _ in range(16):
        P = A.T @ P @ A - (A.T @ P @ B) @ np.linalg.inv(R + B.T @ P @ B) @ (B.T @ P @ A) + Qp
    K = -np.linalg.inv(R + B.T @ P @ B) @ B.T @ P @ A
    x = task.get_init_obs().copy()
    simstate = x.copy()
    obs, ctls = [x.copy()], []
    for _ in range(7):
        u = np.clip(K @ koop._apply_basis(x), -1.0, 1.0)
        simstate = sur.pred(simstate, u)
        x = simstate[:20]
        ctls.append(u)
        obs.append(x.copy())
    ctls.append(np.zeros(2))
    from autompc_amd import Trajectory
    ref = float(task.get_cost()(Trajectory(s, 8, np.array(obs), np.array(ctls))))
    assert abs(sc[0] - ref) <= 1e-10 * abs(ref), (sc[0], ref)
    ref1 = float(task.get_cost()(_dropin(s, task, sur, cands[1])))
    assert abs(sc[1] - ref1) <= 1e-10 * abs(ref1)


def test_tuner_end_to_end():
    s = system(NO, NU)
    trajs = _training_trajs(s, 81, n=8, L=80)
    sur = seeded_mlp(s, [32], "tanh", 95)
    task = Task(s)
    task.set_cost(QuadCost(s, np.eye(NO), 0.1 * np.eye(NU), np.eye(NO), goal=np.zeros(NO)))
    task.set_ctrl_bounds(-np.ones(NU), np.ones(NU))
    task.set_init_obs(np.full(NO, 0.3))
    task.set_num_steps(15)
    ev = LqrCandidateEvaluator(s, task, surrogate=sur)
    tuner = BatchPipelineTuner(s, ev, batch_size=16, model_factory=ARXFactory(s), trajs=trajs, as_configs=True)
    inc, res = tuner.run(32, np.random.default_rng(0))
    assert len(res.costs) == 32 and tuner.models_fitted >= 2
    assert np.isfinite(res.inc_costs[-1]) and res.inc_costs[-1] == min(res.costs)
    assert lqr_candidate_from_config(s, inc)["finite_horizon"]
    cfgs = sample_lqr_pipeline_configs(s, 16, np.random.default_rng(1), model="arx")
    tuner2 = BatchPipelineTuner(s, ev, batch_size=16, model_factory=ARXFactory(s), trajs=trajs)
    inc2, res2 = tuner2.run(16, np.random.default_rng(2), configs=cfgs)
    assert all(a is b for a, b in zip(res2.cfgs, cfgs))
    for c, cost in zip(cfgs, res2.costs):
        if c["_ctrlr:finite_horizon"] == "false":
            assert cost == np.inf
    assert lqr_candidate_from_config(s, inc2)["controller"] == "lqr"
