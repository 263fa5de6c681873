"""Infinite-horizon LQR closed loops on the device (ampc_lqr_plan_set_loop_ex), the drop-in controller under
simulate(), LqrCandidateEvaluator(infinite_horizon="iterate") and the tuner, against the reference's goldens
(tests/golden/gen_golden_lqr_inf.py) and the drop-in.  Needs MI355X."""
import numpy as np
import pytest

from autompc_amd import ARX, ARXFactory, Koopman, QuadCost, Task, simulate, zeros
from autompc_amd import _lib
from autompc_amd.control.lqr import LQR
from autompc_amd.tuning import BatchPipelineTuner, LqrCandidateEvaluator, sample_lqr_pipeline_configs
import lqr_inf_cases as C

pytestmark = pytest.mark.gpu
TRAJ_TOL = 1e-8           # closed loops compound rounding over the episode (test_gpu_lqr.py's bound)
LOOPS = ["arx2", "koop_mlp", "arx4_mlp"]


def _case(name):
    no, nu = dict((n, (o, u)) for n, o, u in C.FIXTURES)[name]
    g = C.gold(name)
    s, m = C.model_of(name, g, no, nu)
    return g, s, m, C.surrogate_of(name, g, s, m)


def _fixture_task(g, s):
    """The fixture's task: a non-zero goal and bounds, neither of which the controller applies."""
    t = Task(s)
    t.set_cost(QuadCost(s, g["Q"], g["R"], np.eye(s.obs_dim), goal=g["goal"]))
    t.set_ctrl_bounds(g["umin"], g["umax"])
    return t


@pytest.mark.parametrize("name", LOOPS)
def test_device_closed_loop_matches_reference(name):
    g, s, m, sur = _case(name)
    no, nu = s.obs_dim, s.ctrl_dim
    hm = _lib.Handle(0, "f64")
    hm.set_linear(*m.to_linear())
    hs = _lib.Handle(0, "f64")
    sur.stage_into(hs)
    plan = _lib.LqrPlan([hm], no, nu)
    _, st, iters = plan.gains_ex([0], g["Q"], g["R"], g["Q"], thresholds=float(g["threshold"]))
    assert st[0] == 0 and iters[0] == int(g["iters"])
    rule = 2 if name == "koop_mlp" else 1
    lifts = [m.device_lift()] if rule == 2 else None
    t0 = zeros(s, 1)
    t0[0].obs[:] = g["init_obs"]
    np.testing.assert_allclose(np.concatenate([m.traj_to_state(t0), np.zeros(nu)]), g["cstate0"], rtol=0, atol=1e-14)
    T = g["obs"].shape[0] - 1
    args = ([m.traj_to_state(t0)], np.asarray(sur.traj_to_state(t0))[None], T)
    plan.set_loop([rule], np.zeros(no), g["umin"], g["umax"], lifts=lifts, clip=[0])
    obs, ctl = plan.closed_loop(hs, *args)
    assert np.abs(obs[0] - g["obs"]).max() / np.abs(g["obs"]).max() < TRAJ_TOL
    assert np.abs(ctl[0] - g["ctrls"]).max() / np.abs(g["ctrls"]).max() < TRAJ_TOL
    if name == "arx2":                 # the bounded task: the flag is really exercised
        assert np.any(np.abs(g["ctrls"]) > g["umax"]) and np.any(np.abs(ctl[0]) > g["umax"])
    # clip = 1 is ampc_lqr_plan_set_loop: the same bits, and on the bounded task another trajectory
    plan.set_loop([rule], g["goal"], g["umin"], g["umax"], lifts=lifts, clip=[1])
    o1, c1 = plan.closed_loop(hs, *args)
    plan.set_loop([rule], g["goal"], g["umin"], g["umax"], lifts=lifts)
    o2, c2 = plan.closed_loop(hs, *args)
    assert np.array_equal(o1, o2) and np.array_equal(c1, c2)
    assert np.all(c1 <= g["umax"]) and np.all(c1 >= g["umin"])
    for obj in (plan, hm, hs):
        obj.close()


@pytest.mark.parametrize("name", LOOPS)
def test_dropin_under_simulate(name):
    g, s, m, sur = _case(name)
    ctl = LQR(s, _fixture_task(g, s), m, "false", infinite_horizon="iterate", threshold=float(g["threshold"]))
    assert ctl.iters == int(g["iters"])
    t0 = zeros(s, 1)
    t0[0].obs[:] = g["init_obs"]
    np.testing.assert_allclose(ctl.traj_to_state(t0), g["cstate0"], rtol=0, atol=1e-14)
    traj = simulate(ctl, g["init_obs"], sim_model=sur, max_steps=g["obs"].shape[0] - 1, silent=True)
    assert np.abs(traj.obs - g["obs"]).max() / np.abs(g["obs"]).max() < TRAJ_TOL
    assert np.abs(traj.ctrls - g["ctrls"]).max() / np.abs(g["ctrls"]).max() < TRAJ_TOL


# ---- the evaluator: 16 candidates, half of them infinite, three models and one that never converges ------------------
NO, NU, STEPS, MAX_ITER = 6, 2, 20, 400


def _training_trajs(s, seed, n=6, L=60):
    """Seeded stable linear system with noise (as gen_golden_lqr.training_trajs)."""
    from autompc_amd import Trajectory
    rng = np.random.default_rng(seed)
    no, nu = s.obs_dim, s.ctrl_dim
    A = 0.9 * np.linalg.qr(rng.normal(size=(no, no)))[0]
    B = 0.3 * rng.normal(size=(no, nu))
    out = []
    for _ in range(n):
        obs, ctl = np.zeros((L, no)), rng.normal(size=(L, nu))
        x = rng.normal(size=no)
        for i in range(L):
            obs[i] = x
            x = A @ x + B @ ctl[i] + 0.01 * rng.normal(size=no)
        out.append(Trajectory(s, L, obs, ctl))
    return out


def _batch():
    s = C.system(NO, NU)
    models = []
    for k in (2, 8):                   # 15 and 63 states
        m = ARX(s, history=k)
        m.train(_training_trajs(s, 40 + k))
        models.append(m)
    koop = Koopman(s, method="lstsq", poly_basis=True, poly_degree=2)
    koop.train(_training_trajs(s, 60, n=8, L=80))
    models.append(koop)
    biased = ARX(s, history=2)         # a bias of 0.3 on every observation: P's corner grows by a constant for ever
    coeffs = models[0].get_parameters()["coeffs"]
    coeffs[:, -(NU + 1)] = 0.3
    biased.set_parameters({"coeffs": coeffs})
    sur = C.seeded_mlp(s, [32], "tanh", 91)
    task = Task(s)
    task.set_cost(QuadCost(s, np.eye(NO), 0.1 * np.eye(NU), 2.0 * np.eye(NO), goal=np.linspace(-0.2, 0.2, NO)))
    task.set_ctrl_bounds(-0.5 * np.ones(NU), 0.5 * np.ones(NU))
    task.set_init_obs(np.random.default_rng(5).uniform(-0.5, 0.5, NO))
    task.set_num_steps(STEPS)
    rng = np.random.default_rng(6)
    cands = []
    for i in range(16):
        c = {"controller": "lqr", "finite_horizon": bool(i % 2), "model": models[i % 3],
             "Q": 10 ** rng.uniform(-1, 1, NO), "R": 10 ** rng.uniform(-1, 1, NU), "F": 10 ** rng.uniform(-1, 1, NO)}
        if c["finite_horizon"]:
            c["horizon"] = int(rng.integers(1, 200))
        cands.append(c)
    cands[14]["model"] = biased        # (an infinite candidate)
    return s, task, sur, cands


def test_evaluator_half_and_half(monkeypatch):
    s, task, sur, cands = _batch()
    calls = {"plans": 0, "gains": 0, "gains_ex": 0, "set_loop": 0, "closed_loop": 0}
    real = _lib.LqrPlan

    class Counting(real):
        def __init__(self, *a, **k):
            calls["plans"] += 1
            super().__init__(*a, **k)

    for name in ("gains", "gains_ex", "set_loop", "closed_loop"):
        def wrap(self, *a, _n=name, **k):
            calls[_n] += 1
            return getattr(real, _n)(self, *a, **k)
        setattr(Counting, name, wrap)
    ev = LqrCandidateEvaluator(s, task, surrogate=sur, infinite_horizon="iterate", inf_max_iter=MAX_ITER)
    monkeypatch.setattr(_lib, "LqrPlan", Counting)
    sc, obs, ctl = ev.evaluate(cands, return_trajectories=True)
    monkeypatch.setattr(_lib, "LqrPlan", real)
    assert calls == {"plans": 1, "gains": 0, "gains_ex": 1, "set_loop": 1, "closed_loop": 1}
    assert ev.host_fallbacks == 0
    inf = np.array([not c["finite_horizon"] for c in cands])
    assert inf.sum() == 8
    # the candidate that cannot converge: inf, status 3, the initial row only, the cap as its count
    assert sc[14] == np.inf and ev.last_status[14] == 3 and ev.last_lengths[14] == 1
    assert ev.last_iterations[14] == MAX_ITER
    ok = np.ones(16, dtype=bool)
    ok[14] = False
    assert np.all(ev.last_status[ok] == 0) and np.all(np.isfinite(sc[ok]))
    unclipped = False
    for i, c in enumerate(cands):
        if c["finite_horizon"]:
            assert ev.last_iterations[i] == c["horizon"] + 1
            continue
        if i == 14:
            continue
        t = Task(s)
        t.set_cost(QuadCost(s, np.diag(c["Q"]), np.diag(c["R"]), np.diag(c["F"]), goal=task.get_cost().get_goal()))
        t.set_ctrl_bounds(task.get_ctrl_bounds()[:, 0], task.get_ctrl_bounds()[:, 1])
        dropin = LQR(s, t, c["model"], "false", infinite_horizon="iterate", max_iter=MAX_ITER)
        assert ev.last_iterations[i] == dropin.iters and 1 < dropin.iters < MAX_ITER
        traj = simulate(dropin, task.get_init_obs(), task.term_cond, sim_model=sur, max_steps=STEPS)
        ref = float(task.get_cost()(traj))
        assert abs(sc[i] - ref) <= 1e-10 * abs(ref), (i, sc[i], ref)
        assert ev.last_lengths[i] == len(traj)
        assert np.abs(obs[i, :len(traj)] - traj.obs).max() / np.abs(traj.obs).max() < TRAJ_TOL
        unclipped = unclipped or bool(np.any(np.abs(ctl[i, :len(traj)]) > 0.5))
    assert unclipped                   # some infinite candidate left the bounds the finite ones are clipped to
    assert np.all(np.abs(ctl[~inf, :STEPS]) <= 0.5)
    # the same batch under "refuse": the finite candidates' scores and rows do not move by a bit
    ev0 = LqrCandidateEvaluator(s, task, surrogate=sur)
    sc0, obs0, ctl0 = ev0.evaluate(cands, return_trajectories=True)
    assert np.all(sc0[inf] == np.inf) and np.all(ev0.last_status[inf] == 2) and np.all(ev0.last_iterations[inf] == 0)
    assert np.array_equal(sc0[~inf], sc[~inf])
    assert np.array_equal(obs0[~inf], obs[~inf]) and np.array_equal(ctl0[~inf], ctl[~inf])


def test_tuner_scores_infinite_configurations():
    s = C.system(NO, NU)
    trajs = _training_trajs(s, 81, n=8, L=80)
    sur = C.seeded_mlp(s, [32], "tanh", 95)
    task = Task(s)
    task.set_cost(QuadCost(s, np.eye(NO), 0.1 * np.eye(NU), np.eye(NO), goal=np.zeros(NO)))
    task.set_ctrl_bounds(-np.ones(NU), np.ones(NU))
    task.set_init_obs(np.full(NO, 0.3))
    task.set_num_steps(15)
    cfgs = sample_lqr_pipeline_configs(s, 32, np.random.default_rng(1), model="arx")
    false = np.array([c["_ctrlr:finite_horizon"] == "false" for c in cfgs])
    assert 8 <= false.sum() <= 24
    costs = {}
    for mode in ("refuse", "iterate"):
        ev = LqrCandidateEvaluator(s, task, surrogate=sur, infinite_horizon=mode, inf_max_iter=MAX_ITER)
        tuner = BatchPipelineTuner(s, ev, batch_size=16, model_factory=ARXFactory(s), trajs=trajs)
        inc, res = tuner.run(32, np.random.default_rng(2), configs=cfgs)
        costs[mode] = np.array(res.costs)
        assert res.inc_costs[-1] == costs[mode].min()
    assert np.all(costs["refuse"][false] == np.inf)
    assert np.isfinite(costs["iterate"][false]).sum() >= 1
    assert np.array_equal(costs["refuse"][~false], costs["iterate"][~false])
    # truedyn_score builds the drop-in with the evaluator's setting
    from autompc_amd.tuning import lqr_candidate_from_config
    i = int(np.nonzero(false & np.isfinite(costs["iterate"]))[0][0])
    cand = lqr_candidate_from_config(s, cfgs[i])
    tuner.fit_models([cand])
    A, B = 0.9 * np.eye(NO), 0.1 * np.ones((NO, NU))
    dyn = lambda x, u: A @ x + B @ u                      # noqa: E731
    assert np.isfinite(tuner.truedyn_score(cand, dyn))
    ev0 = LqrCandidateEvaluator(s, task, surrogate=sur)
    tuner0 = BatchPipelineTuner(s, ev0, batch_size=16, model_factory=ARXFactory(s), trajs=trajs)
    assert tuner0.truedyn_score(cand, dyn) == np.inf
