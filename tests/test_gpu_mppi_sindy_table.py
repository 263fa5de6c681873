"""MPPI candidates on SINDy models of mixed feature libraries in ONE plan (ampc_mppi_plan_set_sindy_models,
csrc/mppi_sindy_table_kernels.hpp; ``CandidateEvaluator(sindy_models="table")``): bit for bit against single-model plans
on the same model (the existing rollout kernels under AMPC_SINDY_G=16), against itself alone / reversed, against the
oracle, and through the evaluator and the tuner.  Plans, models and noise: tests/mppi_sindy_table_cases.py.
Needs MI355X.

A horizon of 1 is not among the problems: ampc_mppi_plan_create has always refused it (the shifted warm start
a[-1] = a[-2] needs two rows); test_one_solve_* checks that it still does, for a plan that would take the table too."""
import functools

import numpy as np
import pytest

import mppi_sindy_table_cases as C
from helpers import rel_err

pytestmark = pytest.mark.gpu


def _solve(name, which, model=None, precision="f64", indicator=False, cap=C.HORIZON_CAP, reuse=None):
    """One solve of a plan over the problems `which` of the set's plan data: on the set's table of models
    (model=None), or all of them on models[model] staged into the plan's handle (the single-model kernels).  Returns per
    problem (costs [N], clipped noise [H][N][nu], updated sequence [H][nu], control [nu])."""
    from autompc_amd import _lib
    system, ms, _, _ = C.models(name, precision)
    d = C.plan_data(name)
    nu = system.ctrl_dim
    which = np.asarray(which)
    idx = d["index"][which]
    h = _lib.Handle(0, precision)
    try:
        ms[int(idx[0]) if model is None else model].stage_into(h)
        h.set_quad_costs(d["Q"], d["R"], d["F"], d["goal"])
        if indicator:
            h.set_indicator_costs(C.indicator_terms(name))
        h.set_ctrl_bounds(np.full(nu, C.LO), np.full(nu, C.HI))
        n = len(which)
        plan = _lib.MppiPlan(h, d["N"][which], d["H"][which], [C.SIGMA] * n, [C.LMDA] * n, cost_index=which)
        plan.set_geometry(0, cap)
        plan.set_noise_ids(which)
        if model is None:
            plan.set_sindy_models([m._dev() for m in ms], idx)
        plan.upload(x0=d["x0"][which], act_seq=np.concatenate([d["act"][b].ravel() for b in which]),
                    eps=np.concatenate([d["eps"][b].ravel() for b in which]))
        plan.solve()
        if reuse is not None:
            reuse(plan)
        a, u, c, e = plan.download(act_seq=True, u=True, costs=True, eps_out=True)
        plan.close()
    finally:
        h.close()
    out, ao, co, eo = [], 0, 0, 0
    for k, b in enumerate(which):
        N, H = int(d["N"][b]), int(d["H"][b])
        out.append((c[co:co + N].copy(), e[eo:eo + N * H * nu].reshape(H, N, nu).copy(),
                    a[ao:ao + H * nu].reshape(H, nu).copy(), u[k].copy()))
        ao, co, eo = ao + H * nu, co + N, eo + N * H * nu
    return out


def _same(got, ref, what):
    for k, (x, y) in enumerate(zip(got, ref)):
        assert np.all(np.isfinite(y)), what
        np.testing.assert_array_equal(x, y, err_msg="%s, output %d" % (what, k))


def _against_single_model_plans(name, precision="f64", indicator=False):
    d = C.plan_data(name)
    B = len(C.N_LIST)
    table = _solve(name, np.arange(B), precision=precision, indicator=indicator)
    for k in range(len(C.SETS[name]["tags"])):
        which = np.nonzero(d["index"] == k)[0]
        single = _solve(name, which, model=k, precision=precision, indicator=indicator)
        for j, b in enumerate(which):
            _same(table[b], single[j], "%s %s, problem %d (N %d, H %d) on model %d"
                  % (name, precision, b, d["N"][b], d["H"][b], k))
    return table


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["trio", "pair", "c1"])
def test_one_solve_is_the_single_model_plans_bit_for_bit(name, monkeypatch):
    """Seven problems (1 .. 130 samples, horizons 2 .. the cap) on a non-monotonic model index in one plan: costs,
    clipped noise, updated sequences and controls of every problem are the bits of a single-model plan on its model
    (same geometry, noise ids and cost block) under AMPC_SINDY_G=16."""
    from autompc_amd import _lib
    monkeypatch.setenv("AMPC_SINDY_G", "16")
    _against_single_model_plans(name)
    system, ms, _, _ = C.models(name)
    h = _lib.Handle(0, "f64")
    ms[0].stage_into(h)
    h.set_quad_costs(*(C.plan_data(name)[k] for k in ("Q", "R", "F", "goal")))
    h.set_ctrl_bounds(np.full(system.ctrl_dim, C.LO), np.full(system.ctrl_dim, C.HI))
    with pytest.raises(_lib.AmpcError, match="horizon>=2"):
        _lib.MppiPlan(h, [4], [1], [C.SIGMA], [C.LMDA])
    h.close()


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["trio", "pair", "c1"])
def test_a_problem_is_the_same_bits_alone_in_the_batch_and_reversed(name):
    B = len(C.N_LIST)
    batch = _solve(name, np.arange(B))
    rev = _solve(name, np.arange(B)[::-1])
    for b in range(B):
        _same(rev[B - 1 - b], batch[b], "%s reversed, problem %d" % (name, b))
        _same(_solve(name, [b])[0], batch[b], "%s alone, problem %d" % (name, b))


# 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp", ["1", "0"])
def test_indicator_terms(fp, monkeypatch):
    """Threshold and box terms on the handle; the trio holds lane-spread entries and a one-thread entry.
    AMPC_SINDY_FP=0 sends every entry to the one-thread body, like the single-model plans under the same setting."""
    monkeypatch.setenv("AMPC_SINDY_G", "16")
    monkeypatch.setenv("AMPC_SINDY_FP", fp)
    with_terms = _against_single_model_plans("trio", indicator=True)
    without = _solve("trio", np.arange(len(C.N_LIST)))
    charged = [float(np.max(a[0] - b[0])) for a, b in zip(with_terms, without)]
    print("indicator terms, AMPC_SINDY_FP=%s: largest charge per problem %s" % (fp, np.round(charged, 3)))
    assert max(charged) >= 1.0                                           # the terms are charged somewhere


# 4 ---------------------------------------------------------------------------------------------------------------
def test_f32(monkeypatch):
    monkeypatch.setenv("AMPC_SINDY_G", "16")
    _against_single_model_plans("trio", precision="f32")


# 5 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["trio", "pair", "c1"])
def test_costs_match_the_oracle(name):
    """1e-10 on the costs, 1e-9 on the updated sequence: the bounds tests/test_gpu_sindy.py holds the single-model
    kernels to."""
    got = _solve(name, np.arange(len(C.N_LIST)))
    for b, ((costs, eps, act, _), (o_costs, o_eps, o_act)) in enumerate(zip(got, C.cpu_rollouts(name))):
        errs = rel_err(costs, o_costs), rel_err(eps, o_eps), rel_err(act, o_act)
        print("%s problem %d vs oracle: costs %.2e clipped noise %.2e sequence %.2e" % ((name, b) + errs))
        assert errs[0] < 1e-10 and errs[1] < 1e-12 and errs[2] < 1e-9


# 6, 7 ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _five():
    """Five models of the trio's system (the trio and two synthetic libraries), six candidates (one model shared,
    horizons and sample counts differ), a SINDy and an MLP surrogate."""
    from autompc_amd import MLP, QuadCost, Task
    system, trio, _, obs = C.models("trio")
    nx, nu = system.obs_dim, system.ctrl_dim
    ms = list(trio) + [C._synthetic(system, kind, "f64")[0] for kind in ("identity", "poly2")]
    rng = np.random.default_rng(41)
    task = Task(system)
    task.set_cost(QuadCost(system, np.eye(nx), 0.05 * np.eye(nu), 2.0 * np.eye(nx)))
    task.set_ctrl_bounds(np.full(nu, C.LO), np.full(nu, C.HI))
    task.set_init_obs(0.5 * obs[3])
    task.set_num_steps(6)
    cands = [dict(horizon=h, sigma=0.05, lmda=0.6, num_path=n, Q=rng.uniform(0.5, 2.0, nx), R=rng.uniform(0.01, 0.1, nu),
                  F=rng.uniform(0.5, 2.0, nx), model=ms[k])
             for h, n, k in ((8, 65, 2), (2, 4, 0), (5, 130, 4), (3, 63, 1), (8, 5, 2), (6, 64, 3))]
    mlp = MLP(system, n_hidden_layers=1, hidden_size_1=16, nonlintype="tanh")
    mlp.weights = [rng.normal(scale=0.2, size=(16, nx + nu)), rng.normal(scale=0.2, size=(nx, 16))]
    mlp.biases = [rng.normal(scale=0.05, size=16), rng.normal(scale=0.01, size=nx)]
    mlp.xu_means, mlp.xu_std = np.zeros(nx + nu), np.ones(nx + nu)
    mlp.dy_means, mlp.dy_std = np.zeros(nx), 0.1 * np.ones(nx)
    return system, task, ms, cands, {"sindy": ms[3], "mlp": mlp}


@pytest.mark.parametrize("surrogate", ["sindy", "mlp"])
def test_evaluator_scores_a_mixed_batch_in_one_plan(surrogate, monkeypatch):
    from autompc_amd import _lib
    from autompc_amd.tuning import CandidateEvaluator
    monkeypatch.setenv("AMPC_SINDY_G", "16")
    system, task, ms, cands, surs = _five()
    sur = surs[surrogate]
    kw = dict(surrogate=sur, horizon_cap=C.HORIZON_CAP)
    ev = CandidateEvaluator(system, task, ms[0], sindy_models="table", **kw)
    scores, obs, ctl = ev.evaluate(cands, n_steps=5, seed=3, return_trajectories=True)
    assert ev.last_models == {"path": "sindy_table", "models": 5, "plans": 1}
    assert np.all(np.isfinite(scores)) and np.all(np.isfinite(obs)) and obs.shape == (6, 6, system.obs_dim)
    for i, c in enumerate(cands):
        alone = CandidateEvaluator(system, task, c["model"], **kw)
        s1, o1, c1 = alone.evaluate([{k: v for k, v in c.items() if k != "model"}], n_steps=5, seed=3,
                                    return_trajectories=True, index_offset=i)
        np.testing.assert_array_equal(scores[i], s1[0])
        np.testing.assert_array_equal(obs[i], o1[0])
        np.testing.assert_array_equal(ctl[i], c1[0])
    # the default is today's behaviour: the library refuses a SINDy model per problem
    with pytest.raises(_lib.AmpcError, match="per-problem models are MLP models"):
        CandidateEvaluator(system, task, ms[0], **kw).evaluate(cands, n_steps=5, seed=3)


def test_tuner_fits_and_scores_a_batch_of_sindy_configurations():
    from autompc_amd import Trajectory
    from autompc_amd.sysid.sindy import SINDyFactory
    from autompc_amd.tuning import BatchPipelineTuner, CandidateEvaluator, random_candidates
    system, task, ms, _, _ = _five()
    nx, nu = system.obs_dim, system.ctrl_dim
    rng = np.random.default_rng(5)
    A = 0.9 * np.eye(nx) + 0.05 * rng.normal(size=(nx, nx))
    Bm = 0.1 * rng.normal(size=(nx, nu))
    trajs = []
    for _ in range(12):
        o, u = np.zeros((40, nx)), rng.uniform(-0.6, 0.8, size=(40, nu))
        x = rng.uniform(-0.4, 0.4, size=nx)
        for t in range(40):
            o[t] = x
            x = A @ x + Bm @ u[t] + 0.02 * np.sin(x[::-1])
        trajs.append(Trajectory(system, 40, o, u))
    libraries = [dict(time_mode="discrete", threshold=1e-3),
                 dict(time_mode="continuous", threshold=1e-3, trig_basis=True, trig_freq=1, trig_interaction=True),
                 dict(time_mode="discrete", threshold=1e-3, poly_basis=True, poly_degree=3, poly_cross_terms=True),
                 dict(time_mode="discrete", threshold=1e-2, poly_basis=True, poly_degree=2)]

    def sampler(n, rng):
        out = random_candidates(system, n, seed=7)
        for i, c in enumerate(out):
            c.update(horizon=min(c["horizon"], C.HORIZON_CAP), sigma=0.05, num_path=c["num_path"] // 8,
                     Q=np.ones(nx), R=0.05 * np.ones(nu), F=np.ones(nx), model_cfg=dict(libraries[i % 4]))
        return out
    ev = CandidateEvaluator(system, task, ms[3], sindy_models="table", horizon_cap=C.HORIZON_CAP)
    tuner = BatchPipelineTuner(system, ev, batch_size=6, sampler=sampler, model_factory=SINDyFactory(system), trajs=trajs,
                               sindy_fit="device")
    inc, res = tuner.run(6, np.random.default_rng(0), seed=2)
    assert ev.last_models == {"path": "sindy_table", "models": 4, "plans": 1}
    assert tuner.models_fitted == 4 and len(res.costs) == 6 and np.all(np.isfinite(res.costs))
    assert len({type(c["model"]).__name__ for c in res.cfgs}) == 1 and len({id(c["model"]) for c in res.cfgs}) == 4
    assert len({c["model"].coefficients.shape for c in res.cfgs}) >= 3                 # three libraries at least
    k = int(np.argmin(res.costs))
    assert res.inc_cfg is res.cfgs[k] and res.inc_costs[-1] == res.costs[k]
    one = ev.evaluate([res.cfgs[k]], seed=2, index_offset=k)
    assert ev.last_models == {"path": "sindy_table", "models": 1, "plans": 1}
    np.testing.assert_array_equal(one[0], res.costs[k])


# 8 ---------------------------------------------------------------------------------------------------------------
def _trio_plan(precision="f64", cap=C.HORIZON_CAP):
    from autompc_amd import _lib
    system, ms, _, _ = C.models("trio", precision)
    d = C.plan_data("trio")
    nu = system.ctrl_dim
    h = _lib.Handle(0, precision)
    ms[0].stage_into(h)
    h.set_quad_costs(d["Q"], d["R"], d["F"], d["goal"])
    h.set_ctrl_bounds(np.full(nu, C.LO), np.full(nu, C.HI))
    plan = _lib.MppiPlan(h, [5, 64], [3, 8], [C.SIGMA] * 2, [C.LMDA] * 2, cost_index=[0, 1])
    plan.set_geometry(0, cap)
    return h, plan, ms


def test_refusals():
    from autompc_amd import MLP, _lib
    h, plan, ms = _trio_plan()
    handles = [m._dev() for m in ms]
    who = "ampc_mppi_plan_set_sindy_models"

    def refused(match, hs, index=(0, 1), p=plan, code=-1):
        with pytest.raises(_lib.AmpcError, match=match) as e:
            p.set_sindy_models(hs, index)
        assert who in str(e.value) and e.value.code == code
    # a model handle without a SINDy model / without any model
    system = C.models("trio")[0]
    mlp = MLP(system, n_hidden_layers=1, hidden_size_1=16)
    hm = _lib.Handle(0, "f64", jit=False)
    mlp.stage_into(hm)
    refused("model handle holds no SINDy model", [handles[0], hm])
    refused("model handle holds no SINDy model", [handles[0], _lib.Handle(0, "f64")])
    # a plan handle without one
    hm.set_quad_costs(np.eye(3), np.eye(2), np.eye(3), np.zeros(3))
    hm.set_ctrl_bounds(-np.ones(2), np.ones(2))
    refused("plan handle's model is not a SINDy model", handles[:2], p=_lib.MppiPlan(hm, [5, 64], [3, 8], [0.1] * 2, [1.0] * 2))
    # other dimensions, another precision
    refused("state and control dimensions", [handles[0], C.models("c1")[1][0]._dev()])
    refused("device and precision", [handles[0], C.models("trio", "f32")[1][1]._dev()])
    # a model_index out of range
    refused("model_index out of range", handles, index=(0, 3))
    refused("model_index out of range", handles, index=(-1, 0))
    # a state lift on the plan: nx = 3 observations, one basis function
    plan.set_state_lift(np.array([0], dtype=np.int32), np.array([0.0]))
    refused("state lift", handles)
    plan.set_state_lift([], [])
    # the table and the other two per-problem model calls exclude each other
    plan.set_sindy_models(handles, (2, 0))
    with pytest.raises(_lib.AmpcError, match="ampc_mppi_plan_set_models.*table of SINDy models"):
        plan.set_models(handles, (0, 1))
    with pytest.raises(_lib.AmpcError, match="ampc_mppi_plan_set_model_table.*table of SINDy models"):
        plan.set_model_table([mlp, mlp], (0, 1))
    # ... and a lift set afterwards is refused at solve time
    plan.set_state_lift(np.array([0], dtype=np.int32), np.array([0.0]))
    with pytest.raises(_lib.AmpcError, match="ampc_mppi_solve.*state lift"):
        plan.solve()
    plan.close()
    h.close()
    hm.close()


def test_removing_the_table_restores_the_plans_own_model(monkeypatch):
    monkeypatch.setenv("AMPC_SINDY_G", "16")
    d = C.plan_data("trio")
    which = np.array([3, 6])                                             # (63 and 130 samples; table entries 0 and 1)
    k0 = int(d["index"][which[0]])
    own = _solve("trio", which, model=k0)

    def remove_and_solve_again(plan):
        plan.set_sindy_models(None, None)
        plan.upload(act_seq=np.concatenate([d["act"][b].ravel() for b in which]))
        plan.solve()
    back = _solve("trio", which, reuse=remove_and_solve_again)           # (its handle holds models[index[which[0]]])
    for j in range(2):
        _same(back[j], own[j], "table removed, problem %d" % which[j])


def test_a_declined_table_runs_one_plan_per_model(monkeypatch):
    """Return code -3 (an entry's LDS need exceeds 160 KB).  No model of the cases reaches the limit at any horizon cap:
    an entry that does not fit the lane-spread body takes the one-thread body, whose need does not grow with the
    horizon (the largest here, hc_trig: 87 columns of 64 samples and a 10 KB program, 55 KB).  So the refusal is put in
    the binding's place.  The evaluator then gives every model a plan of its own: the same scores."""
    from autompc_amd import _lib
    from autompc_amd.tuning import CandidateEvaluator
    monkeypatch.setenv("AMPC_SINDY_G", "16")
    system, task, ms, cands, surs = _five()
    ev = CandidateEvaluator(system, task, ms[0], surrogate=surs["sindy"], sindy_models="table",
                            horizon_cap=C.HORIZON_CAP)
    want = ev.evaluate(cands, n_steps=5, seed=3)
    assert ev.last_models["path"] == "sindy_table"
    real = _lib.MppiPlan.set_sindy_models

    def declined(self, handles, model_index):
        if handles:
            err = _lib.AmpcError("ampc_mppi_plan_set_sindy_models: declined by the test")
            err.code = _lib.MPPI_TABLE_NO_FIT
            raise err
        real(self, handles, model_index)
    monkeypatch.setattr(_lib.MppiPlan, "set_sindy_models", declined)
    got = ev.evaluate(cands, n_steps=5, seed=3)
    assert ev.last_models == {"path": "model", "models": 5, "plans": 5}
    np.testing.assert_array_equal(got, want)
