"""MPPI candidates on linear models (ARX / Koopman) of mixed state dimension in ONE plan
(ampc_mppi_plan_set_linear_models / ampc_mppi_closed_loop_linear, csrc/mppi_linear_table_kernels.hpp;
``CandidateEvaluator(linear_models="table")``): bit for bit against single-model plans on linear_rollout_kernel
(models staged under AMPC_LINEAR_WIDE=1), against itself alone / reversed, against the oracle, the closed loop against
simulate()'s own loop on the host, the refusals, and through the evaluator and the tuner.  Plans, models and noise:
tests/mppi_linear_table_cases.py.  Needs MI355X."""
import functools

import numpy as np
import pytest

import mppi_linear_table_cases as C
from helpers import make_system, rel_err

pytestmark = pytest.mark.gpu


def _handle(name, A, B, precision, indicator, wide):
    """A handle holding (A, B) with the set's cost blocks and bounds; wide: staged for the K-tiled linear kernels
    whatever its size (AMPC_LINEAR_WIDE=1), else the way ampc_set_linear picks by itself."""
    from autompc_amd import _lib
    d = C.plan_data(name)
    h = _lib.Handle(0, precision)
    with pytest.MonkeyPatch.context() as mp:
        if wide:
            mp.setenv("AMPC_LINEAR_WIDE", "1")
        else:
            mp.delenv("AMPC_LINEAR_WIDE", raising=False)
        h.set_linear(A, B)
    h.set_quad_costs(d["Q"], d["R"], d["F"], d["goal"])
    if indicator:
        h.set_indicator_costs(C.indicator_terms(name))
    h.set_ctrl_bounds(np.full(B.shape[1], C.LO), np.full(B.shape[1], C.HI))
    return h


def _solve(name, which, model=None, precision="f64", indicator=False, cap=C.HORIZON_CAP, after=None):
    """One solve of a plan over the problems `which` of the set's plan data: on the set's table of models
    (model=None), or all of them on model `model` staged into the plan's handle (linear_rollout_kernel).  Returns per
    problem (costs [N], clipped noise [H][N][nu], updated sequence [H][nu], control [nu])."""
    from autompc_amd import _lib
    system, ab = C.matrices(name)
    d = C.plan_data(name)
    nu = system.ctrl_dim
    which = np.asarray(which)
    idx = d["index"][which]
    opened = []
    try:
        k0 = int(idx[0]) if model is None else model
        h = _handle(name, *ab[k0], precision, indicator, wide=model is not None)
        opened.append(h)
        n = len(which)
        plan = _lib.MppiPlan(h, d["N"][which], d["H"][which], [C.SIGMA] * n, [C.LMDA] * n, cost_index=which)
        opened.append(plan)
        plan.set_geometry(0, cap)
        plan.set_noise_ids(which)
        if model is None:
            # the table's handles in either staging form: every other one wide
            hs = [_handle(name, A, B, precision, False, wide=bool(k % 2)) for k, (A, B) in enumerate(ab)]
            opened.extend(hs)
            plan.set_linear_models(hs, idx)
            assert plan.linear_x0_sizes.tolist() == [C.SETS[name]["nx"][int(k)] for k in idx]
        plan.upload(x0=np.concatenate([d["x0"][b] for b in which]),
                    act_seq=np.concatenate([d["act"][b].ravel() for b in which]),
                    eps=np.concatenate([d["eps"][b].ravel() for b in which]))
        plan.solve()
        a, u, c, e = plan.download(act_seq=True, u=True, costs=True, eps_out=True)
        if after is not None:
            after(plan, opened)
    finally:
        for o in reversed(opened):
            o.close()
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
    for k in sorted(set(d["index"].tolist())):
        which = np.nonzero(d["index"] == k)[0]
        single = _solve(name, which, model=k, precision=precision, indicator=indicator)
        for j, b in enumerate(which):
            _same(table[b], single[j], "%s %s, problem %d (N %d, H %d) on model %d (nx %d)"
                  % (name, precision, b, d["N"][b], d["H"][b], k, C.SETS[name]["nx"][k]))
    return table


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precision", [("edges", "f64"), ("wide", "f64"), ("k4", "f64"), ("nu6", "f64"),
                                            ("edges", "f32")])
def test_one_solve_is_the_single_model_plans_bit_for_bit(name, precision):
    """Seven problems (1 .. 130 samples, horizons 2 .. the cap) on a non-monotonic model index in one plan: costs,
    clipped noise, updated sequences and controls of every problem are the bits of a single-model plan on its model
    (linear_rollout_kernel: staged under AMPC_LINEAR_WIDE=1; same horizon cap, noise ids and cost block)."""
    _against_single_model_plans(name, precision)


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["edges", "wide"])
def test_a_problem_is_the_same_bits_alone_in_the_batch_and_reversed(name):
    B = len(C.N_LIST)
    batch = _solve(name, np.arange(B))
    rev = _solve(name, np.arange(B)[::-1])
    for b in range(B):
        _same(rev[B - 1 - b], batch[b], "%s reversed, problem %d" % (name, b))
        _same(_solve(name, [b])[0], batch[b], "%s alone, problem %d" % (name, b))


# 3 ---------------------------------------------------------------------------------------------------------------
def test_indicator_terms():
    """Threshold and box terms on the plan handle: bit for bit the single-model plans, and charged somewhere."""
    with_terms = _against_single_model_plans("edges", indicator=True)
    without = _solve("edges", np.arange(len(C.N_LIST)))
    charged = [float(np.max(a[0] - b[0])) for a, b in zip(with_terms, without)]
    print("indicator terms: largest charge per problem %s" % np.round(charged, 3))
    assert max(charged) >= 1.0


# 4 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.SETS))
def test_costs_match_the_oracle(name):
    """The bounds tests/test_linear_wide.py::test_wide_linear_mppi_vs_oracle holds linear_rollout_kernel to in f64: 1e-9
    on the costs, 1e-8 on the updated sequence and the control."""
    got = _solve(name, np.arange(len(C.N_LIST)))
    for b, ((costs, eps, act, u), (o_costs, o_eps, o_act)) in enumerate(zip(got, C.cpu_rollouts(name))):
        errs = rel_err(costs, o_costs), rel_err(eps, o_eps), rel_err(act, o_act), rel_err(u, o_act[0] * C.HI)
        print("%s problem %d vs oracle: costs %.2e clipped noise %.2e sequence %.2e control %.2e" % ((name, b) + errs))
        assert errs[0] < 1e-9 and errs[1] < 1e-9 and errs[2] < 1e-8 and errs[3] < 1e-8


# 5 ---------------------------------------------------------------------------------------------------------------
T = 8


@functools.lru_cache(maxsize=None)
def _loop():
    """Six trained controller models on one system (ARX of history 1, 2, 4; Koopman with the identity only, a degree-3
    polynomial and a trig basis), an MLP surrogate, seven candidates in non-monotonic model order (one model twice),
    recorded noise and warm starts for T control steps."""
    from autompc_amd import ARX, MLP, Koopman, QuadCost, Task
    from kstep_mlp_cases import synthetic_trajs
    system = make_system(3, 2)
    no, nu = 3, 2
    trajs = synthetic_trajs(system, seed=5)
    ms = [ARX(system, history=1), ARX(system, history=2), ARX(system, history=4), Koopman(system),
          Koopman(system, poly_basis="true", poly_degree=3), Koopman(system, trig_basis="true", trig_freq=2, strict_reference=False)]
    for m in ms:
        m.train(trajs, silent=True)
    assert [m.state_dim for m in ms] == [4, 9, 19, 3, 9, 15]
    rng = np.random.default_rng(41)
    mlp = MLP(system, n_hidden_layers=1, hidden_size_1=16, nonlintype="tanh")
    mlp.weights = [rng.normal(scale=0.2, size=(16, no + nu)), rng.normal(scale=0.2, size=(no, 16))]
    mlp.biases = [rng.normal(scale=0.05, size=16), rng.normal(scale=0.01, size=no)]
    mlp.xu_means, mlp.xu_std = np.zeros(no + nu), np.ones(no + nu)
    mlp.dy_means, mlp.dy_std = np.zeros(no), 0.1 * np.ones(no)
    task = Task(system)
    task.set_cost(QuadCost(system, np.eye(no), 0.05 * np.eye(nu), 2.0 * np.eye(no), goal=np.array([0.05, -0.02, 0.0])))
    task.set_ctrl_bounds(-np.ones(nu), np.ones(nu))
    task.set_init_obs(np.array([0.1, -0.05, 0.02]))
    task.set_num_steps(T + 1)
    cands = [dict(horizon=h, sigma=0.3, lmda=0.6, num_path=n, Q=rng.uniform(0.5, 2.0, no), R=rng.uniform(0.01, 0.1, nu),
                  F=rng.uniform(0.5, 2.0, no), model=ms[k])
             for h, n, k in ((8, 33, 4), (2, 4, 0), (5, 40, 5), (3, 17, 2), (8, 5, 1), (6, 16, 3), (4, 20, 4))]
    eps = [[rng.normal(scale=np.sqrt(c["sigma"]), size=(c["num_path"], c["horizon"], nu)) for c in cands]
           for _ in range(T)]
    acts = [rng.normal(scale=np.sqrt(c["sigma"]), size=(c["horizon"], nu)) for c in cands]
    return system, task, ms, mlp, cands, eps, acts


def _flat_eps(eps, which):
    return np.concatenate([np.concatenate([eps[s][i].ravel() for i in which]) for s in range(len(eps))])


def _host_loop(i):
    """simulate() (utils/simulation.py:44-63) for candidate i: the model's own update_state, the oracle's MPPI solve
    with the step's noise, surrogate.pred."""
    from autompc_amd import Trajectory
    from autompc_amd.tuning.batch_eval import score_trajectories
    from oracle.costs import QuadCostOracle
    from oracle.mppi import MPPIOracle
    system, task, _, mlp, cands, eps, acts = _loop()
    c = cands[i]
    m = c["model"]
    no, nu = system.obs_dim, system.ctrl_dim
    goal = task.get_cost().get_goal()
    np.random.seed(0)
    orc = MPPIOracle(C.LinearOracle(system, m.A, m.B), QuadCostOracle(np.diag(c["Q"]), np.diag(c["R"]), np.diag(c["F"]), goal),
                     np.tile([-1.0, 1.0], (nu, 1)), horizon=c["horizon"], num_path=c["num_path"], sigma=c["sigma"],
                     lmda=c["lmda"])
    orc.act_sequence = acts[i].copy()
    sim = np.asarray(task.get_init_obs(), dtype=np.float64)
    state = m.traj_to_state(Trajectory(system, 1, sim[None, :].copy(), np.zeros((1, nu))))
    u = np.zeros(nu)
    obs, ctl = [sim.copy()], []
    for s in range(T):
        state = m.update_state(state, u, sim[:no])
        costs, e = orc.do_rollouts(state, eps[s][i])
        orc.update(costs, e)
        u = orc.act_sequence[0] * orc.ctrl_scale
        sim = mlp.pred(sim, u)
        obs.append(sim.copy())
        ctl.append(u.copy())
    ctl.append(np.zeros(nu))
    obs, ctl = np.array(obs), np.array(ctl)
    return obs, ctl, score_trajectories(task.get_cost(), obs[None], ctl[None])[0]


def test_closed_loop_is_simulate_with_every_models_own_update_state():
    """1e-8 on the rows, 1e-7 relative on the score: the bounds tests/test_linear_wide.py holds the evaluator to against
    simulate()."""
    from autompc_amd.tuning import CandidateEvaluator
    system, task, ms, mlp, cands, eps, acts = _loop()
    B = len(cands)
    kw = dict(surrogate=mlp, horizon_cap=C.HORIZON_CAP, linear_models="table")
    ev = CandidateEvaluator(system, task, ms[0], **kw)
    scores, obs, ctl = ev.evaluate(cands, eps_all=_flat_eps(eps, range(B)), act_init=np.concatenate([a.ravel() for a in acts]),
                                   return_trajectories=True)
    assert ev.last_models == {"path": "linear_table", "models": 6, "plans": 1}
    assert obs.shape == (B, T + 1, mlp.state_dim) and ctl.shape == (B, T + 1, 2)
    for i in range(B):
        o, c, s = _host_loop(i)
        eo, ec, es = float(np.max(np.abs(obs[i] - o))), float(np.max(np.abs(ctl[i] - c))), abs(scores[i] - s) / abs(s)
        print("candidate %d (%s, %d states): rows %.2e controls %.2e score %.2e"
              % (i, type(cands[i]["model"]).__name__, cands[i]["model"].state_dim, eo, ec, es))
        assert eo < 1e-8 and ec < 1e-8 and es < 1e-7
    for i, c in enumerate(cands):
        # alone in a table of one entry: the same bits
        one = CandidateEvaluator(system, task, c["model"], **kw)
        s1 = one.evaluate([c], eps_all=_flat_eps(eps, [i]), act_init=acts[i].ravel(), index_offset=i)
        assert one.last_models == {"path": "linear_table", "models": 1, "plans": 1}
        np.testing.assert_array_equal(s1[0], scores[i])
        # a Koopman candidate on the existing single-lift evaluator: the same bits, when its plan handle is staged for
        # linear_rollout_kernel (AMPC_LINEAR_WIDE=1; at these sizes ampc_set_linear would otherwise stage an identity
        # network for the MLP tile, another summation order)
        if hasattr(c["model"], "device_lift"):
            old = CandidateEvaluator(system, task, c["model"], surrogate=mlp, horizon_cap=C.HORIZON_CAP, tile_rows=16)
            with pytest.MonkeyPatch.context() as mp:
                mp.setenv("AMPC_LINEAR_WIDE", "1")
                s0 = old.evaluate([{k: v for k, v in c.items() if k != "model"}], eps_all=_flat_eps(eps, [i]),
                                  act_init=acts[i].ravel(), index_offset=i)
            np.testing.assert_array_equal(s0[0], scores[i])
    # an episode in segments (a termination condition that never fires) continues on the device: the same bits
    # (with a user condition the episode runs num_steps control steps: batch_eval.episode_of)
    import copy
    task2 = copy.copy(task)
    task2.set_num_steps(T)
    task2.set_term_cond(lambda traj: False)
    seg = CandidateEvaluator(system, task2, ms[0], term_check_every=3, **kw)
    s2, o2, c2 = seg.evaluate(cands, eps_all=_flat_eps(eps, range(B)), act_init=np.concatenate([a.ravel() for a in acts]),
                              return_trajectories=True)
    assert seg.last_models["path"] == "linear_table"
    np.testing.assert_array_equal(s2, scores)
    np.testing.assert_array_equal(o2, obs)
    np.testing.assert_array_equal(c2, ctl)
    # Philox noise: a candidate's score does not depend on the batch it is in
    both = ev.evaluate(cands, seed=5)
    assert np.all(np.isfinite(both))
    np.testing.assert_array_equal(ev.evaluate([cands[2]], seed=5, index_offset=2)[0], both[2])


# 6 ---------------------------------------------------------------------------------------------------------------
def test_refusals_and_removal():
    from autompc_amd import _lib
    name = "edges"
    system, ab = C.matrices(name)
    d = C.plan_data(name)
    B = len(C.N_LIST)
    idx = d["index"]
    opened = []
    try:
        hs = [_handle(name, A, Bm, "f64", False, wide=bool(k % 2)) for k, (A, Bm) in enumerate(ab)]
        opened.extend(hs)
        k0 = int(idx[0])
        h = _handle(name, *ab[k0], "f64", False, wide=False)
        opened.append(h)

        def plan_of(handle, cap=C.HORIZON_CAP):
            p = _lib.MppiPlan(handle, d["N"], d["H"], [C.SIGMA] * B, [C.LMDA] * B, cost_index=np.arange(B))
            opened.append(p)
            p.set_geometry(0, cap)
            return p
        plan = plan_of(h)
        who = "ampc_mppi_plan_set_linear_models"
        lib = plan.lib
        with pytest.raises(_lib.AmpcError, match=who + ": NULL argument"):
            _lib.check(lib.ampc_mppi_plan_set_linear_models(plan._p, 2, None, None, None, None, None, None))
        with pytest.raises(_lib.AmpcError, match="model_index out of range"):
            plan.set_linear_models(hs, np.full(B, len(hs)))
        # handles without a linear model: the plan's, a table entry's
        mlp_h = _lib.Handle(0, "f64")
        opened.append(mlp_h)
        rng = np.random.default_rng(0)
        mlp_h.set_mlp(3, 2, [rng.normal(size=(16, 5)), rng.normal(size=(3, 16))], [np.zeros(16), np.zeros(3)], "tanh",
                      np.zeros(5), np.ones(5), np.zeros(3), np.ones(3))
        mlp_h.set_quad_costs(d["Q"], d["R"], d["F"], d["goal"])
        mlp_h.set_ctrl_bounds(np.full(2, C.LO), np.full(2, C.HI))
        with pytest.raises(_lib.AmpcError, match="plan handle's model is not a linear model"):
            plan_of(mlp_h).set_linear_models(hs, idx)
        with pytest.raises(_lib.AmpcError, match="a model handle holds no linear model"):
            plan.set_linear_models(hs[:5] + [mlp_h], idx)
        # other controls, precision
        other = _lib.Handle(0, "f64")
        opened.append(other)
        other.set_linear(0.5 * np.eye(4), np.ones((4, 3)))
        with pytest.raises(_lib.AmpcError, match="control dimension"):
            plan.set_linear_models(hs[:5] + [other], idx)
        f32 = _lib.Handle(0, "f32")
        opened.append(f32)
        f32.set_linear(*ab[0])
        with pytest.raises(_lib.AmpcError, match="device and precision"):
            plan.set_linear_models(hs[:5] + [f32], idx)
        # fewer states than the observation; the rules
        small = _lib.Handle(0, "f64")
        opened.append(small)
        small.set_linear(0.5 * np.eye(2), np.ones((2, 2)))
        with pytest.raises(_lib.AmpcError, match="nx < obs_dim"):
            plan.set_linear_models(hs[:5] + [small], idx)
        with pytest.raises(_lib.AmpcError, match="rule 0 .* needs nx == obs_dim"):
            plan.set_linear_models(hs, idx, rules=[0, 0, 1, 1, 1, 1])
        ident = (np.array([0], dtype=np.int32), np.array([1.0]))
        with pytest.raises(_lib.AmpcError, match="n_basis \\* obs_dim"):
            plan.set_linear_models(hs, idx, rules=[0, 2, 1, 1, 1, 1], lifts=[None, ident, None, None, None, None])
        three = lambda kinds, pars: (np.array(kinds, dtype=np.int32), np.array(pars, dtype=np.float64))
        with pytest.raises(_lib.AmpcError, match="lift kind must be"):
            plan.set_linear_models(hs, idx, rules=[0, 2, 1, 1, 1, 1], lifts=[None, three([0, 4, 2], [1, 1, 1])] + [None] * 4)
        with pytest.raises(_lib.AmpcError, match="powers must be integers"):
            plan.set_linear_models(hs, idx, rules=[0, 2, 1, 1, 1, 1], lifts=[None, three([0, 1, 2], [1, 2.5, 1])] + [None] * 4)
        # a plan with a state lift, or per-problem models of one shape
        lifted = plan_of(hs[0])
        lifted.set_state_lift([0], [1.0])
        with pytest.raises(_lib.AmpcError, match="state lift"):
            lifted.set_linear_models(hs, idx)
        # ... nothing of the above changed the plan: it still solves on its handle's model
        # the table in; what a plan holding it refuses
        plan.set_linear_models(hs, idx)
        with pytest.raises(_lib.AmpcError, match="table of linear models"):
            plan.set_state_lift([0], [1.0])
        with pytest.raises(_lib.AmpcError, match="table of linear models"):
            plan.set_sindy_models([hs[0]], np.zeros(B, dtype=np.int32))
        with pytest.raises(_lib.AmpcError, match="table of linear models"):
            plan.set_models([hs[0]], np.zeros(B, dtype=np.int32))
        with pytest.raises(_lib.AmpcError, match="tile_rows must be 0 or 16"):
            plan.set_geometry(32, C.HORIZON_CAP)
        plan.set_geometry(16, C.HORIZON_CAP)
        x0 = np.concatenate(d["x0"])
        u = np.empty((B, 2))
        with pytest.raises(_lib.AmpcError, match="ampc_mppi_run: .* ragged"):
            _lib.check(lib.ampc_mppi_run(plan._p, _lib.dptr(x0), None, 0, 0, 0, _lib.dptr(u)))
        with pytest.raises(_lib.AmpcError, match="ampc_mppi_set_x0_dev: .* ragged"):
            plan.set_x0_dev(1)
        with pytest.raises(_lib.AmpcError, match="set without rules"):
            plan.closed_loop_linear(hs[0], 2, x0, np.zeros((B, 3)))
        with pytest.raises(_lib.AmpcError, match="ampc_mppi_closed_loop_linear"):
            plan.closed_loop(np.zeros((B, h.nx)), 2, surrogate=hs[0])
        with pytest.raises(ValueError, match="x0 has"):
            plan.upload(x0=np.zeros((B, 3)))
        # -3: a 256-state entry and a horizon cap whose map exceeds 160 KB (2 x 16 x 261 [x | u] rows + cap x 2 controls)
        wide_ab = C.matrices("wide")[1][4]
        wide = _handle(name, *wide_ab, "f64", False, wide=False)
        opened.append(wide)
        cap = (160 * 1024 // 8 - 2 * 16 * 261) // 2 + 1
        big = plan_of(h, cap)
        with pytest.raises(_lib.AmpcError, match="more than 160 KB") as e:
            big.set_linear_models(hs[:5] + [wide], idx)
        assert e.value.code == _lib.MPPI_TABLE_NO_FIT == -3
        big.set_linear_models(hs, idx)                       # (without it the same plan takes the table)
    finally:
        for o in reversed(opened):
            o.close()


def test_removal_restores_the_single_model_plan():
    name = "k4"
    d = C.plan_data(name)
    which = np.nonzero(d["index"] == 1)[0]
    before = _solve(name, which, model=1)
    out = {}

    def swap(plan, opened):
        system, ab = C.matrices(name)
        hs = [_handle(name, A, B, "f64", False, wide=False) for A, B in ab]
        opened.extend(hs)
        plan.set_linear_models(hs, np.ones(len(which), dtype=np.int32))
        plan.set_linear_models(None, None)
        plan.set_geometry(0, C.HORIZON_CAP)
        plan.upload(x0=np.concatenate([d["x0"][b] for b in which]),
                    act_seq=np.concatenate([d["act"][b].ravel() for b in which]),
                    eps=np.concatenate([d["eps"][b].ravel() for b in which]))
        plan.solve()
        out["again"] = plan.download(act_seq=True, u=True, costs=True, eps_out=True)
    _solve(name, which, model=1, after=swap)
    a, u, c, e = out["again"]
    np.testing.assert_array_equal(c, np.concatenate([r[0] for r in before]))
    np.testing.assert_array_equal(u, np.stack([r[3] for r in before]))
    np.testing.assert_array_equal(a, np.concatenate([r[2].ravel() for r in before]))


def test_the_default_is_unchanged_for_a_same_dimension_batch():
    """Two Koopman models of one basis: the "shape" default runs them in one plan as before (on the MLP tile, as an
    identity network), each candidate with the score it has alone.  The table runs the same closed loops on
    linear_rollout_kernel's arithmetic: both are within the 1e-7 the evaluator is held to against simulate(), so within
    2e-7 of each other."""
    from autompc_amd import Koopman
    from autompc_amd.tuning import CandidateEvaluator
    from kstep_mlp_cases import synthetic_trajs
    system, task, ms, mlp, cands, _, _ = _loop()
    twin = Koopman(system, poly_basis="true", poly_degree=3)
    twin.train(synthetic_trajs(system, seed=6), silent=True)
    batch = [dict(cands[0], model=ms[4]), dict(cands[6], model=twin)]
    ev = CandidateEvaluator(system, task, ms[4], surrogate=mlp, horizon_cap=C.HORIZON_CAP, tile_rows=16)
    s = ev.evaluate(batch, n_steps=4, seed=3)
    assert ev.last_models == {"path": "shape", "models": 2, "plans": 1}
    assert ev.linear_models == "shape" and np.all(np.isfinite(s))
    for i, c in enumerate(batch):
        alone = CandidateEvaluator(system, task, c["model"], surrogate=mlp, horizon_cap=C.HORIZON_CAP, tile_rows=16)
        np.testing.assert_array_equal(alone.evaluate([c], n_steps=4, seed=3, index_offset=i)[0], s[i])
    tab = CandidateEvaluator(system, task, ms[4], surrogate=mlp, horizon_cap=C.HORIZON_CAP, linear_models="table")
    st = tab.evaluate(batch, n_steps=4, seed=3)
    assert tab.last_models == {"path": "linear_table", "models": 2, "plans": 1}
    print("shape default against the table: relative difference %s" % (np.abs(st - s) / np.abs(s)))
    np.testing.assert_allclose(st, s, rtol=2e-7)


# 7 ---------------------------------------------------------------------------------------------------------------
def test_tuner_fits_and_scores_a_batch_of_arx_configurations_in_one_plan():
    from autompc_amd.sysid.linear import ARXFactory
    from autompc_amd.tuning import BatchPipelineTuner, CandidateEvaluator, random_candidates
    from kstep_mlp_cases import synthetic_trajs
    system, task, ms, mlp, _, _, _ = _loop()
    no, nu = system.obs_dim, system.ctrl_dim
    trajs = synthetic_trajs(system, seed=5)

    def sampler(n, rng):
        out = random_candidates(system, n, seed=7)
        for i, c in enumerate(out):
            c.update(horizon=min(c["horizon"], C.HORIZON_CAP), sigma=0.3, num_path=max(4, c["num_path"] // 16),
                     Q=np.ones(no), R=0.05 * np.ones(nu), F=np.ones(no), model_cfg={"history": 1 + (3 * i) % 10})
        return out
    ev = CandidateEvaluator(system, task, ms[0], surrogate=mlp, linear_models="table", horizon_cap=C.HORIZON_CAP)
    tuner = BatchPipelineTuner(system, ev, batch_size=8, sampler=sampler, model_factory=ARXFactory(system), trajs=trajs,
                               linear_fit="device")
    inc, res = tuner.run(8, np.random.default_rng(0), seed=2)
    assert ev.last_models == {"path": "linear_table", "models": 8, "plans": 1}
    assert tuner.models_fitted == 8 and len(res.costs) == 8 and np.all(np.isfinite(res.costs))
    assert len({c["model"].state_dim for c in res.cfgs}) == 8
