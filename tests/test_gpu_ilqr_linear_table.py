"""The iLQR plan that holds a table of linear models of mixed state dimension (ampc_ilqr_plan_set_linear_models,
csrc/ilqr_linear_table_kernels.hpp) on the device: against the oracle's iLQR, bit for bit against single-model plans on
the wide linear path (handles staged under AMPC_LINEAR_WIDE=1), against itself alone / reversed / at another table
position / after a slot held another size, the sweep alone (max_iter = 1), the closed loop against simulate() with every
model's own update_state, the refusals, and through the evaluator and the tuner.  Problems and models:
tests/ilqr_linear_table_cases.py.  Needs MI355X."""
import functools

import numpy as np
import pytest

import ilqr_linear_table_cases as C
from helpers import make_system, rel_err

pytestmark = pytest.mark.gpu

# the entry each set's plan handle is staged with by default: 3 states as an identity network, 128 states wide, 23 states
PLAN_MODEL = {"edges": 0, "wide": 4, "nu6": 1}
KEYS = ("converged", "iters", "status", "objective", "states", "ctrls", "Ks", "ks", "states_tail", "Ks_tail")


def _handle(name, A, B, wide):
    """A handle holding (A, B) with the set's cost blocks and bounds; wide: staged for the wide linear kernels whatever
    its size (AMPC_LINEAR_WIDE=1), else the way ampc_set_linear picks by itself."""
    from autompc_amd import _lib
    d = C.problems(name)
    h = _lib.Handle(0, "f64", jit=False)
    with pytest.MonkeyPatch.context() as mp:
        if wide:
            mp.setenv("AMPC_LINEAR_WIDE", "1")
        else:
            mp.delenv("AMPC_LINEAR_WIDE", raising=False)
        h.set_linear(A, B)
    h.set_quad_costs(d["Q"], d["R"], d["F"], d["goal"])
    nu = B.shape[1]
    h.set_ctrl_bounds(np.full(nu, C.LO), np.full(nu, C.HI))
    return h


class _Table:
    """The set's models on handles of their own (alternating staging forms) and a plan of `slots` slots on a table of
    them; plan_model: the entry the plan handle is staged with, plan_wide: its staging form."""

    def __init__(self, name, slots, order=None, plan_model=None, plan_wide=False, rules=None, lifts=None):
        from autompc_amd import _lib
        system, ab = C.matrices(name)
        self.name, self.order = name, list(range(len(ab))) if order is None else list(order)
        self.opened = []
        self.handles = [_handle(name, *ab[k], wide=bool(k % 2)) for k in self.order]
        self.opened.extend(self.handles)
        self.h = _handle(name, *ab[PLAN_MODEL[name] if plan_model is None else plan_model], wide=plan_wide)
        self.opened.append(self.h)
        self.plan = _lib.IlqrPlan(self.h, slots, C.PLAN_H, C.DT, cost_index=np.zeros(slots, dtype=np.int32),
                                  clip_to_bounds=True)
        self.opened.append(self.plan)
        self.plan.set_linear_models(self.handles, rules, lifts)

    def solve(self, which=None, max_iter=C.MAX_ITER):
        """Problems `which` of the set (all by default) through the queue; model_index follows the table's order."""
        d = C.problems(self.name)
        which = list(range(len(d["index"]))) if which is None else list(which)
        pos = {k: i for i, k in enumerate(self.order)}
        mi = np.array([pos[int(d["index"][j])] for j in which], dtype=np.int32)
        return self.plan.solve_queue([d["x0"][j] for j in which], None, np.array(which, dtype=np.int32), max_iter=max_iter,
                                     horizon=d["hz"][which], model_index=mi)

    def close(self):
        for o in reversed(self.opened):
            o.close()


def _batch(name, slots=4, max_iter=C.MAX_ITER):
    """The set's problems through ONE table plan (shared by the tests; read-only)."""
    return _batch_cached(name, slots, max_iter)


@functools.lru_cache(maxsize=None)
def _batch_cached(name, slots, max_iter):
    t = _Table(name, slots)
    try:
        return t.solve(max_iter=max_iter)
    finally:
        t.close()


def _same(a, b, ja, jb):
    for k in KEYS:
        np.testing.assert_array_equal(np.asarray(a[k][ja]), np.asarray(b[k][jb]), err_msg=k)


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slots", [4, 2])
@pytest.mark.parametrize("name", sorted(C.SETS))
def test_against_the_oracle(name, slots):
    """The oracle's decisions; states 1e-7, controls, gains 1e-6, objective 1e-8 relative -- the bounds
    tests/test_linear_wide.py::test_wide_linear_ilqr_vs_oracle_and_queue holds the wide path to; zeros past a problem's
    own horizon and own nx."""
    d = C.problems(name)
    got = _batch(name, slots)
    ref = C.oracle_solves(name)
    worst = dict(states=0.0, ctrls=0.0, Ks=0.0, objective=0.0)
    for j, r in enumerate(ref):
        Hj = int(d["hz"][j])
        assert bool(got["converged"][j]) == r["converged"] and int(got["iters"][j]) == r["iters"], (name, j)
        assert int(got["status"][j]) == 0
        e = dict(states=rel_err(got["states"][j][:Hj + 1], r["states"]), ctrls=rel_err(got["ctrls"][j][:Hj], r["ctrls"]),
                 Ks=rel_err(got["Ks"][j][:Hj], r["Ks"]),
                 objective=abs(got["objective"][j] - r["objective"]) / max(1.0, abs(r["objective"])))
        for k, v in e.items():
            worst[k] = max(worst[k], float(v))
        assert e["states"] < 1e-7 and e["ctrls"] < 1e-6 and e["Ks"] < 1e-6 and e["objective"] < 1e-8, (name, j, e)
        assert not np.any(got["states"][j][Hj + 1:]) and not np.any(got["ctrls"][j][Hj:])
        assert not np.any(got["Ks"][j][Hj:]) and not np.any(got["ks"][j][Hj:])
        assert not np.any(got["states_tail"][j]) and not np.any(got["Ks_tail"][j])
    print("%s, %d slots: largest deviation from the oracle %s" % (name, slots, worst))


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.SETS))
def test_bit_for_bit_the_single_model_plan(name):
    """Every key of solve_queue's result equals that of a plan on ONE model staged for the wide linear path
    (ilqr_riccati_wide_kernel + ilqr_iter_kernel<double, 1, 8, 2>), same horizon, cost block and bounds."""
    from autompc_amd import _lib
    system, ab = C.matrices(name)
    d = C.problems(name)
    got = _batch(name)
    for j, k in enumerate(d["index"]):
        h = _handle(name, *ab[int(k)], wide=True)
        plan = _lib.IlqrPlan(h, 1, C.PLAN_H, C.DT, cost_index=np.zeros(1, dtype=np.int32), clip_to_bounds=True)
        ref = plan.solve_queue(d["x0"][j][None, :], None, np.array([j], dtype=np.int32), max_iter=C.MAX_ITER,
                               horizon=d["hz"][j:j + 1])
        plan.close()
        h.close()
        for key in ("converged", "iters", "status", "objective", "states", "ctrls", "Ks", "ks"):
            np.testing.assert_array_equal(np.asarray(got[key][j]), ref[key][0], err_msg="%s problem %d %s" % (name, j, key))


# 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.SETS))
def test_same_bits_alone_reversed_moved_and_after_another_size(name):
    d = C.problems(name)
    P = len(d["index"])
    got = _batch(name)
    n_models = len(C.SETS[name]["nx"])
    # reversed problem order, and the table rotated so that every model sits at another position
    t = _Table(name, 4, order=[(k + 2) % n_models for k in range(n_models)], plan_model=1, plan_wide=True)
    try:
        rev = t.solve(list(range(P))[::-1])
        for j in range(P):
            _same(got, rev, j, P - 1 - j)
        # alone, through one slot of the same plan
        for j in (0, 3, P - 1):
            one = t.solve([j])
            _same(got, one, j, 0)
    finally:
        t.close()
    # one slot: it holds the widest model, then the narrowest, then each other problem -- stale rows in a region
    # sized for the widest entry would show
    nx = np.array(C.SETS[name]["nx"])[d["index"]]
    seq = [int(np.argmax(nx)), int(np.argmin(nx))] + [j for j in range(P) if j not in (int(np.argmax(nx)), int(np.argmin(nx)))]
    seq += [int(np.argmax(nx)), int(np.argmin(nx))]
    t = _Table(name, 1)
    try:
        ser = t.solve(seq)
        for i, j in enumerate(seq):
            _same(got, ser, j, i)
    finally:
        t.close()


# 4 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(C.SETS))
def test_one_iteration_isolates_the_sweep(name):
    """max_iter = 1: the gains depend on the sweep alone (ilqr_riccati_wide_table_kernel)."""
    d = C.problems(name)
    got = _batch(name, 4, 1)
    ref = C.oracle_solves(name, False, 1)
    worst = 0.0
    for j, r in enumerate(ref):
        Hj = int(d["hz"][j])
        assert int(got["iters"][j]) == 1 and int(got["status"][j]) == 0
        eK, ek = float(rel_err(got["Ks"][j][:Hj], r["Ks"])), float(rel_err(got["ks"][j][:Hj], r["ks"]))
        worst = max(worst, eK, ek)
        assert eK < 1e-6 and ek < 1e-6, (name, j, eK, ek)
    print("%s: largest gain deviation after one sweep %.2e" % (name, worst))


# 6 ---------------------------------------------------------------------------------------------------------------
def test_refusals_and_removal():
    from autompc_amd import _lib
    name = "edges"
    system, ab = C.matrices(name)
    d = C.problems(name)
    no, nu = system.obs_dim, system.ctrl_dim
    got = _batch(name)
    t = _Table(name, 4)
    opened = []
    try:
        plan, hs = t.plan, t.handles

        def refused(match, fn, *a, **kw):
            with pytest.raises(_lib.AmpcError, match=match) as e:
                fn(*a, **kw)
            return e.value
        # the non-queue call, the observation-state closed loop, the other tables
        refused("ampc_ilqr_solve: the plan holds a table of linear models", plan.solve, np.zeros((4, 3)),
                np.zeros((4, C.PLAN_H, nu)))
        refused("ampc_ilqr_closed_loop: the plan holds a table of linear models", plan.closed_loop, np.zeros((1, 3)), 2)
        refused("ampc_ilqr_plan_set_models: the plan holds a table of linear models", plan.set_models, hs[:1])
        refused("the plan holds a table of linear models", plan.set_sindy_models, hs[:1])
        # the closed loop on a table without rules
        refused("without rules", plan.closed_loop_linear, None, [d["x0"][6]], np.zeros((1, 3)), 2, model_index=[0])
        # f32, another control dimension, too many states, fewer states than observations, a handle without a linear model
        h32 = _lib.Handle(0, "f32")
        opened.append(h32)
        h32.set_linear(*ab[0])
        e = refused("f64 only", plan.set_linear_models, [hs[0], h32])
        assert e.code == -1
        hu = _lib.Handle(0, "f64")
        opened.append(hu)
        hu.set_linear(ab[1][0], np.zeros((14, 3)))
        refused("control dimension", plan.set_linear_models, [hu])
        hw = _lib.Handle(0, "f64")
        opened.append(hw)
        hw.set_linear(0.5 * np.eye(129), np.zeros((129, nu)))
        refused("up to 128 model states", plan.set_linear_models, [hs[0], hw])
        hn = _lib.Handle(0, "f64")
        opened.append(hn)
        hn.set_linear(0.5 * np.eye(2), np.zeros((2, nu)))
        refused("fewer states than the cost's observation", plan.set_linear_models, [hn])
        he = _lib.Handle(0, "f64")
        opened.append(he)
        refused("holds no linear model", plan.set_linear_models, [he])
        refused("rule 0 .* needs nx == obs_dim", plan.set_linear_models, hs[:2], [0, 0])
        refused("n_basis \\* obs_dim", plan.set_linear_models, hs[:2], [0, 2], [None, ([0, 1], [0.0, 2.0])])
        with pytest.raises(ValueError, match="model_index out of range"):
            plan.solve_queue([d["x0"][6]], model_index=[len(hs)])
        from autompc_amd import MLP
        mlp = MLP(system, n_hidden_layers=1, hidden_size_1=16, nonlintype="tanh")
        rng = np.random.default_rng(3)
        mlp.weights = [rng.normal(scale=0.2, size=(16, no + nu)), rng.normal(scale=0.2, size=(no, 16))]
        mlp.biases = [np.zeros(16), np.zeros(no)]
        mlp.xu_means, mlp.xu_std = np.zeros(no + nu), np.ones(no + nu)
        mlp.dy_means, mlp.dy_std = np.zeros(no), np.ones(no)
        refused("the plan holds a table of linear models", plan.set_model_table, [mlp])
        # every refused replacing call above left the old table working: the same bits
        again = t.solve()
        for j in range(len(d["index"])):
            _same(got, again, j, j)
        # removal: the plan as it was built
        x = d["x0"][6][None, :]                      # (a problem on the 3-state model the plan handle holds)
        fresh = _lib.IlqrPlan(t.h, 4, C.PLAN_H, C.DT, cost_index=np.zeros(4, dtype=np.int32), clip_to_bounds=True)
        opened.append(fresh)
        want = fresh.solve_queue(x, None, np.array([6], dtype=np.int32), horizon=d["hz"][6:7])
        plan.set_linear_models(None)
        back = plan.solve_queue(x, None, np.array([6], dtype=np.int32), horizon=d["hz"][6:7])
        for k in want:
            np.testing.assert_array_equal(back[k], want[k])
        plan.solve(np.tile(x, (4, 1)), np.zeros((4, C.PLAN_H, nu)))            # (allowed again)
        # ... and the other tables refuse a linear table in turn
        mlp_h = _lib.Handle(0, "f64")
        opened.append(mlp_h)
        rng = np.random.default_rng(3)
        mlp_h.set_mlp(no, nu, [rng.normal(scale=0.2, size=(16, no + nu)), rng.normal(scale=0.2, size=(no, 16))],
                      [np.zeros(16), np.zeros(no)], "tanh", np.zeros(no + nu), np.ones(no + nu), np.zeros(no), np.ones(no))
        mlp_h.set_quad_costs(d["Q"], d["R"], d["F"], d["goal"])
        p2 = _lib.IlqrPlan(mlp_h, 2, 4, C.DT)
        opened.append(p2)
        refused("the plan handle's model is not a linear model", p2.set_linear_models, hs[:1])
    finally:
        for o in reversed(opened):
            o.close()
        t.close()


def test_lds_refusal_returns_no_fit():
    """90 observations: a 90-state plan handle fits the line search's LDS, a 128-state entry does not."""
    from autompc_amd import _lib
    no, nu = 90, 2
    rng = np.random.default_rng(9)
    opened = []
    try:
        hs = []
        for nx in (90, 128):
            h = _lib.Handle(0, "f64")
            opened.append(h)
            h.set_linear(0.5 * np.eye(nx), rng.normal(scale=0.1, size=(nx, nu)))
            hs.append(h)
        hs[0].set_quad_costs(np.eye(no)[None], np.eye(nu)[None], np.eye(no)[None], np.zeros((1, no)))
        plan = _lib.IlqrPlan(hs[0], 1, 2, C.DT)
        opened.append(plan)
        plan.set_linear_models(hs[:1])
        with pytest.raises(_lib.AmpcError, match="more than 160 KB") as e:
            plan.set_linear_models(hs)
        assert e.value.code == _lib.ILQR_TABLE_NO_FIT
        out = plan.solve_queue([0.1 * np.ones(no)], model_index=[0], max_iter=3)     # the old table still works
        assert int(out["status"][0]) == 0 and out["states"][0].shape == (3, no)
    finally:
        for o in reversed(opened):
            o.close()


# 5 ---------------------------------------------------------------------------------------------------------------
T = 6


@functools.lru_cache(maxsize=None)
def _loop():
    """Seven trained controller models on one system (ARX of history 1, 2, 4 -- rule 1; Koopman with the identity only --
    rule 0, the observation state; with a degree-3 polynomial, a trig and a mixed basis -- rule 2: power, sin and cos
    lifts), an MLP surrogate and eight candidates in non-monotonic model order (one model twice)."""
    from autompc_amd import ARX, MLP, Koopman, QuadCost, Task
    from kstep_mlp_cases import synthetic_trajs
    system = make_system(3, 2)
    no, nu = 3, 2
    trajs = synthetic_trajs(system, seed=5)
    ms = [ARX(system, history=1), ARX(system, history=2), ARX(system, history=4), Koopman(system),
          Koopman(system, poly_basis="true", poly_degree=3), Koopman(system, trig_basis="true", trig_freq=2),
          Koopman(system, poly_basis="true", poly_degree=2, trig_basis="true", trig_freq=2)]
    for m in ms:
        m.train(trajs, silent=True)
    rng = np.random.default_rng(43)
    mlp = MLP(system, n_hidden_layers=1, hidden_size_1=16, nonlintype="tanh")
    mlp.weights = [rng.normal(scale=0.2, size=(16, no + nu)), rng.normal(scale=0.2, size=(no, 16))]
    mlp.biases = [rng.normal(scale=0.05, size=16), rng.normal(scale=0.01, size=no)]
    mlp.xu_means, mlp.xu_std = np.zeros(no + nu), np.ones(no + nu)
    mlp.dy_means, mlp.dy_std = np.zeros(no), 0.1 * np.ones(no)
    task = Task(system)
    task.set_cost(QuadCost(system, np.eye(no), 0.05 * np.eye(nu), 2.0 * np.eye(no), goal=np.array([0.05, -0.02, 0.0])))
    task.set_ctrl_bounds(-np.ones(nu), np.ones(nu))
    task.set_init_obs(np.array([0.2, -0.15, 0.1]))
    task.set_num_steps(T + 1)
    cands = [dict(horizon=h, Q=rng.uniform(0.5, 2.0, no), R=rng.uniform(0.01, 0.1, nu), F=rng.uniform(0.5, 2.0, no), model=ms[k])
             for h, k in ((8, 4), (2, 0), (5, 5), (3, 2), (8, 1), (6, 3), (4, 4), (7, 6))]
    return system, task, ms, mlp, cands


def _oracle_model(m):
    """The oracle's restatement of a trained ARX / Koopman model (oracle/linear.py), on the model's (A, B)."""
    from autompc_amd import ARX
    from oracle.linear import ARXOracle, KoopmanOracle
    if isinstance(m, ARX):
        return ARXOracle(m.system, m.k, A=m.A, B=m.B)
    return KoopmanOracle(m.system, poly_basis=m.poly_basis, poly_degree=m.poly_degree, trig_basis=m.trig_basis, A=m.A, B=m.B)


def _oracle_episode(i):
    """oracle.closed_loop.simulate with the oracle's iLQR and the oracle model's update_state for candidate i."""
    from oracle.closed_loop import simulate
    from oracle.costs import QuadCostOracle
    from oracle.ilqr import ILQROracle
    system, task, _, mlp, cands = _loop()
    c = cands[i]
    om = _oracle_model(c["model"])
    nu = system.ctrl_dim
    assert om.state_dim == c["model"].state_dim
    ctl = ILQROracle(om, QuadCostOracle(np.diag(c["Q"]), np.diag(c["R"]), np.diag(c["F"]), task.get_cost().get_goal()),
                     system.dt, c["horizon"], ubounds=(-np.ones(nu), np.ones(nu)))
    return simulate(ctl, task.get_init_obs(), mlp, T,
                    traj_to_constate=lambda o: np.concatenate([om.state_from_first_obs(o), np.zeros(nu)]))


def test_closed_loop_is_simulate_with_every_models_own_update_state():
    """1e-8 on observations and controls: the bound tests/test_linear_wide.py holds its device iLQR and Koopman
    episodes to.  Eight chains through three slots."""
    from autompc_amd.tuning import IlqrCandidateEvaluator
    system, task, ms, mlp, cands = _loop()
    B = len(cands)
    assert sorted({m.state_dim for m in ms}) == [3, 4, 9, 18, 19]
    kw = dict(surrogate=mlp, linear_models="table", max_slots=3)
    ev = IlqrCandidateEvaluator(system, task, ms[0], **kw)
    scores, obs, ctl = ev.evaluate(cands, return_trajectories=True)
    assert ev.last_models == {"path": "linear_table", "models": 7, "plans": 1}
    assert obs.shape == (B, T + 1, mlp.state_dim) and ctl.shape == (B, T + 1, 2)
    for i in range(B):
        o, c = _oracle_episode(i)
        eo, ec = float(np.max(np.abs(obs[i] - o))), float(np.max(np.abs(ctl[i] - c)))
        print("candidate %d (%s, %d states): observations %.2e controls %.2e, %d of %d controls at a bound"
              % (i, type(cands[i]["model"]).__name__, cands[i]["model"].state_dim, eo, ec,
                 int(np.sum(np.abs(c[:T]) == 1.0)), c[:T].size))
        assert eo < 1e-8 and ec < 1e-8
    assert np.max(np.abs(ctl)) == 1.0                       # the bounds bite somewhere
    # the evaluator's own term_cond path: every model's update_state on the host, one solve_queue per control step
    # (with a user condition the episode runs num_steps control steps: batch_eval.episode_of)
    import copy
    task2 = copy.copy(task)
    task2.set_num_steps(T)
    task2.set_term_cond(lambda traj: False)
    host = IlqrCandidateEvaluator(system, task2, ms[0], **kw)
    s2, o2, c2 = host.evaluate(cands, return_trajectories=True)
    assert host.last_models["path"] == "linear_table"
    eo, ec = float(np.max(np.abs(o2 - obs))), float(np.max(np.abs(c2 - ctl)))
    print("device loop against the host update_state path: observations %.2e controls %.2e" % (eo, ec))
    assert eo < 1e-8 and ec < 1e-8 and np.max(np.abs(s2 - scores) / np.abs(scores)) < 1e-8
    # a chain is the same bits alone and inside the batch
    for i in (0, 3, 5, 7):
        one = IlqrCandidateEvaluator(system, task, cands[i]["model"], **kw)
        s1, o1, c1 = one.evaluate([cands[i]], return_trajectories=True)
        assert one.last_models == {"path": "linear_table", "models": 1, "plans": 1}
        np.testing.assert_array_equal(s1[0], scores[i])
        np.testing.assert_array_equal(o1[0], obs[i])
        np.testing.assert_array_equal(c1[0], ctl[i])


# 7 ---------------------------------------------------------------------------------------------------------------
def test_evaluator_scores_are_simulate_with_the_drop_in_controller():
    from autompc_amd import IterativeLQR, QuadCost, Task, simulate
    from autompc_amd.tuning import IlqrCandidateEvaluator
    system, task, ms, mlp, cands = _loop()
    nu = system.ctrl_dim
    # the default still refuses: Koopman outright, an ARX with a surrogate that is not itself
    for m in (ms[4], ms[1]):
        with pytest.raises(TypeError, match="score .* candidates with simulate\\(\\) and the drop-in controller"):
            IlqrCandidateEvaluator(system, task, m, surrogate=mlp)
    ev = IlqrCandidateEvaluator(system, task, ms[4], surrogate=mlp, linear_models="table")
    scores = ev.evaluate(cands)
    assert ev.last_models == {"path": "linear_table", "models": 7, "plans": 1}
    for i, c in enumerate(cands):
        t1 = Task(system)
        t1.set_cost(QuadCost(system, np.diag(c["Q"]), np.diag(c["R"]), np.diag(c["F"]), goal=task.get_cost().get_goal()))
        t1.set_ctrl_bounds(-np.ones(nu), np.ones(nu))
        ctl = IterativeLQR(system, t1, c["model"], c["horizon"])
        ctl.reset()
        traj = simulate(ctl, task.get_init_obs(), task.term_cond, sim_model=mlp, max_steps=T)
        want = task.get_cost()(traj)
        print("candidate %d: score %.12g, simulate() %.12g" % (i, scores[i], want))
        assert abs(scores[i] - want) < 1e-8 * abs(want)
    # a batch the table does not take (an MLP among the models) gets the constructor's refusal from evaluate()
    with pytest.raises(TypeError, match="drop-in controller"):
        ev.evaluate([cands[0], dict(cands[1], model=mlp)])


def test_tuner_fits_and_scores_an_arx_batch_with_the_table_evaluator():
    from autompc_amd.sysid.linear import ARXFactory
    from autompc_amd.tuning import BatchPipelineTuner, IlqrCandidateEvaluator
    from kstep_mlp_cases import synthetic_trajs
    system, task, ms, mlp, _ = _loop()
    trajs = synthetic_trajs(system, seed=5)
    ev = IlqrCandidateEvaluator(system, task, ms[1], surrogate=mlp, linear_models="table")
    tuner = BatchPipelineTuner(system, ev, batch_size=6, model_factory=ARXFactory(system), trajs=trajs)
    # the tuner draws ARX sub-configurations for this evaluator ...
    drawn = tuner.ask(12, np.random.default_rng(0))
    assert all(set(c["model_cfg"]) == {"history"} and 1 <= c["model_cfg"]["history"] <= 10 for c in drawn)
    assert len({c["model_cfg"]["history"] for c in drawn}) > 1

    # ... and fits and scores one small batch of them (short horizons: the test stays quick)
    def sampler(n, rng):
        out = tuner._random_search(n, rng)
        for i, c in enumerate(out):
            c.update(horizon=3 + i % 5, model_cfg={"history": 1 + (3 * i) % 10})
        return out
    tuner = BatchPipelineTuner(system, ev, batch_size=6, sampler=sampler, model_factory=ARXFactory(system), trajs=trajs)
    inc, res = tuner.run(6, np.random.default_rng(0), seed=2)
    assert ev.last_models == {"path": "linear_table", "models": 6, "plans": 1}
    assert tuner.models_fitted == 6 and len(res.costs) == 6 and np.all(np.isfinite(res.costs))
    assert len({c["model"].state_dim for c in res.cfgs}) == 6
