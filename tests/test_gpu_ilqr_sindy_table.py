"""iLQR candidates on SINDy models of mixed feature libraries in ONE plan (ampc_ilqr_plan_set_sindy_models,
csrc/ilqr_sindy_table_kernels.hpp; ``IlqrCandidateEvaluator(sindy_models="table")``) against the oracle (ILQROracle +
SINDyOracle), against single-model plans, and through the evaluator and the tuner (needs MI355X).  Problems, models and
the oracle's solves: tests/ilqr_sindy_table_cases.py; tests/test_ilqr_sindy_table_host.py shows that these problems do
not amplify rounding into other decisions.  Bounds: states / controls / objective 1e-9 and gains 1e-8 where the oracle
converged, 1e-6 / 1e-5 where it ran to the cap (the project's iLQR bounds, tests/test_gpu_ilqr_table.py)."""
import functools

import numpy as np
import pytest

import ilqr_sindy_table_cases as C
import mppi_sindy_table_cases as M
from helpers import rel_err

pytestmark = pytest.mark.gpu

SETS = sorted(C.PROBLEMS)


def _close(opened):
    for o in reversed(opened):
        o.close()


def _plan(name, slots, opened, table=True, models=None, own=0, precision="f64"):
    """A plan whose cost block j is problem j's; its handle holds model `own` of the set."""
    from autompc_amd import _lib
    system, ms, _, _ = M.models(name, precision)
    d = M.plan_data(name)
    nu = system.ctrl_dim
    bs = [p[1] for p in C.PROBLEMS[name]]
    h = _lib.Handle(0, precision, jit=False)
    opened.append(h)
    ms[own].stage_into(h)
    h.set_cost_blocks(d["Q"][bs], d["R"][bs], d["F"][bs], d["goal"][bs])
    h.set_ctrl_bounds(np.full(nu, C.LO), np.full(nu, C.HI))
    plan = _lib.IlqrPlan(h, slots, C.PLAN_H, system.dt, cost_index=np.arange(slots), clip_to_bounds=True)
    opened.append(plan)
    if table:
        plan.set_sindy_models([m._dev() for m in (ms if models is None else models)])
    return plan


def _queue(plan, name, order=None, index=None, max_iter=C.MAX_ITER, with_index=True):
    order = np.arange(len(C.PROBLEMS[name])) if order is None else np.asarray(order)
    index = C.model_index(name) if index is None else np.asarray(index, dtype=np.int32)
    return plan.solve_queue(C.x0s(name)[order], None, order, max_iter=max_iter, horizon=C.horizons(name)[order],
                            model_index=index[order] if with_index else None)


KEYS = ("states", "ctrls", "Ks", "ks", "objective", "converged", "iters", "status")


def _same(a, i, b, j, what):
    for key in KEYS:
        np.testing.assert_array_equal(a[key][i], b[key][j], err_msg="%s: %s" % (what, key))


def _against_oracle(out, name, want, slots):
    worst = {True: np.zeros(5), False: np.zeros(5)}
    hz = C.horizons(name)
    for j, o in enumerate(want):
        H = int(hz[j])
        assert bool(out["converged"][j]) == o["converged"] and int(out["iters"][j]) == o["iters"], (name, j)
        assert int(out["status"][j]) == 0
        dev = np.array([rel_err(out["states"][j, :H + 1], o["states"]), rel_err(out["ctrls"][j, :H], o["ctrls"]),
                        abs(out["objective"][j] - o["obj"]) / max(1.0, abs(o["obj"])),
                        rel_err(out["Ks"][j, :H], o["Ks"]), rel_err(out["ks"][j, :H], o["ks"])])
        print("%s, %d slots, problem %d (%s): states %.2e ctrls %.2e objective %.2e Ks %.2e ks %.2e"
              % (name, slots, j, "converged" if o["converged"] else "cap", *dev))
        worst[o["converged"]] = np.maximum(worst[o["converged"]], dev)
        tol, gtol = (1e-9, 1e-8) if o["converged"] else (1e-6, 1e-5)
        # (ks as test_gpu_ilqr.py bounds it: relative, or -- the feed-forward of a converged solve is ~0 -- absolute)
        ks_abs = float(np.max(np.abs(out["ks"][j, :H] - o["ks"])))
        assert dev[:3].max() < tol and dev[3] < gtol and (dev[4] < gtol or ks_abs < 1e-8), (name, j, dev, ks_abs)
        assert not out["states"][j, H + 1:].any() and not out["Ks"][j, H:].any()        # rows past the horizon: zeros
    print("%s, %d slots: largest deviation, converged: %s; at the cap: %s" % (name, slots, worst[True], worst[False]))


@functools.lru_cache(maxsize=None)
def _batch(name):
    """Every problem of a set through four slots of one table plan (shared, read-only)."""
    opened = []
    try:
        return _queue(_plan(name, 4, opened), name)
    finally:
        _close(opened)


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SETS)
def test_problems_through_fewer_slots_match_the_oracle(name):
    """solve_queue with a non-monotonic model_index, every model shared, per-problem horizons 2..25: through four slots,
    and through two (refill)."""
    _against_oracle(_batch(name), name, C.solves(name), 4)
    opened = []
    try:
        two = _queue(_plan(name, 2, opened), name)
    finally:
        _close(opened)
    _against_oracle(two, name, C.solves(name), 2)
    for j in range(len(C.PROBLEMS[name])):
        _same(two, j, _batch(name), j, "%s: two slots vs four, problem %d" % (name, j))


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SETS)
def test_first_iteration_gains_check_the_jacobian_kernel(name):
    """A solve capped at max_iter = 1: one rollout of the guess, one refresh, one sweep -- the gains are a function of
    the Jacobians alone."""
    opened = []
    try:
        out = _queue(_plan(name, 4, opened), name, max_iter=1)
    finally:
        _close(opened)
    worst = np.zeros(2)
    for j, o in enumerate(C.first_iterations(name)):
        H = int(C.horizons(name)[j])
        dev = np.array([rel_err(out["Ks"][j, :H], o["Ks"]), rel_err(out["ks"][j, :H], o["ks"])])
        print("%s, problem %d: Ks %.2e ks %.2e" % (name, j, *dev))
        assert int(out["iters"][j]) == 1 and int(out["status"][j]) == 0
        worst = np.maximum(worst, dev)
    print("%s: largest deviation of the first iteration's gains: Ks %.2e ks %.2e" % (name, *worst))
    assert worst.max() < 1e-9


# 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SETS)
def test_a_problem_is_the_same_bits_alone_reversed_and_at_another_table_position(name):
    system, ms, _, _ = M.models(name)
    P = len(C.PROBLEMS[name])
    batch = _batch(name)
    opened = []
    try:
        plan = _plan(name, 4, opened)
        rev = np.arange(P)[::-1]
        out = _queue(plan, name, order=rev)
        for k, j in enumerate(rev):
            _same(out, k, batch, j, "%s reversed, problem %d" % (name, j))
        for j in range(P):
            one = _queue(plan, name, order=[j])
            _same(one, 0, batch, j, "%s alone, problem %d" % (name, j))
        # the table rotated by one: every entry at another position (and the plan handle's own model no longer first)
        n = len(ms)
        plan.set_sindy_models([ms[(k + 1) % n]._dev() for k in range(n)])
        moved = _queue(plan, name, index=(C.model_index(name) - 1) % n)
        for j in range(P):
            _same(moved, j, batch, j, "%s, table rotated, problem %d" % (name, j))
    finally:
        _close(opened)


# 4 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SETS)
def test_problems_agree_with_single_model_plans(name):
    """The existing path: a plan on the model's own handle, no table.  The lane-spread body sums in another order, so
    the comparison is 1e-9, not bitwise; the decisions are the same."""
    batch = _batch(name)
    idx, hz = C.model_index(name), C.horizons(name)
    worst = 0.0
    for k in sorted(set(idx.tolist())):
        opened = []
        try:
            plan = _plan(name, 1, opened, table=False, own=k)
            for j in np.nonzero(idx == k)[0]:
                one = _queue(plan, name, order=[j], with_index=False)
                H = int(hz[j])
                assert int(one["converged"][0]) == int(batch["converged"][j]) and int(one["iters"][0]) == int(batch["iters"][j])
                dev = max(rel_err(batch["states"][j, :H + 1], one["states"][0, :H + 1]),
                          rel_err(batch["ctrls"][j, :H], one["ctrls"][0, :H]))
                print("%s, problem %d: table vs single-model plan %.2e" % (name, j, dev))
                worst = max(worst, dev)
        finally:
            _close(opened)
    assert worst < 1e-9


def test_removing_the_table_restores_the_single_model_results():
    name, j = "trio", 2                                    # (cross5 at horizon 16; the plan's handle holds cross5)
    k = int(C.model_index(name)[j])
    opened = []
    try:
        plan = _plan(name, 2, opened, table=False, own=k)
        own = _queue(plan, name, order=[j], with_index=False)
        plan.set_sindy_models([m._dev() for m in M.models(name)[1]])
        tab = _queue(plan, name, order=[j, 0])
        _same(tab, 0, _batch(name), j, "table on another handle")
        plan.set_sindy_models(None)
        back = _queue(plan, name, order=[j], with_index=False)
        _same(back, 0, own, 0, "table removed")
        plan.set_sindy_models(None)                         # (nothing to remove: accepted)
    finally:
        _close(opened)


# 5 ---------------------------------------------------------------------------------------------------------------
def _surrogate(kind):
    S = C.batch()
    if kind == "sindy":
        return S["models"][0][0]
    import ilqr_table_cases
    return ilqr_table_cases.hip_model(S["system"], C.mlp_surrogate_params(S["system"]))


@functools.lru_cache(maxsize=None)
def _table_scores(kind):
    from autompc_amd.tuning import IlqrCandidateEvaluator
    S = C.batch()
    ev = IlqrCandidateEvaluator(S["system"], S["task"], S["models"][0][0], surrogate=_surrogate(kind), sindy_models="table")
    out = ev.evaluate(S["cands"], n_steps=C.STEPS, init_obs=S["init"], return_trajectories=True, max_iter=C.MAX_ITER)
    return out, dict(ev.last_models), ev.last_iterations.copy()


@pytest.mark.parametrize("kind", ["sindy", "mlp"])
def test_evaluator_scores_six_candidates_on_five_models_in_one_plan(kind):
    from autompc_amd import _lib
    from autompc_amd.tuning import IlqrCandidateEvaluator
    S = C.batch()
    (scores, obs, ctl), info, its = _table_scores(kind)
    assert info == {"path": "sindy_table", "models": 5, "plans": 1}
    assert obs.shape == (6, C.STEPS + 1, S["system"].obs_dim)
    worst = np.zeros(3)
    for i, loop in enumerate(C.oracle_loops(kind)):
        dev = np.array([rel_err(obs[i], loop["obs"]), rel_err(ctl[i], loop["ctrls"]),
                        abs(scores[i] - loop["score"]) / abs(loop["score"])])
        print("%s surrogate, candidate %d vs the oracle: obs %.2e ctrls %.2e score %.2e" % (kind, i, *dev))
        worst = np.maximum(worst, dev)
        assert int(its[i]) == loop["iters"], i
    assert worst.max() < 1e-9
    kw = dict(n_steps=C.STEPS, init_obs=S["init"], return_trajectories=True, max_iter=C.MAX_ITER)
    worst = np.zeros(3)
    for i, c in enumerate(S["cands"]):
        alone = IlqrCandidateEvaluator(S["system"], S["task"], c["model"], surrogate=_surrogate(kind))
        s1, o1, c1 = alone.evaluate([{k: v for k, v in c.items() if k != "model"}], **kw)
        assert alone.last_models["path"] == "shape"
        worst = np.maximum(worst, [rel_err(obs[i], o1[0]), rel_err(ctl[i], c1[0]), abs(scores[i] - s1[0]) / abs(s1[0])])
        assert int(alone.last_iterations[0]) == int(its[i]), i
    print("%s surrogate, table vs one-candidate evaluators: obs %.2e ctrls %.2e score %.2e" % (kind, *worst))
    assert worst.max() < 1e-9
    # the default is today's behaviour: the library refuses a SINDy model per slot
    with pytest.raises(_lib.AmpcError, match="per-problem models are MLP models"):
        IlqrCandidateEvaluator(S["system"], S["task"], S["models"][0][0], surrogate=_surrogate(kind)).evaluate(
            S["cands"], n_steps=C.STEPS, init_obs=S["init"], max_iter=C.MAX_ITER)


def test_a_singular_candidate_scores_inf_and_disturbs_nobody():
    from autompc_amd.tuning import IlqrCandidateEvaluator
    S = C.batch()
    (s, obs, ctl), _, _ = _table_scores("sindy")
    nx, nu = S["system"].obs_dim, S["system"].ctrl_dim
    sing = dict(S["cands"][1], Q=np.zeros(nx), R=np.zeros(nu), F=np.zeros(nx))
    cands = S["cands"][:3] + [sing] + S["cands"][3:]
    ev = IlqrCandidateEvaluator(S["system"], S["task"], S["models"][0][0], surrogate=_surrogate("sindy"),
                                sindy_models="table")
    s_x, obs_x, ctl_x = ev.evaluate(cands, n_steps=C.STEPS, init_obs=S["init"], return_trajectories=True,
                                    max_iter=C.MAX_ITER)
    assert ev.last_models == {"path": "sindy_table", "models": 5, "plans": 1}
    assert np.isinf(s_x[3])
    keep = [0, 1, 2, 4, 5, 6]
    np.testing.assert_array_equal(s_x[keep], s)
    np.testing.assert_array_equal(obs_x[keep], obs)
    np.testing.assert_array_equal(ctl_x[keep], ctl)


def test_user_term_cond_runs_the_host_loop_on_the_table():
    """Episodes that a user condition ends at different rows: one queue of solves per control step on the table plan;
    score and length equal the one-candidate evaluation."""
    from autompc_amd.tuning import IlqrCandidateEvaluator
    S = C.batch()
    task = C.make_task(S["system"])
    task.set_num_steps(5)
    task.set_term_cond(lambda traj: len(traj) >= 3 + int(40.0 * abs(traj.ctrls[0, 0])) % 3)
    ev = IlqrCandidateEvaluator(S["system"], task, S["models"][0][0], sindy_models="table")
    scores = ev.evaluate(S["cands"], init_obs=S["init"], max_iter=C.MAX_ITER)
    assert ev.last_models == {"path": "sindy_table", "models": 5, "plans": 1}
    lengths = ev.last_lengths.copy()
    print("rows per candidate:", lengths.tolist())
    assert np.all(np.isfinite(scores)) and 3 <= lengths.min() and lengths.max() <= 5
    for i, c in enumerate(S["cands"]):
        one = ev.evaluate([c], init_obs=S["init"], max_iter=C.MAX_ITER)
        assert ev.last_models == {"path": "sindy_table", "models": 1, "plans": 1}
        assert one[0] == scores[i] and int(ev.last_lengths[0]) == int(lengths[i])


def test_tuner_fits_and_scores_a_batch_of_sindy_configurations():
    from autompc_amd import Trajectory
    from autompc_amd.sysid.sindy import SINDyFactory
    from autompc_amd.tuning import BatchPipelineTuner, IlqrCandidateEvaluator, random_ilqr_candidates
    S = C.batch()
    system = S["system"]
    nx, nu = system.obs_dim, system.ctrl_dim
    task = C.make_task(system)
    task.set_init_obs(S["init"])
    task.set_num_steps(4)
    rng = np.random.default_rng(5)
    A = 0.9 * np.eye(nx) + 0.05 * rng.normal(size=(nx, nx))
    Bm = 0.1 * rng.normal(size=(nx, nu))
    trajs = []
    for _ in range(12):
        o, u = np.zeros((40, nx)), rng.uniform(C.LO, C.HI, size=(40, nu))
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
        out = random_ilqr_candidates(system, n, seed=7)
        for i, c in enumerate(out):
            c.update(Q=np.ones(nx), R=0.05 * np.ones(nu), F=np.ones(nx), model_cfg=dict(libraries[i % 4]))
        return out
    ev = IlqrCandidateEvaluator(system, task, S["models"][0][0], sindy_models="table")
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
    assert one[0] == res.costs[k]


# 6 ---------------------------------------------------------------------------------------------------------------
def test_refusals():
    from autompc_amd import MLP, SINDy, _lib
    who = "ampc_ilqr_plan_set_sindy_models"
    system, ms, _, _ = M.models("trio")
    handles = [m._dev() for m in ms]
    opened = []

    def refused(plan, hs, match, code=-1):
        with pytest.raises(_lib.AmpcError, match=match) as e:
            plan.set_sindy_models(hs)
        assert who in str(e.value) and e.value.code == code

    def plan_on(stage, precision="f64", no=3, nu=2):
        h = _lib.Handle(0, precision, jit=False)
        opened.append(h)
        stage(h)
        h.set_quad_costs(np.eye(no)[None], np.eye(nu)[None], np.eye(no)[None], np.zeros((1, no)))
        plan = _lib.IlqrPlan(h, 2, 5, system.dt)
        opened.append(plan)
        return plan

    try:
        good = plan_on(ms[0].stage_into)
        lib = _lib.load()
        # NULL arguments on a live plan
        assert lib.ampc_ilqr_plan_set_sindy_models(good._p, 2, None) == -1
        assert (who + ": NULL argument").encode() in lib.ampc_last_error()
        assert lib.ampc_ilqr_plan_set_sindy_models(good._p, -1, None) == -1
        assert (who + ": NULL argument").encode() in lib.ampc_last_error()
        assert lib.ampc_ilqr_plan_set_sindy_models(None, 1, None) == -1
        assert (who + ": NULL plan").encode() in lib.ampc_last_error()
        arr = (_lib.c_void_p * 2)(handles[0]._h, None)
        assert lib.ampc_ilqr_plan_set_sindy_models(good._p, 2, arr) == -1
        assert (who + ": NULL model handle").encode() in lib.ampc_last_error()
        # an f32 plan
        ms32 = M.models("trio", "f32")[1]
        refused(plan_on(ms32[0].stage_into, "f32"), [m._dev() for m in ms32], "f64 only")
        # a plan handle / a model handle without a SINDy model
        mlp = MLP(system, n_hidden_layers=1, hidden_size_1=16)
        mlp.jit_kernels = False
        refused(plan_on(mlp.stage_into), handles, "plan handle's model is not a SINDy model")
        hm = _lib.Handle(0, "f64", jit=False)
        opened.append(hm)
        mlp.stage_into(hm)
        refused(good, [handles[0], hm], "model handle holds no SINDy model")
        he = _lib.Handle(0, "f64", jit=False)
        opened.append(he)
        refused(good, [handles[0], he], "model handle holds no SINDy model")
        # other dimensions, another precision
        refused(good, [handles[0], M.models("c1")[1][0]._dev()], "state and control dimensions")
        refused(good, [handles[0], ms32[1]._dev()], "device and precision")
        # a cost on fewer observations than the model has states
        refused(plan_on(ms[0].stage_into, no=2), handles, "observation dimension must be the state dimension")
        # the table and the other two per-slot model calls exclude each other
        good.set_sindy_models(handles)
        with pytest.raises(_lib.AmpcError, match="ampc_ilqr_plan_set_models: the plan holds a table of SINDy models"):
            good.set_models([handles[0]])
        with pytest.raises(_lib.AmpcError, match="ampc_ilqr_plan_set_model_table: the plan holds a table of SINDy models"):
            good.set_model_table([mlp])
        # a model_index past the table; none without a table
        with pytest.raises(_lib.AmpcError, match="bad model_index"):
            good.solve_queue(np.zeros((2, 3)), None, None, max_iter=1, model_index=[0, 3])
        with pytest.raises(_lib.AmpcError, match="bad model_index"):
            good.closed_loop(np.zeros((2, 3)), 1, max_iter=1, model_index=[-1, 0])
        # a refused replacement leaves the table in place
        refused(good, [handles[0], hm], "model handle holds no SINDy model")
        out = good.solve_queue(0.1 * np.ones((2, 3)), None, None, max_iter=2, model_index=[2, 1])
        assert np.all(np.isfinite(out["objective"])) and not out["status"].any()
        good.set_sindy_models(None)
        with pytest.raises(_lib.AmpcError, match="no model table"):
            good.solve_queue(np.zeros((2, 3)), None, None, max_iter=1, model_index=[0, 1])
        # an MLP plan that holds set_model_table / set_models entries refuses this call by its handle already; the two
        # messages of the entry itself run in the stand-alone host check (tools/ilqr_sindy_table_hostcheck.cpp)
        tab = plan_on(mlp.stage_into)
        tab.set_model_table([mlp])
        refused(tab, handles, "plan handle's model is not a SINDy model")
    finally:
        _close(opened)


def test_a_declined_table_runs_one_plan_per_model(monkeypatch):
    """Return code -3 (an entry's LDS need exceeds 160 KB).  No plan inside the entry's other limits reaches it: the
    largest map here -- hc_trigx, 16 rows of 17 + 6 + 1 and of 17, no table, nothing staged, a dense 17 / 6 cost block
    -- is under 20 KB, and a staged program adds at most 48 KB.  So the refusal is put in the binding's place (as the
    MPPI table's tests do); the refusal itself runs in the stand-alone host check.  The evaluator then gives every
    model a plan of its own on the single-model kernels: the same scores within 1e-9 (another summation order)."""
    from autompc_amd import _lib
    from autompc_amd.tuning import IlqrCandidateEvaluator
    S = C.batch()
    (want, _, _), _, _ = _table_scores("sindy")
    ev = IlqrCandidateEvaluator(S["system"], S["task"], S["models"][0][0], surrogate=_surrogate("sindy"),
                                sindy_models="table")
    real = _lib.IlqrPlan.set_sindy_models

    def declined(self, handles):
        if handles:
            err = _lib.AmpcError("ampc_ilqr_plan_set_sindy_models: declined by the test")
            err.code = _lib.ILQR_TABLE_NO_FIT
            raise err
        real(self, handles)
    monkeypatch.setattr(_lib.IlqrPlan, "set_sindy_models", declined)
    got = ev.evaluate(S["cands"], n_steps=C.STEPS, init_obs=S["init"], max_iter=C.MAX_ITER)
    assert ev.last_models == {"path": "model", "models": 5, "plans": 5}
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=0)
