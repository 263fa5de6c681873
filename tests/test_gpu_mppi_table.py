"""MPPI candidates on MLP models of mixed shapes in ONE plan (ampc_mppi_plan_set_model_table, csrc/mppi_table_kernels.hpp;
``CandidateEvaluator(mlp_models="table")``) against the oracle, the reference's golden closed loop and the default
one-plan-per-shape path (needs MI355X).  Six models sit on the kernel's edges: one 16-unit layer, widths that are no
multiple of the 16-column tile, the widest network, a one-unit layer, four layers, 255 units; sample counts of exactly one
tile, a tile plus one row, less than a tile; horizons from the minimum to the cap."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (before the library, as in test_gpu_kstep_mlp.py: the device fit runs on torch's GPU)

import mppi_table_cases as C
from conftest import golden
from helpers import check_weights, golden_params, make_system, rel_err
from oracle import mlp as omlp

pytestmark = pytest.mark.gpu

_hip_model, _task, _stack, _six, _fed_noise = C.hip_model, C.make_task, C.stack, C.six, C.fed_noise
EDGES, T = C.EDGES, C.T


def _evaluator(S, mode="table", **kw):
    from autompc_amd.tuning import CandidateEvaluator
    return CandidateEvaluator(S["system"], kw.pop("task", S["task"]), S["own"], surrogate=S["sur"], mlp_models=mode, **kw)


def _against_the_oracle(S, ev, steps, what):
    """Every candidate's obs, ctrls and score against its own MPPIOracle + MLPOracle closed loop, fed the same noise
    (written as test_candidate_batch_matches_oracle_per_candidate writes it); returns the largest deviations."""
    cands, init = S["cands"], S["init"]
    acts, eps = _fed_noise(cands, S["system"].ctrl_dim, steps)
    eps_all = np.concatenate([np.concatenate([e.ravel() for e in step]) for step in eps])
    scores, obs, ctrls = ev.evaluate(cands, n_steps=steps, init_obs=init, eps_all=eps_all,
                                     act_init=np.concatenate([a.ravel() for a in acts]), return_trajectories=True)
    assert ev.last_models == {"path": "table", "models": len(cands), "plans": 1}
    worst = np.zeros(3)
    for b, c in enumerate(cands):
        o_obs, o_ctl, ref = C.oracle_loop(S, b, steps, acts, eps)
        dev = np.array([rel_err(obs[b], o_obs), rel_err(ctrls[b], o_ctl),
                        abs(scores[b] - ref) / abs(ref)])
        print("%s, candidate %d: obs %.2e ctrls %.2e score %.2e" % (what, b, *dev))
        worst = np.maximum(worst, dev)
    print("%s: largest deviation from the oracle: obs %.2e ctrls %.2e score %.2e" % (what, *worst))
    assert worst.max() < 1e-9
    return worst


# 1 ---------------------------------------------------------------------------------------------------------------
def test_six_edge_shapes_in_one_plan_match_the_oracle_per_candidate():
    """1e-9 relative, the project's k-step bound.  On exactly these candidates a rounding-level perturbation of the
    oracle (a permutation of the hidden units) moves trajectories and scores by at most 7e-15 over the four steps."""
    S = _six()
    _against_the_oracle(S, _evaluator(S), T, "six edge shapes")


@pytest.mark.parametrize("which", ["sixteen", "forty_eight"])
def test_two_more_systems_in_one_plan_match_the_oracle_per_candidate(which):
    """16 / 16 (in = 32, one output tile) and 48 / 16 (in = 64, three output tiles): four models each, widths 15, 65,
    129, 193 and a depth-3 net, 5 / 16 / 17 / 33 samples, horizons 2 to 7.  1e-9 as above: on these candidates a
    permutation of the oracle's hidden units moves trajectories and scores by less than 1e-12
    (test_mppi_table_host.py)."""
    S = getattr(C, which)()
    assert {c["num_path"] for c in S["cands"]} == {5, 16, 17, 33} and len(S["cands"]) == 4
    _against_the_oracle(S, _evaluator(S), T, "%d states / %d controls" % (S["system"].obs_dim, S["system"].ctrl_dim))


# 2 ---------------------------------------------------------------------------------------------------------------
def test_reference_golden_closed_loop_as_one_candidate_of_a_table_plan():
    from autompc_amd import QuadCost
    g = golden("loop_mppi")
    nx, N, H, steps = int(g["nx"]), int(g["N"]), int(g["H"]), 20
    system = make_system(nx, 1)
    p = golden_params(nx, 1, g["hidden"], g["activation"], g["mlp_seed"], True)
    check_weights(p, g)
    task = _task(system, QuadCost(system, g["Q"], g["R"], g["F"], goal=g["goal"]))
    task.set_ctrl_bounds([g["bounds"][0]], [g["bounds"][1]])
    np.random.seed(int(g["np_seed"]))
    scale = np.sqrt(float(g["sigma"]))
    act0 = np.random.normal(scale=scale, size=(H, 1))
    eps_g = np.stack([np.random.normal(scale=scale, size=(N, H, 1)) for _ in range(steps)])
    gold = dict(horizon=H, sigma=float(g["sigma"]), lmda=float(g["lmda"]), num_path=N, Q=g["Q"], R=g["R"], F=g["F"])
    own = _hip_model(system, p)
    others = [dict(gold, horizon=7, num_path=21, model=_hip_model(system, golden_params(nx, 1, [20], "tanh", 5, True))),
              dict(gold, horizon=12, num_path=40,
                   model=_hip_model(system, golden_params(nx, 1, [33, 17], "relu", 6, True)))]
    cands = [others[0], gold, others[1]]
    rng = np.random.default_rng(1)
    acts = [rng.normal(scale=scale, size=(7, 1)), act0, rng.normal(scale=scale, size=(12, 1))]
    eps_all = np.concatenate([np.concatenate([rng.normal(scale=scale, size=21 * 7), eps_g[s].ravel(),
                                              rng.normal(scale=scale, size=40 * 12)]) for s in range(steps)])
    from autompc_amd.tuning import CandidateEvaluator
    ev = CandidateEvaluator(system, task, own, mlp_models="table")
    scores, obs, ctrls = ev.evaluate(cands, n_steps=steps, init_obs=g["init"], eps_all=eps_all,
                                     act_init=np.concatenate([a.ravel() for a in acts]), return_trajectories=True)
    assert ev.last_models == {"path": "table", "models": 3, "plans": 1}
    print("golden loop_mppi in a table plan: obs %.2e ctrls %.2e score %.2e"
          % (rel_err(obs[1], g["obs"]), rel_err(ctrls[1], g["ctrls"]), abs(scores[1] - g["score"]) / abs(g["score"])))
    assert rel_err(obs[1], g["obs"]) < 1e-7 and rel_err(ctrls[1], g["ctrls"]) < 1e-7
    assert abs(scores[1] - g["score"]) < 1e-7 * abs(g["score"])
    assert np.all(np.isfinite(scores))


# 3, 4 ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _six_on_device_noise():
    S = _six()
    ev = _evaluator(S)
    out = ev.evaluate(S["cands"], n_steps=T, seed=3, init_obs=S["init"], return_trajectories=True)
    return out, dict(ev.last_models)


def test_table_scores_agree_with_the_default_path():
    S = _six()
    (s_tab, _, _), info = _six_on_device_noise()
    assert info == {"path": "table", "models": 6, "plans": 1}
    ev = _evaluator(S, "shape")
    s_shape = ev.evaluate(S["cands"], n_steps=T, seed=3, init_obs=S["init"])
    assert ev.last_models == {"path": "shape", "models": 6, "plans": 6}
    print("table vs shape, six candidates: %.2e" % float(np.max(np.abs(s_tab - s_shape) / np.abs(s_shape))))
    np.testing.assert_allclose(s_tab, s_shape, rtol=1e-9, atol=0)


def test_a_candidate_is_the_same_bits_alone_reversed_and_in_the_batch():
    S = _six()
    (s, obs, ctl), _ = _six_on_device_noise()
    ev = _evaluator(S)
    rev = list(range(6))[::-1]
    s_r, obs_r, ctl_r = ev.evaluate([S["cands"][i] for i in rev], n_steps=T, seed=3, init_obs=S["init"],
                                    return_trajectories=True, index_offset=np.array(rev))
    np.testing.assert_array_equal(s_r[::-1], s)
    np.testing.assert_array_equal(obs_r[::-1], obs)
    np.testing.assert_array_equal(ctl_r[::-1], ctl)
    for i in range(6):
        s_1, obs_1, ctl_1 = ev.evaluate([S["cands"][i]], n_steps=T, seed=3, init_obs=S["init"],
                                        return_trajectories=True, index_offset=i)
        assert ev.last_models == {"path": "table", "models": 1, "plans": 1}
        np.testing.assert_array_equal(s_1[0], s[i])
        np.testing.assert_array_equal(obs_1[0], obs[i])
        np.testing.assert_array_equal(ctl_1[0], ctl[i])
    s_again, _, _ = ev.evaluate(S["cands"], n_steps=T, seed=3, init_obs=S["init"], return_trajectories=True)
    np.testing.assert_array_equal(s_again, s)


# 5 ---------------------------------------------------------------------------------------------------------------
def _spd(n, rng, scale=1.0):
    a = rng.normal(size=(n, n))
    return scale * (a @ a.T / n + np.eye(n))


def test_dense_and_affine_cost_blocks_agree_with_the_default_path():
    from autompc_amd import QuadCost
    S = _six()
    system = S["system"]
    nx, nu = 17, 6
    rng = np.random.default_rng(12)
    base = [S["cands"][i] for i in (0, 1, 3, 4)]

    def two_goals(diagonal):
        mk = (lambda n, sc: np.diag(rng.uniform(0.5, 2.0, size=n)) * sc) if diagonal else (lambda n, sc: _spd(n, rng, sc))
        return (QuadCost(system, mk(nx, 1.0), mk(nu, 0.1), mk(nx, 2.0), goal=rng.normal(scale=0.1, size=nx))
                + QuadCost(system, mk(nx, 0.5), mk(nu, 0.05), mk(nx, 0.5), goal=rng.normal(scale=0.1, size=nx)))
    # dense, non-diagonal Q / R / F on two candidates and sums of quadratics with different goals on two others ...
    dense = [dict(base[0], Q=_spd(nx, rng), R=_spd(nu, rng, 0.1), F=_spd(nx, rng, 2.0)),
             dict(base[1], Q=_spd(nx, rng), R=_spd(nu, rng, 0.1), F=_spd(nx, rng, 2.0)),
             dict(base[2], cost=two_goals(False)), dict(base[3], cost=two_goals(False))]
    # ... and the affine part on the diagonal fast path
    diag = [dict(base[2], cost=two_goals(True)), dict(base[0], cost=two_goals(True))]
    for name, cands in (("dense + affine", dense), ("diagonal + affine", diag)):
        ev_t, ev_s = _evaluator(S), _evaluator(S, "shape")
        a = ev_t.evaluate(cands, n_steps=T, seed=5, init_obs=S["init"])
        b = ev_s.evaluate(cands, n_steps=T, seed=5, init_obs=S["init"])
        assert ev_t.last_models["path"] == "table" and ev_s.last_models["path"] == "shape"
        print("%s cost blocks, table vs shape: %.2e" % (name, float(np.max(np.abs(a - b) / np.abs(b)))))
        np.testing.assert_allclose(a, b, rtol=1e-9, atol=0)


def _direct_plan(system, models, idx, n, hz, term_mode, cap=30, alone=None):
    """A handle + plan over len(idx) problems (samples n[b], horizon hz[b]) with fed x0 / warm start / noise: problem b
    on models[idx[b]] through a table, or -- alone = k -- every problem on models[k], staged into the handle, on the
    run-time-shape kernels."""
    from autompc_amd import _lib
    nx, nu = system.obs_dim, system.ctrl_dim
    table = alone is None
    h = _lib.Handle(0, "f64", jit=False)
    models[0 if table else alone].stage_into(h)
    rng = np.random.default_rng(21)
    B = len(idx)
    h.set_quad_costs(np.stack([np.diag(rng.uniform(0.5, 2.0, nx)) for _ in range(B)]),
                     np.stack([np.diag(rng.uniform(0.01, 0.1, nu)) for _ in range(B)]),
                     np.stack([np.diag(rng.uniform(0.5, 2.0, nx)) for _ in range(B)]), np.zeros((B, nx)))
    h.set_ctrl_bounds(-np.ones(nu), np.ones(nu))
    plan = _lib.MppiPlan(h, n, hz, [0.5] * B, [0.8] * B, cost_index=np.arange(B), term_mode=term_mode)
    plan.set_geometry(16, cap)
    if table:
        plan.set_model_table(models, idx)
    x0 = rng.uniform(-0.1, 0.1, size=(B, nx))
    act = np.concatenate([rng.normal(scale=0.5, size=hz[b] * nu) for b in range(B)])
    eps = np.concatenate([rng.normal(scale=0.7, size=n[b] * hz[b] * nu) for b in range(B)])
    plan.upload(x0=x0, act_seq=act, eps=eps)
    return h, plan


@pytest.mark.parametrize("term_mode", [0, 1])
def test_direct_plan_costs_in_both_terminal_modes_match_the_per_model_plans(term_mode):
    S = _six()
    models = [c["model"] for c in S["cands"]]
    idx, n, hz = [4, 1, 1], [33, 17, 16], [16, 5, 9]
    h, plan = _direct_plan(S["system"], models, idx, n, hz, term_mode)
    assert plan.info()["samples_per_wg"] == 16 and plan.info()["workgroups"] == 3 + 2 + 1
    plan.solve()
    a, u, c, _ = plan.download(costs=True)
    off = np.concatenate([[0], np.cumsum(n)])
    aoff = np.concatenate([[0], np.cumsum(np.array(hz) * 6)])
    for b in range(3):
        # the same problem alone, on a handle that holds its model, on the run-time-shape kernels
        hb, pb = _direct_plan(S["system"], models, idx, n, hz, term_mode, alone=idx[b])
        pb.solve()
        a1, u1, c1, _ = pb.download(costs=True)
        print("term_mode %d, problem %d: costs %.2e u %.2e" % (term_mode, b, rel_err(c[off[b]:off[b + 1]],
                                                                                      c1[off[b]:off[b + 1]]),
                                                                rel_err(u[b], u1[b])))
        np.testing.assert_allclose(c[off[b]:off[b + 1]], c1[off[b]:off[b + 1]], rtol=1e-9, atol=0)
        np.testing.assert_allclose(u[b], u1[b], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(a[aoff[b]:aoff[b + 1]], a1[aoff[b]:aoff[b + 1]], rtol=1e-9, atol=1e-12)
        pb.close()
        hb.close()
    plan.close()
    h.close()


# 6 ---------------------------------------------------------------------------------------------------------------
WIDE_U = [([24], "tanh", 21, 30), ([40, 17], "relu", 16, 11)]


@functools.lru_cache(maxsize=None)
def _wide_u():
    return _stack(8, 16, WIDE_U, seed=70)


@pytest.mark.parametrize("cap, fused", [(30, True), (40, False)])
def test_both_update_paths_match_the_oracle(cap, fused):
    """nx = 8, nu = 16: at a horizon cap of 30 the tile's clipped noise [30][16][16] fits the LDS map and the update
    runs through the tile partials (147 680 bytes); at a cap of 40 it does not (169 440 bytes) and the rollout writes
    eps_out for mppi_update_kernel."""
    from autompc_amd import _lib
    S = _wide_u()
    models = [c["model"] for c in S["cands"]]
    h, plan = _direct_plan(S["system"], models, [0, 1], [21, 16], [30, 11], 0, cap=cap)
    plan.set_outputs(keep_eps_out=False)
    plan.solve()
    if fused:          # the clipped noise never left the workgroup
        with pytest.raises(_lib.AmpcError, match="eps_out was not kept"):
            plan.download(eps_out=True)
    else:
        assert np.all(np.isfinite(plan.download(eps_out=True)[3]))
    plan.close()
    h.close()
    _against_the_oracle(S, _evaluator(S, horizon_cap=cap), 3, "nu = 16, horizon cap %d" % cap)


# 7 ---------------------------------------------------------------------------------------------------------------
def test_parameters_of_the_device_fit_are_read_in_place():
    from autompc_amd import MLP, _lib
    from autompc_amd.evaluation import model_metrics as MM
    from autompc_amd.sysid.mlp_fit import fit_mlps
    from autompc_amd.tuning import CandidateEvaluator
    from kstep_mlp_cases import synthetic_trajs
    s = make_system(3, 2)
    trajs = synthetic_trajs(s, seed=5)
    models = [MLP(s, n_hidden_layers=1, hidden_size_1=20, nonlintype="tanh", n_train_iters=3, n_batch=32, lr=1e-3, seed=1),
              MLP(s, n_hidden_layers=3, hidden_size_1=17, hidden_size_2=33, hidden_size_3=16, nonlintype="selu",
                  n_train_iters=3, n_batch=32, lr=3e-4, seed=2),
              MLP(s, n_hidden_layers=2, hidden_size_1=64, hidden_size_2=31, nonlintype="sigmoid", n_train_iters=3,
                  n_batch=32, lr=1e-3, seed=3)]
    for m in models:
        m.jit_kernels = False
    assert fit_mlps(models, trajs, fit="device")["device_models"] == 3
    twins = []
    for m in models:
        t = MLP(s, n_hidden_layers=len(m.hidden_sizes), nonlintype=m.nonlintype,
                **{"hidden_size_%d" % (i + 1): h for i, h in enumerate(m.hidden_sizes)})
        t.jit_kernels = False
        t.set_parameters(m.get_parameters())
        twins.append(t)
    for m in models:
        m._weights = m._biases = None                                       # (get_parameters fetched them)
    # the table a plan is given names the fit's own tensors
    h, plan = _direct_plan(s, twins, [0, 1, 2], [16, 20, 5], [4, 6, 3], 0)
    plan.set_model_table(models, [2, 0, 1])
    args = plan._table_args
    assert args["on_device"].tolist() == [1, 1, 1]
    for k, m in enumerate(models):
        for l in range(len(m.hidden_sizes) + 1):
            assert int(args["weights"][k, l]) == m._dev_params["w"][l].data_ptr()
            assert int(args["biases"][k, l]) == m._dev_params["b"][l].data_ptr()
        for i in range(4):
            assert int(args["norms"][k, i]) == m._dev_params["norm_dev"][i].data_ptr()
    plan.solve()
    assert np.all(np.isfinite(plan.download()[1]))
    plan.close()
    h.close()
    # twins that hold host copies of the same parameters score the same bits
    task = _task(s)
    cand = lambda m, i: dict(horizon=5 + i, sigma=0.4, lmda=0.7, num_path=20 + 7 * i, Q=np.ones(3), R=0.1 * np.ones(2),
                             F=np.ones(3), model=m)
    kw = dict(n_steps=T, seed=2, init_obs=np.array([0.1, -0.05, 0.02]))
    ev = CandidateEvaluator(s, task, twins[0], mlp_models="table")
    dev = ev.evaluate([cand(m, i) for i, m in enumerate(models)], **kw)
    assert ev.last_models == {"path": "table", "models": 3, "plans": 1}
    assert all(m._handle is None and m._weights is None for m in models)    # nothing was staged or fetched
    assert not MM.mlp_batch_args(twins)["on_device"].any()
    host = ev.evaluate([cand(m, i) for i, m in enumerate(twins)], **kw)
    mixed = ev.evaluate([cand(m, i) for i, m in enumerate([twins[0], models[1], twins[2]])], **kw)
    assert np.all(np.isfinite(dev))
    np.testing.assert_array_equal(host, dev)
    np.testing.assert_array_equal(mixed, dev)


# 8 ---------------------------------------------------------------------------------------------------------------
def test_declined_batches_return_exactly_the_default_result():
    from autompc_amd import QuadCost, ThresholdCost
    from autompc_amd.tuning import CandidateEvaluator
    S = _six()
    system = S["system"]
    cands = [S["cands"][i] for i in (0, 1, 3)]
    kw = dict(n_steps=2, seed=4, init_obs=S["init"])
    # an f32 evaluator (its models are f32 as well)
    c32 = [dict(c, model=_hip_model(system, S["params"][i], "f32")) for c, i in zip(cands, (0, 1, 3))]
    own32 = _hip_model(system, S["params"][0], "f32")
    out = {}
    for mode in ("table", "shape"):
        ev = CandidateEvaluator(system, S["task"], own32, precision="f32", mlp_models=mode)
        out[mode] = ev.evaluate(c32, **kw)
        assert ev.last_models == {"path": "shape", "models": 3, "plans": 3}
    np.testing.assert_array_equal(out["table"], out["shape"])
    # a task cost with a threshold term
    cost = QuadCost(system, np.eye(17), 0.01 * np.eye(6), np.eye(17)) + ThresholdCost(system, np.zeros(17), (0, 3), 0.05)
    for mode in ("table", "shape"):
        ev = _evaluator(S, mode, task=_task(system, cost))
        out[mode] = ev.evaluate(cands, **kw)
        assert ev.last_models == {"path": "shape", "models": 3, "plans": 3}
    np.testing.assert_array_equal(out["table"], out["shape"])
    # an LDS map over 160 KB (64 states, 16 controls, a horizon cap of 200): the library refuses with its code and
    # the batch goes the default way
    W = _stack(64, 16, [([16], "relu", 16, 3), ([20], "tanh", 8, 4)], seed=80)
    for mode in ("table", "shape"):
        ev = _evaluator(W, mode, horizon_cap=200, tile_rows=16)
        out[mode] = ev.evaluate(W["cands"], n_steps=1, seed=1, init_obs=W["init"])
        assert ev.last_models == {"path": "shape", "models": 2, "plans": 2}
    np.testing.assert_array_equal(out["table"], out["shape"])


def _refused(fn, text, code=-1):
    from autompc_amd import _lib
    with pytest.raises(_lib.AmpcError, match=text) as e:
        fn()
    assert e.value.code == code


def test_refusals_of_the_entry():
    from autompc_amd import MLP, _lib
    from autompc_amd.costs.terms import cost_terms
    from autompc_amd import QuadCost, ThresholdCost
    s = make_system(3, 2)
    mk = lambda hidden, act="tanh", sy=s, precision="f64", seed=1: _hip_model(
        sy, omlp.random_params(sy.obs_dim, sy.ctrl_dim, hidden, act, seed=seed), precision)
    a, b = mk([16]), mk([33, 17], "relu", seed=2)

    def fresh(model=a, precision="f64", horizon=5):
        h = _lib.Handle(0, precision, jit=False)
        model.stage_into(h)
        h.set_quad_costs(np.eye(3), 0.1 * np.eye(2), np.eye(3), np.zeros(3))
        h.set_ctrl_bounds(-np.ones(2), np.ones(2))
        return h, _lib.MppiPlan(h, [16, 20], horizon, 0.5, 1.0)

    h, plan = fresh()
    plan.set_model_table([a, b], [0, 1])                                     # (accepted: the cases below are refusals)
    assert plan.info()["samples_per_wg"] == 16 and plan.info()["workgroups"] == 3
    plan.set_geometry(0, 12)
    plan.set_geometry(16, 30)
    assert plan.info()["samples_per_wg"] == 16
    _refused(lambda: plan.set_geometry(32, 30), "tile_rows must be 0 or 16")
    _refused(lambda: plan.set_geometry(4, 30), "tile_rows must be 0 or 16")
    _refused(lambda: plan.set_model_table([a, b], [0, 2]), "model_index out of range")
    _refused(lambda: plan.set_model_table([a, b], [-1, 0]), "model_index out of range")
    _refused(lambda: plan.set_model_table([a, mk([16], sy=make_system(4, 2))], [0, 1]), "nx \\+ nu inputs and gives nx outputs")
    _refused(lambda: plan.set_model_table([a, mk([16], sy=make_system(3, 1))], [0, 1]), "nx \\+ nu inputs and gives nx outputs")
    _refused(lambda: plan.set_model_table([a, mk([257])], [0, 1]), "hidden widths must be in 1..256")
    # indicator terms set AFTER the table: refused at solve time; then at the next set_model_table
    ind = cost_terms(ThresholdCost(s, np.zeros(3), (0, 2), 0.1), 3, 2)
    h.set_indicator_costs(ind)
    _refused(plan.solve, "indicator cost terms")
    _refused(lambda: plan.set_model_table([a, b], [0, 1]), "indicator cost terms")
    h.set_indicator_costs(None)
    plan.upload(x0=np.zeros((2, 3)))
    plan.solve()                                                             # (and runs again without them)
    # per-problem models of one shape on a table plan, and the other way round
    _refused(lambda: plan.set_models([a._dev()], [0, 0]), "remove it first")
    plan.set_model_table(None, None)
    assert plan.info()["workgroups"] != 0
    # a state lift
    plan.set_state_lift([0], [1.0])
    _refused(lambda: plan.set_model_table([a, b], [0, 1]), "state lift")
    plan.close()
    h.close()
    # an f32 plan
    a32 = mk([16], precision="f32")
    h, plan = fresh(a32, "f32")
    _refused(lambda: plan.set_model_table([a, b], [0, 1]), "f64 only")
    plan.close()
    h.close()
    # a handle whose model is not an MLP
    h = _lib.Handle(0, "f64", jit=False)
    h.set_linear(0.9 * np.eye(70), np.ones((70, 2)))
    h.set_quad_costs(np.eye(70), 0.1 * np.eye(2), np.eye(70), np.zeros(70))
    h.set_ctrl_bounds(-np.ones(2), np.ones(2))
    plan = _lib.MppiPlan(h, [16, 20], 5, 0.5, 1.0)
    _refused(lambda: plan.set_model_table([a, b], [0, 1]), "not an MLP")
    plan.close()
    h.close()
    # an LDS map over 160 KB: its own code
    big = make_system(64, 16)
    m64 = mk([16], sy=big)
    h = _lib.Handle(0, "f64", jit=False)
    m64.stage_into(h)
    h.set_quad_costs(np.eye(64), 0.1 * np.eye(16), np.eye(64), np.zeros(64))
    h.set_ctrl_bounds(-np.ones(16), np.ones(16))
    plan = _lib.MppiPlan(h, [16], 5, 0.5, 1.0)
    plan.set_model_table([m64], [0])                                         # (148 640 bytes at the plan's own horizon)
    _refused(lambda: plan.set_geometry(16, 200), "more than 160 KB")
    plan.close()
    plan = _lib.MppiPlan(h, [16], 200, 0.5, 1.0)
    _refused(lambda: plan.set_model_table([m64], [0]), "more than 160 KB", _lib.MPPI_TABLE_NO_FIT)
    plan.close()
    h.close()


# 9 ---------------------------------------------------------------------------------------------------------------
def test_user_term_cond_in_segments_is_per_candidate_and_batch_invariant():
    """Candidates on four shapes that stop at different rows (a row count read off the size of the candidate's own first
    control, which follows its noise level), checked every two steps: the survivors' plan gets the table again, and every
    score and length equals the candidate's one-candidate evaluation with another segment length."""
    from autompc_amd import QuadCost, Task
    from autompc_amd.tuning import CandidateEvaluator
    nx, steps = 4, 12
    system = make_system(nx, 1)
    shapes = [([16], "relu"), ([33, 17], "tanh"), ([1, 40], "sigmoid"), ([255], "selu")]
    models = [_hip_model(system, golden_params(nx, 1, h, a, 50 + i, True)) for i, (h, a) in enumerate(shapes)]
    task = Task(system)
    task.set_cost(QuadCost(system, np.eye(nx), 0.01 * np.eye(1), np.eye(nx)))
    task.set_ctrl_bounds([-1.0], [1.0])
    task.set_init_obs(np.array([0.3, -0.2, 0.1, 0.05]))
    task.set_num_steps(steps)
    task.set_term_cond(lambda traj: len(traj) >= 3 + int(8.0 * abs(traj.ctrls[0, 0])))
    cands = [dict(horizon=6 + 2 * i, sigma=sg, lmda=0.5, num_path=24 + 9 * i, Q=np.ones(nx) * (1.0 + i),
                  R=np.array([0.01]), F=np.ones(nx), model=models[i]) for i, sg in enumerate([2.0, 0.6, 0.15, 0.01])]
    ev = CandidateEvaluator(system, task, models[0], term_check_every=2, mlp_models="table")
    s, obs, ctrls = ev.evaluate(cands, seed=3, return_trajectories=True)
    assert ev.last_models == {"path": "table", "models": 4, "plans": 1}
    lengths = ev.last_lengths.copy()
    print("rows per candidate:", lengths.tolist())
    assert len(set(lengths.tolist())) > 1 and lengths.max() <= steps + 1
    # (the setup: candidates leave at different segment boundaries, so the survivors' smaller plans really ran)
    assert len({(int(L) - 2) // 2 for L in lengths}) > 1
    for b, L in enumerate(lengths):
        assert np.all(np.isnan(obs[b, L:])) and np.all(np.isfinite(obs[b, :L]))
    ev1 = CandidateEvaluator(system, task, models[0], term_check_every=1, mlp_models="table")
    for b in range(len(cands)):
        alone = ev1.evaluate([cands[b]], seed=3, index_offset=b)
        assert ev1.last_models["path"] == "table"
        assert alone[0] == s[b] and ev1.last_lengths.tolist() == [lengths[b]]
