"""The host side of the MPPI plan that holds a table of linear models of mixed state dimension (no GPU):
``linear_table_decision``, the evaluator's constructor argument, the tuner's model sub-space, the bindings, and the
precondition of the bitwise GPU tests -- every rollout of tests/mppi_linear_table_cases.py has a finite cost on the
CPU."""
import numpy as np
import pytest

import mppi_linear_table_cases as C
from autompc_amd import ARX, MLP, Koopman, SINDy, System
from autompc_amd.tuning.batch_eval import linear_table_decision


def _system():
    return System(["x0", "x1", "x2"], ["u0", "u1"], dt=0.05)


def _cand(model=None):
    c = dict(horizon=5, sigma=0.5, lmda=0.5, num_path=8, Q=np.ones(3), R=np.ones(2), F=np.ones(3))
    if model is not None:
        c["model"] = model
    return c


def _arx(s, history, **kw):
    m = ARX(s, history=history, **kw)
    rng = np.random.default_rng(history)
    m.set_parameters({"coeffs": 0.1 * rng.normal(size=(s.obs_dim, m._get_fvec_size()))})
    return m


def _koop(s, **kw):
    m = Koopman(s, **kw)
    n = m.state_dim
    m.set_parameters({"A": 0.5 * np.eye(n), "B": 0.1 * np.ones((n, s.ctrl_dim))})
    return m


def test_linear_table_decision():
    s = _system()
    own = _arx(s, 2)
    a, b = _arx(s, 1), _arx(s, 10)
    k = _koop(s, poly_basis="true", poly_degree=3, trig_basis="true", trig_freq=2)
    ident = _koop(s)
    assert linear_table_decision([_cand(a), _cand(k), _cand(), _cand(b), _cand(ident)], own) == (True, "")
    assert linear_table_decision([_cand(), _cand()], own, "f64", 0, 3) == (True, "")
    # an MLP or a SINDy model in the batch -- carried by a candidate, or the evaluator's own standing in
    mlp = MLP(s, n_hidden_layers=1, hidden_size_1=16)
    ok, why = linear_table_decision([_cand(a), _cand(mlp)], own)
    assert not ok and "MLP is not an ARX or Koopman model" in why
    ok, why = linear_table_decision([_cand(a), _cand(SINDy(s))], own)
    assert not ok and "SINDy is not an ARX or Koopman model" in why
    ok, why = linear_table_decision([_cand(a), _cand()], mlp)
    assert not ok and "not an ARX or Koopman model" in why
    assert linear_table_decision([_cand(a), _cand(k)], mlp) == (True, "")    # (nobody runs on the evaluator's own)
    # an untrained model
    ok, why = linear_table_decision([_cand(a), _cand(ARX(s, history=3))], own)
    assert not ok and "not trained" in why
    ok, why = linear_table_decision([_cand(Koopman(s))], own)
    assert not ok and "not trained" in why
    # product terms
    ok, why = linear_table_decision([_cand(_koop(s, poly_basis="true", poly_degree=2, product_terms="true"))], own)
    assert not ok and "product terms" in why
    # another system, precision, device
    ok, why = linear_table_decision([_cand(a), _cand(_arx(System(["y0", "y1", "y2"], ["u0", "u1"], dt=0.05), 2))], own)
    assert not ok and "another system" in why
    ok, why = linear_table_decision([_cand(a), _cand(_arx(s, 2, precision="f32"))], own)
    assert not ok and "f32" in why
    ok, why = linear_table_decision([_cand(a)], own, precision="f32")
    assert not ok and "f32" in why
    assert linear_table_decision([_cand(_arx(s, 2, precision="f32"))], _arx(s, 3, precision="f32"), precision="f32")[0]
    ok, why = linear_table_decision([_cand(_arx(s, 2, device=1))], own)
    assert not ok and "device" in why
    # 257 states: 3 observations x (1 + 42 + 2 * 21 + ...) -- an ARX of history 52 has 1 + 52 * 3 + 51 * 2 = 259
    wide = _arx(s, 52)
    assert wide.state_dim > 256
    ok, why = linear_table_decision([_cand(wide)], own)
    assert not ok and "more than 256" in why
    big = Koopman(s, trig_basis="true", trig_freq=43, strict_reference=False)      # 3 * (1 + 86) = 261
    big.set_parameters({"A": np.zeros((big.state_dim,) * 2), "B": np.zeros((big.state_dim, 2))})
    ok, why = linear_table_decision([_cand(big)], own)
    assert not ok and "more than 256" in why


def _task(s):
    from autompc_amd import QuadCost, Task
    task = Task(s)
    task.set_cost(QuadCost(s, np.eye(3), np.eye(2), np.eye(3)))
    task.set_ctrl_bounds(-np.ones(2), np.ones(2))
    task.set_init_obs(np.zeros(3))
    task.set_num_steps(5)
    return task


def test_evaluator_checks_its_argument():
    from autompc_amd.tuning import CandidateEvaluator
    s = _system()
    task = _task(s)
    own = _arx(s, 2)
    assert CandidateEvaluator(s, task, own).linear_models == "shape"
    assert CandidateEvaluator(s, task, own, linear_models="table").linear_models == "table"
    for bad in ("single", "Table", None, 1):
        with pytest.raises(ValueError, match="linear_models"):
            CandidateEvaluator(s, task, own, linear_models=bad)
    # an ARX controller model with a surrogate that is not itself: refused by default, taken under "table"
    mlp = MLP(s, n_hidden_layers=1, hidden_size_1=16)
    with pytest.raises(TypeError, match="score such candidates with simulate"):
        CandidateEvaluator(s, task, own, surrogate=mlp)
    ev = CandidateEvaluator(s, task, own, surrogate=mlp, linear_models="table")
    # ... and a batch that does not take the table gets the constructor's refusal from evaluate()
    with pytest.raises(TypeError, match="score such candidates with simulate"):
        ev.evaluate([_cand(), _cand(mlp)], n_steps=2)


def test_tuner_draws_linear_model_configurations_for_a_table_evaluator():
    from autompc_amd.sysid.linear import ARXFactory, KoopmanFactory
    from autompc_amd.tuning import BatchPipelineTuner, CandidateEvaluator
    s = _system()
    task = _task(s)
    mlp = MLP(s, n_hidden_layers=1, hidden_size_1=16)
    trajs = []
    ev = CandidateEvaluator(s, task, _arx(s, 2), surrogate=mlp, linear_models="table")
    tuner = BatchPipelineTuner(s, ev, model_factory=ARXFactory(s), trajs=trajs)
    cands = tuner.ask(12, np.random.default_rng(0))
    assert all(set(c["model_cfg"]) == {"history"} and 1 <= c["model_cfg"]["history"] <= 10 for c in cands)
    assert len({c["model_cfg"]["history"] for c in cands}) > 1
    tuner = BatchPipelineTuner(s, ev, model_factory=KoopmanFactory(s), trajs=trajs)
    cands = tuner.ask(12, np.random.default_rng(0))
    assert all("method" in c["model_cfg"] and "poly_basis" in c["model_cfg"] for c in cands)
    # the default evaluator keeps what the tuner did before
    ev0 = CandidateEvaluator(s, task, mlp)
    tuner = BatchPipelineTuner(s, ev0, model_factory=ARXFactory(s), trajs=trajs)
    assert all("history" not in c["model_cfg"] for c in tuner.ask(4, np.random.default_rng(0)))


def test_prototypes_of_the_new_entries():
    from ctypes import POINTER, c_double, c_int, c_uint64, c_void_p
    from autompc_amd import _lib
    ip, dp = POINTER(c_int), POINTER(c_double)
    assert _lib.SIGNATURES["ampc_mppi_plan_set_linear_models"] == (
        c_int, [c_void_p, c_int, POINTER(c_void_p), ip, ip, ip, ip, dp])
    assert _lib.SIGNATURES["ampc_mppi_closed_loop_linear"] == (
        c_int, [c_void_p, c_void_p, dp, dp, c_int, c_uint64, dp, c_int, ip, dp, dp, dp, dp])
    assert hasattr(_lib.MppiPlan, "set_linear_models") and hasattr(_lib.MppiPlan, "closed_loop_linear")
    lib = _lib.load()                                   # (the library exports them)
    assert lib.ampc_mppi_plan_set_linear_models and lib.ampc_mppi_closed_loop_linear


@pytest.mark.parametrize("name", sorted(C.SETS))
def test_every_rollout_of_the_cases_is_finite_on_the_cpu(name):
    system, ab = C.matrices(name)
    d = C.plan_data(name)
    s = C.SETS[name]
    assert len(ab) == len(s["nx"])
    assert set(d["index"].tolist()) == set(range(len(ab) - 1))           # every model but the spare is used
    assert not np.all(np.diff(d["index"]) >= 0)                          # non-monotonic
    assert int(d["H"].max()) == C.HORIZON_CAP and int(d["H"].min()) == 2
    assert all(x.shape == (s["nx"][k],) for x, k in zip(d["x0"], d["index"]))
    clipped = 0
    for b, (costs, eps, act) in enumerate(C.cpu_rollouts(name)):
        assert costs.shape == (int(d["N"][b]),) and np.all(np.isfinite(costs)), (name, b)
        assert np.all(np.isfinite(eps)) and np.all(np.isfinite(act))
        clipped += int(np.sum(eps != np.transpose(d["eps"][b], (1, 0, 2))))
    assert clipped > 0                                                   # the bounds bite somewhere


def test_the_sets_cover_the_kernel_paths_they_name():
    e, w, k4 = C.SETS["edges"], C.SETS["wide"], C.SETS["k4"]
    assert [C.ksn(n, e["nu"]) for n in e["nx"][:5]] == [2, 3, 5, 5, 5]
    assert [(n + 15) // 16 for n in e["nx"][:5]] == [1, 1, 1, 1, 2]
    assert [C.ksn(n, k4["nu"]) for n in k4["nx"][:2]] == [2, 4]
    assert w["nx"][:5] == (62, 64, 65, 130, 256) and (130 + 15) // 16 > 8
