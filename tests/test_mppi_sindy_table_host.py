"""The host side of the MPPI plan that holds a table of SINDy models (no GPU): ``sindy_table_decision``, the
evaluator's constructor argument, and the precondition of the bitwise GPU tests -- every rollout of
tests/mppi_sindy_table_cases.py has a finite cost on the CPU."""
import numpy as np
import pytest

import mppi_sindy_table_cases as C
from autompc_amd import MLP, SINDy, System
from autompc_amd.tuning.batch_eval import sindy_table_decision


def _cand(model=None):
    c = dict(horizon=5, sigma=0.5, lmda=0.5, num_path=8, Q=np.ones(3), R=np.ones(2), F=np.ones(3))
    if model is not None:
        c["model"] = model
    return c


def test_sindy_table_decision():
    s = System(["x0", "x1", "x2"], ["u0", "u1"], dt=0.05)
    own = SINDy(s)
    a = SINDy(s, trig_basis=True, trig_freq=2, trig_interaction=True, time_mode="continuous")
    b = SINDy(s, poly_basis=True, poly_degree=3, poly_cross_terms=True)
    assert sindy_table_decision([_cand(a), _cand(b), _cand(), _cand(a)], own) == (True, "")
    assert sindy_table_decision([_cand(), _cand()], own, "f64", 0, None) == (True, "")
    # an MLP in the batch -- carried by a candidate, or the evaluator's own standing in for a candidate without one
    mlp = MLP(s, n_hidden_layers=1, hidden_size_1=16)
    ok, why = sindy_table_decision([_cand(a), _cand(mlp)], own)
    assert not ok and "MLP is not a SINDy model" in why
    ok, why = sindy_table_decision([_cand(a), _cand()], mlp)
    assert not ok and "not a SINDy model" in why
    assert sindy_table_decision([_cand(a), _cand(b)], mlp) == (True, "")     # (nobody runs on the evaluator's own)
    # another system
    other = SINDy(System(["y0", "y1", "y2"], ["u0", "u1"], dt=0.05))
    ok, why = sindy_table_decision([_cand(a), _cand(other)], own)
    assert not ok and "another system" in why
    # a lift
    ok, why = sindy_table_decision([_cand(a)], own, lift=([0], [0.0]))
    assert not ok and "lift" in why
    # another precision, another device
    ok, why = sindy_table_decision([_cand(a), _cand(SINDy(s, precision="f32"))], own)
    assert not ok and "f32" in why
    ok, why = sindy_table_decision([_cand(a)], own, precision="f32")
    assert not ok and "f32" in why
    assert sindy_table_decision([_cand(SINDy(s, precision="f32"))], SINDy(s, precision="f32"), precision="f32")[0]
    ok, why = sindy_table_decision([_cand(SINDy(s, device=1))], own)
    assert not ok and "device" in why


def test_evaluator_checks_its_argument():
    from autompc_amd import QuadCost, Task
    from autompc_amd.tuning import CandidateEvaluator
    s = System(["x0", "x1", "x2"], ["u0", "u1"], dt=0.05)
    task = Task(s)
    task.set_cost(QuadCost(s, np.eye(3), np.eye(2), np.eye(3)))
    task.set_ctrl_bounds(-np.ones(2), np.ones(2))
    task.set_init_obs(np.zeros(3))
    assert CandidateEvaluator(s, task, SINDy(s)).sindy_models == "single"
    assert CandidateEvaluator(s, task, SINDy(s), sindy_models="table").sindy_models == "table"
    for bad in ("shape", "Table", None, 1):
        with pytest.raises(ValueError, match="sindy_models"):
            CandidateEvaluator(s, task, SINDy(s), sindy_models=bad)


def test_prototype_of_the_new_entry():
    from ctypes import POINTER, c_int, c_void_p
    from autompc_amd import _lib
    assert _lib.SIGNATURES["ampc_mppi_plan_set_sindy_models"] == (c_int, [c_void_p, c_int, POINTER(c_void_p),
                                                                          POINTER(c_int)])
    assert hasattr(_lib.MppiPlan, "set_sindy_models")


@pytest.mark.parametrize("name", sorted(C.SETS))
def test_every_rollout_of_the_cases_is_finite_on_the_cpu(name):
    system, ms, _, _ = C.models(name)
    d = C.plan_data(name)
    assert len(ms) == len(C.SETS[name]["tags"]) == len(C.SPREAD[name])
    assert set(d["index"].tolist()) == set(range(len(ms)))               # every model is used ...
    assert max(np.bincount(d["index"])) >= 2                             # ... one at least twice
    assert not np.all(np.diff(d["index"]) >= 0)                          # non-monotonic
    assert int(d["H"].max()) == C.HORIZON_CAP and int(d["H"].min()) == 2
    clipped = 0
    for b, (costs, eps, act) in enumerate(C.cpu_rollouts(name)):
        assert costs.shape == (int(d["N"][b]),) and np.all(np.isfinite(costs)), (name, b)
        assert np.all(np.isfinite(eps)) and np.all(np.isfinite(act))
        clipped += int(np.sum(eps != np.transpose(d["eps"][b], (1, 0, 2))))
    assert clipped > 0                                                   # the bounds bite somewhere


@pytest.mark.parametrize("name", ["trio"])
def test_indicator_terms_of_the_cases_tell_rollouts_apart(name):
    """The threshold / box terms (the GPU test puts them on the trio: lane-spread and one-thread entries) are violated
    by some states the plan visits and not by others (the initial states: the terms are charged on every stage's
    state, the first one included)."""
    kinds, params = C.indicator_terms(name)
    assert sorted(int(k) for k in kinds) == [1, 2]
    x0 = C.plan_data(name)["x0"]
    nx = x0.shape[1]
    thr = np.max(np.abs(x0[:, :2]), axis=1) > 0.25
    lim = np.tile([-0.3, 0.35], (nx, 1))
    lim[0, 0], lim[nx - 1, 1] = -np.inf, np.inf
    box = np.any((x0 < lim[:, 0]) | (x0 > lim[:, 1]), axis=1)
    assert len({(bool(a), bool(b)) for a, b in zip(thr, box)}) >= 2
