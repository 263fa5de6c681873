"""The host side of MPPI plans that hold MLP models of mixed shapes (ampc_mppi_plan_set_model_table,
tuning/batch_eval.py: ``mlp_models="table"``): the ABI, the refusal that needs no device, the option and the pure-Python
decision whether ONE plan takes a batch, and the conditioning of the candidates test_gpu_mppi_table.py holds to 1e-9
against the oracle.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

from autompc_amd import MLP, QuadCost, Task
from helpers import make_system

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _task(system, threshold=False):
    from autompc_amd import ThresholdCost
    nx, nu = system.obs_dim, system.ctrl_dim
    task = Task(system)
    cost = QuadCost(system, np.eye(nx), 0.01 * np.eye(nu), np.eye(nx))
    if threshold:
        cost = cost + ThresholdCost(system, goal=np.zeros(nx), threshold=0.5, obs_range=(0, 2))
    task.set_cost(cost)
    task.set_ctrl_bounds(-np.ones(nu), np.ones(nu))
    return task


def _cand(model=None):
    c = dict(horizon=5, sigma=0.5, lmda=1.0, num_path=16, Q=np.ones(3), R=np.ones(2), F=np.ones(3))
    if model is not None:
        c["model"] = model
    return c


def test_abi_exports_and_binds_the_entry():
    from autompc_amd import _lib
    from autompc_amd.csrc import build as B
    lib = ctypes.CDLL(B.build(verbose=False))
    assert hasattr(lib, "ampc_mppi_plan_set_model_table")
    assert len(_lib.SIGNATURES["ampc_mppi_plan_set_model_table"][1]) == 10
    header = open(os.path.join(ROOT, "include", "autompc_hip.h")).read()
    assert "ampc_mppi_plan_set_model_table(" in header
    units = {u[1]: u[2] for u in B.UNITS}
    assert units["launch_mppi_table.cpp"] == ["-DAMPC_T=double", "-DAMPC_T_IS_F64=1"]
    assert _lib.load().ampc_version() == 114
    assert hasattr(_lib.MppiPlan, "set_model_table") and _lib.MPPI_TABLE_NO_FIT == -3


def test_null_plan_is_refused_without_a_device():
    from autompc_amd import _lib
    lib = _lib.load()
    z = np.zeros(8, dtype=np.int32)
    rc = lib.ampc_mppi_plan_set_model_table(None, 1, _lib.iptr(z), _lib.iptr(z), _lib.iptr(z), None, None, None,
                                            _lib.iptr(z), _lib.iptr(z))
    assert rc != 0 and b"ampc_mppi_plan_set_model_table: NULL plan" in lib.ampc_last_error()
    rc = lib.ampc_mppi_plan_set_model_table(None, 0, None, None, None, None, None, None, None, None)
    assert rc != 0 and b"NULL plan" in lib.ampc_last_error()
    with pytest.raises(_lib.AmpcError) as e:
        _lib.check(rc)
    assert e.value.code == rc


def test_option_is_checked_and_the_default_is_shape():
    from autompc_amd.tuning import CandidateEvaluator
    s = make_system(3, 2)
    m = MLP(s, n_hidden_layers=1, hidden_size_1=16)
    ev = CandidateEvaluator(s, _task(s), m)
    assert ev.mlp_models == "shape" and ev.last_models is None
    assert CandidateEvaluator(s, _task(s), m, mlp_models="table").mlp_models == "table"
    for bad in ("bogus", None, "Table", 1):
        with pytest.raises(ValueError, match="mlp_models"):
            CandidateEvaluator(s, _task(s), m, mlp_models=bad)


def test_table_decision():
    from autompc_amd.tuning.batch_eval import table_decision
    s = make_system(3, 2)
    cost = _task(s).get_cost()
    kw = dict(precision="f64", device=0, task_cost=cost, obs_dim=3, ctrl_dim=2)
    own = MLP(s, n_hidden_layers=1, hidden_size_1=16)
    a = MLP(s, n_hidden_layers=2, hidden_size_1=256, hidden_size_2=1, nonlintype="tanh")
    b = MLP(s, n_hidden_layers=4, hidden_size=40, nonlintype="selu")
    # mixed shapes, a candidate without "model" (the evaluator's own), and one shape alone
    assert table_decision([_cand(a), _cand(b), _cand()], own, **kw) == (True, "")
    assert table_decision([_cand(), _cand()], own, **kw) == (True, "")
    assert table_decision([_cand(a)], own, **kw) == (True, "")
    # an f32 evaluator; an f32 model among f64 ones
    ok, why = table_decision([_cand(a)], own, **dict(kw, precision="f32"))
    assert not ok and "f64 only" in why
    ok, why = table_decision([_cand(a), _cand(MLP(s, n_hidden_layers=1, hidden_size_1=16, precision="f32"))], own, **kw)
    assert not ok and "not an f64 MLP" in why

    class Foreign(MLP):
        def pred_batch(self, states, ctrls):
            return states

    ok, why = table_decision([_cand(a), _cand(Foreign(s, n_hidden_layers=1, hidden_size_1=16))], own, **kw)
    assert not ok and "Foreign" in why
    # over the kernel's limits: width 257, five layers -- as a candidate's model and as the evaluator's own
    wide = MLP(s, n_hidden_layers=1, hidden_size_1=257)
    deep = MLP(s, n_hidden_layers=5, hidden_size=16)
    assert not table_decision([_cand(a), _cand(wide)], own, **kw)[0]
    assert not table_decision([_cand(a), _cand(deep)], own, **kw)[0]
    assert not table_decision([_cand(a), _cand()], wide, **kw)[0]
    assert table_decision([_cand(a)], wide, **kw)[0]           # (the evaluator's own model runs no candidate here)
    # two devices; models of another device than the evaluator's
    on1 = MLP(s, n_hidden_layers=1, hidden_size_1=16, device=1)
    ok, why = table_decision([_cand(a), _cand(on1)], own, **kw)
    assert not ok and "different devices" in why
    ok, why = table_decision([_cand(on1)], own, **kw)
    assert not ok and "another device" in why
    assert table_decision([_cand(on1)], own, **dict(kw, device=1))[0]
    # a task cost with an indicator term, a lifted controller model
    ok, why = table_decision([_cand(a)], own, **dict(kw, task_cost=_task(s, threshold=True).get_cost()))
    assert not ok and "indicator" in why
    ok, why = table_decision([_cand(a)], own, lift=([0], [1.0]), **kw)
    assert not ok and "lift" in why


def test_shape_groups_of_a_declined_batch_stay_on_the_default_path(monkeypatch):
    """A batch the table declines goes the "shape" way as a whole: its groups do not try the table again."""
    from autompc_amd.tuning import CandidateEvaluator
    s = make_system(3, 2)
    own = MLP(s, n_hidden_layers=1, hidden_size_1=16)
    ev = CandidateEvaluator(s, _task(s), own, mlp_models="table")
    seen = []

    def fake_evaluate(self_, cands, **kw):
        seen.append((self_.mlp_models, len(cands)))
        return np.zeros(len(cands))

    other = MLP(s, n_hidden_layers=1, hidden_size_1=257)
    import copy
    orig = copy.copy
    monkeypatch.setattr(copy, "copy", lambda o: _Sub(orig(o), fake_evaluate) if isinstance(o, CandidateEvaluator) else orig(o))
    out = ev.evaluate([_cand(), _cand(other), _cand(other)], n_steps=1)
    assert out.shape == (3,) and sorted(seen) == [("shape", 1), ("shape", 2)]
    assert ev.last_models == {"path": "shape", "models": 2, "plans": 2}


class _Sub:
    """A shape group's evaluator whose evaluate() is recorded instead of run (no GPU here)."""

    def __init__(self, ev, fn):
        object.__setattr__(self, "_ev", ev)
        object.__setattr__(self, "_fn", fn)

    def __getattr__(self, name):
        return getattr(self._ev, name)

    def __setattr__(self, name, value):
        setattr(self._ev, name, value)

    def evaluate(self, cands, **kw):
        return self._fn(self._ev, cands, **kw)


@pytest.mark.parametrize("which", ["sixteen", "forty_eight"])
def test_new_table_candidates_are_well_conditioned(which):
    """What a rounding-level restatement of the oracle -- every hidden layer's units in another order, so every sum in
    another order -- does to the closed loops test_gpu_mppi_table.py compares with at 1e-9: below 1e-12 on every
    candidate of the two further systems, so the 1e-9 holds three orders of allowance and no candidate sits on a
    switch of the softmin or of a clipped control."""
    import mppi_table_cases as C
    from helpers import rel_err
    from ilqr_table_cases import permuted
    S = getattr(C, which)()
    nu = S["system"].ctrl_dim
    acts, eps = C.fed_noise(S["cands"], nu, C.T)
    worst = 0.0
    for b in range(len(S["cands"])):
        obs, ctl, score = C.oracle_loop(S, b, C.T, acts, eps)
        obs_p, ctl_p, score_p = C.oracle_loop(S, b, C.T, acts, eps, p=permuted(S["params"][b]))
        dev = max(rel_err(obs_p, obs), rel_err(ctl_p, ctl), abs(score_p - score) / abs(score))
        print("%s, candidate %d: a permutation of the hidden units moves the oracle's loop by %.2e" % (which, b, dev))
        assert np.all(np.isfinite(obs)) and np.any(np.abs(ctl[:-1]) < 1.0) and np.any(ctl[:-1] != 0.0)
        worst = max(worst, dev)
    assert worst < 1e-12
