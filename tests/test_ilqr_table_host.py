"""The host side of iLQR plans that hold MLP models of mixed shapes (ampc_ilqr_plan_set_model_table,
tuning/batch_eval.py: ``IlqrCandidateEvaluator(mlp_models="table")``): the ABI, the refusal that needs no device, the
option, the pure-Python decision whether ONE plan takes a batch, and how far a rounding-level change of the summation
order moves the candidates that test_gpu_ilqr_table.py compares against the oracle.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

import ilqr_table_cases as cases
from autompc_amd import MLP
from helpers import make_system

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cand(model=None):
    c = dict(horizon=5, Q=np.ones(3), R=np.ones(2), F=np.ones(3))
    if model is not None:
        c["model"] = model
    return c


def test_abi_exports_and_binds_the_entry():
    from autompc_amd import _lib
    from autompc_amd.csrc import build as B
    lib = ctypes.CDLL(B.build(verbose=False))
    assert hasattr(lib, "ampc_ilqr_plan_set_model_table")
    assert len(_lib.SIGNATURES["ampc_ilqr_plan_set_model_table"][1]) == 9
    header = open(os.path.join(ROOT, "include", "autompc_hip.h")).read()
    assert "ampc_ilqr_plan_set_model_table(" in header
    units = {u[1]: u[2] for u in B.UNITS}
    assert units["launch_ilqr_table.cpp"] == ["-DAMPC_T=double", "-DAMPC_T_IS_F64=1"]
    assert _lib.load().ampc_version() == 114
    assert hasattr(_lib.IlqrPlan, "set_model_table") and _lib.ILQR_TABLE_NO_FIT == -3


def test_null_plan_is_refused_without_a_device():
    from autompc_amd import _lib
    lib = _lib.load()
    z = np.zeros(8, dtype=np.int32)
    rc = lib.ampc_ilqr_plan_set_model_table(None, 1, _lib.iptr(z), _lib.iptr(z), _lib.iptr(z), None, None, None,
                                            _lib.iptr(z))
    assert rc != 0 and b"ampc_ilqr_plan_set_model_table: NULL plan" in lib.ampc_last_error()
    rc = lib.ampc_ilqr_plan_set_model_table(None, 0, None, None, None, None, None, None, None)
    assert rc != 0 and b"NULL plan" in lib.ampc_last_error()
    with pytest.raises(_lib.AmpcError) as e:
        _lib.check(rc)
    assert e.value.code == rc


def test_option_is_checked_and_the_default_is_shape():
    from autompc_amd.tuning import IlqrCandidateEvaluator
    s = make_system(3, 2)
    m = MLP(s, n_hidden_layers=1, hidden_size_1=16)
    task = cases.make_task(s)
    ev = IlqrCandidateEvaluator(s, task, m)
    assert ev.mlp_models == "shape" and ev.last_models is None
    assert IlqrCandidateEvaluator(s, task, m, mlp_models="table").mlp_models == "table"
    for bad in ("bogus", None, "Table", 1):
        with pytest.raises(ValueError, match="mlp_models"):
            IlqrCandidateEvaluator(s, task, m, mlp_models=bad)
    with pytest.raises(ValueError, match="one_plan"):
        IlqrCandidateEvaluator(s, task, m, mlp_models="table", one_plan=False)
    assert IlqrCandidateEvaluator(s, task, m, one_plan=False).mlp_models == "shape"


class _Recorder:
    """A table evaluation recorded instead of run (no GPU here)."""

    def __init__(self):
        self.calls = []

    def __call__(self, ev, candidates, n_steps, init_obs, return_trajectories, max_iter, opened):
        self.calls.append((ev._table, ev.mlp_models, len(candidates)))
        ev.last_lengths = None
        return np.zeros(len(candidates))


def test_the_decision_routes_the_batch(monkeypatch):
    """Mixed shapes go as one table plan; a non-MLP model, nx + nu = 64 and models of another device or system go the
    default way, each for its reason; an f32 evaluator does not exist (iLQR solves in f64) and the decision says no."""
    from autompc_amd.tuning import IlqrCandidateEvaluator
    from autompc_amd.tuning.batch_eval import ilqr_table_decision, table_decision
    s = make_system(3, 2)
    own = MLP(s, n_hidden_layers=1, hidden_size_1=16)
    a = MLP(s, n_hidden_layers=2, hidden_size_1=256, hidden_size_2=1, nonlintype="tanh")
    b = MLP(s, n_hidden_layers=4, hidden_size=40, nonlintype="selu")
    kw = dict(precision="f64", device=0, task_cost=None, obs_dim=3, ctrl_dim=2)
    assert table_decision([_cand(a), _cand(b), _cand()], own, **kw) == (True, "")
    ok, why = table_decision([_cand(a)], own, **dict(kw, precision="f32"))
    assert not ok and "f64 only" in why
    with pytest.raises(ValueError, match="f64"):
        IlqrCandidateEvaluator(s, cases.make_task(s), own, precision="f32", mlp_models="table")

    class Foreign(MLP):
        def pred_batch(self, states, ctrls):
            return states

    ok, why = table_decision([_cand(a), _cand(Foreign(s, n_hidden_layers=1, hidden_size_1=16))], own, **kw)
    assert not ok and "Foreign" in why
    on1 = MLP(s, n_hidden_layers=1, hidden_size_1=16, device=1)
    ok, why = table_decision([_cand(a), _cand(on1)], own, **kw)
    assert not ok and "different devices" in why
    ok, why = table_decision([_cand(on1)], own, **kw)
    assert not ok and "another device" in why
    other = MLP(make_system(4, 2), n_hidden_layers=1, hidden_size_1=16)
    ok, why = table_decision([_cand(a), _cand(other)], own, **kw)
    assert not ok and ("systems" in why or "not an f64 MLP" in why)

    # what the evaluator does with the answer
    rec = _Recorder()
    monkeypatch.setattr(IlqrCandidateEvaluator, "_evaluate", lambda self, *args: rec(self, *args))
    shape_runs = []
    from autompc_amd.tuning import CandidateEvaluator
    monkeypatch.setattr(CandidateEvaluator, "_evaluate_shape_groups",
                        lambda self, groups, cands, ids, kw_: shape_runs.append(len(groups)) or np.ones(len(cands)))
    ev = IlqrCandidateEvaluator(s, cases.make_task(s), own, mlp_models="table")
    out = ev.evaluate([_cand(a), _cand(b), _cand()], n_steps=1)
    assert out.tolist() == [0.0, 0.0, 0.0] and rec.calls == [(True, "table", 3)] and not shape_runs
    assert ev.last_models == {"path": "table", "models": 3, "plans": 1}
    out = ev.evaluate([_cand(a), _cand(Foreign(s, n_hidden_layers=1, hidden_size_1=16)), _cand()], n_steps=1)
    assert out.tolist() == [1.0, 1.0, 1.0] and len(rec.calls) == 1 and shape_runs == [3]
    assert ev.last_models == {"path": "shape", "models": 3, "plans": 3}
    # 48 + 16 = 64 inputs: inside the table kernels' limits, over the sweep's
    big = make_system(48, 16)
    mb = MLP(big, n_hidden_layers=1, hidden_size_1=16)
    mb2 = MLP(big, n_hidden_layers=1, hidden_size_1=32)
    cb = lambda m: dict(horizon=5, Q=np.ones(48), R=np.ones(16), F=np.ones(48), model=m)
    assert table_decision([cb(mb), cb(mb2)], mb, **dict(kw, obs_dim=48, ctrl_dim=16)) == (True, "")
    ok, why = ilqr_table_decision([cb(mb), cb(mb2)], mb, "f64", 0, 48, 16)
    assert not ok and "63" in why
    assert ilqr_table_decision([_cand(a), _cand(b), _cand()], own, "f64", 0, 3, 2) == (True, "")
    evb = IlqrCandidateEvaluator(big, cases.make_task(big), mb, mlp_models="table")
    evb.evaluate([cb(mb), cb(mb2)], n_steps=1)
    assert len(rec.calls) == 1 and evb.last_models == {"path": "shape", "models": 2, "plans": 2}


def test_a_library_refusal_with_the_no_fit_code_falls_back_to_the_default_path(monkeypatch):
    """Code -3 (the kernel's LDS map) sends the batch the default way; any other refusal is raised."""
    from autompc_amd import _lib
    from autompc_amd.tuning import CandidateEvaluator, IlqrCandidateEvaluator
    s = make_system(3, 2)
    own = MLP(s, n_hidden_layers=1, hidden_size_1=16)
    a = MLP(s, n_hidden_layers=2, hidden_size_1=32, hidden_size_2=8)
    codes = []

    def refuse(self, *args):
        if self._table:
            err = _lib.AmpcError("ampc_ilqr_plan_set_model_table: refused")
            err.code = codes[-1]
            raise err
        return np.full(len(args[0]), 2.0)

    monkeypatch.setattr(IlqrCandidateEvaluator, "_evaluate", refuse)
    monkeypatch.setattr(CandidateEvaluator, "_evaluate_shape_groups",
                        lambda self, groups, cands, ids, kw_: np.full(len(cands), 3.0))
    ev = IlqrCandidateEvaluator(s, cases.make_task(s), own, mlp_models="table")
    codes.append(_lib.ILQR_TABLE_NO_FIT)
    assert ev.evaluate([_cand(a), _cand()], n_steps=1).tolist() == [3.0, 3.0]
    assert ev.last_models == {"path": "shape", "models": 2, "plans": 2}
    assert ev.evaluate([_cand(), _cand()], n_steps=1).tolist() == [2.0, 2.0]
    assert ev.last_models == {"path": "shape", "models": 1, "plans": 1}
    codes.append(-1)
    with pytest.raises(_lib.AmpcError, match="refused"):
        ev.evaluate([_cand(a), _cand()], n_steps=1)


def _dev(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


def test_the_shared_candidates_do_not_amplify_rounding():
    """For exactly the candidates of the GPU tests (ilqr_table_cases.six: these shapes, horizons, max_iter = 8, bounds
    +-1, three control steps), ILQROracle on each model and on a hidden-unit permutation of it -- which changes every
    summation order, as another kernel does: acceptance decisions, iteration counts and `converged` are identical,
    trajectories and gains move by less than 1e-12 relative to max(1, |.|).  Measured here: decisions identical, largest
    movement 1.1e-15."""
    S = cases.six()
    worst = 0.0
    for b, ref in enumerate(cases.six_loops()):
        alt = cases.oracle_loop(S, b, cases.permuted(S["params"][b]))
        for s, (r, a) in enumerate(zip(ref["solves"], alt["solves"])):
            assert (r["converged"], r["iters"], r["decisions"]) == (a["converged"], a["iters"], a["decisions"]), (b, s)
            d = max(_dev(a[k], r[k]) for k in ("states", "ctrls", "Ks", "ks"))
            worst = max(worst, d)
        worst = max(worst, _dev(alt["obs"], ref["obs"]), _dev(alt["ctrls"], ref["ctrls"]))
        print("candidate %d: iterations %s converged %s" % (b, [r["iters"] for r in ref["solves"]],
                                                            [r["converged"] for r in ref["solves"]]))
    print("largest movement under a hidden-unit permutation: %.2e" % worst)
    assert worst < 1e-12
