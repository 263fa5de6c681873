"""The host side of the iLQR plan that holds a table of SINDy models (no GPU): ``ilqr_sindy_table_decision``, the
evaluator's argument checks, the new entry's prototype, the body every entry of the cases takes, and the precondition
of the GPU tests' comparison of decisions -- every problem of tests/ilqr_sindy_table_cases.py keeps its acceptance
decisions, iteration count and ``converged`` flag under 1e-13 relative perturbations of its model's coefficients."""
import numpy as np
import pytest

import ilqr_sindy_table_cases as C
import mppi_sindy_table_cases as M
from autompc_amd import MLP, SINDy, System
from autompc_amd.tuning.batch_eval import ilqr_sindy_table_body, ilqr_sindy_table_decision


def _cand(model=None):
    c = dict(horizon=5, Q=np.ones(3), R=np.ones(2), F=np.ones(3))
    if model is not None:
        c["model"] = model
    return c


def test_ilqr_sindy_table_decision():
    s = System(["x0", "x1", "x2"], ["u0", "u1"], dt=0.05)
    own = SINDy(s)
    a, b = SINDy(s, trig_basis=True, trig_freq=2), SINDy(s, poly_basis=True, poly_degree=3, time_mode="continuous")
    assert ilqr_sindy_table_decision([_cand(a), _cand(b), _cand(), _cand(a)], own, "f64", 0, 3, 2) == (True, "")
    assert ilqr_sindy_table_decision([_cand(), _cand()], own) == (True, "")
    mlp = MLP(s, n_hidden_layers=1, hidden_size_1=8)
    ok, why = ilqr_sindy_table_decision([_cand(a), _cand(mlp)], own, "f64", 0, 3, 2)
    assert not ok and "MLP is not a SINDy model" in why
    ok, why = ilqr_sindy_table_decision([_cand(a), _cand()], mlp, "f64", 0, 3, 2)
    assert not ok and "not a SINDy model" in why                    # (a candidate without a model runs on the evaluator's)
    assert ilqr_sindy_table_decision([_cand(a), _cand(b)], mlp, "f64", 0, 3, 2) == (True, "")
    other = SINDy(System(["y0", "y1", "y2"], ["u0", "u1"], dt=0.05))
    ok, why = ilqr_sindy_table_decision([_cand(a), _cand(other)], own, "f64", 0, 3, 2)
    assert not ok and "another system" in why
    ok, why = ilqr_sindy_table_decision([_cand(a), _cand(SINDy(s, precision="f32"))], own, "f64", 0, 3, 2)
    assert not ok and "f32" in why
    ok, why = ilqr_sindy_table_decision([_cand(SINDy(s, precision="f32"))], SINDy(s, precision="f32"), "f32", 0, 3, 2)
    assert not ok and "f64 only" in why
    ok, why = ilqr_sindy_table_decision([_cand(SINDy(s, device=1))], own, "f64", 0, 3, 2)
    assert not ok and "another device" in why
    big = System(["x%d" % i for i in range(60)], ["u%d" % i for i in range(4)], dt=0.05)
    ok, why = ilqr_sindy_table_decision([_cand(SINDy(big))], SINDy(big), "f64", 0, 60, 4)
    assert not ok and "63" in why
    assert ilqr_sindy_table_decision([_cand(SINDy(big))], SINDy(big), "f64", 0, 60, 3) == (True, "")


def test_evaluator_checks_its_argument():
    from autompc_amd import QuadCost, Task
    from autompc_amd.tuning import IlqrCandidateEvaluator
    s = System(["x0", "x1", "x2"], ["u0", "u1"], dt=0.05)
    task = Task(s)
    task.set_cost(QuadCost(s, np.eye(3), np.eye(2), np.eye(3)))
    task.set_ctrl_bounds(-np.ones(2), np.ones(2))
    task.set_init_obs(np.zeros(3))
    assert IlqrCandidateEvaluator(s, task, SINDy(s)).sindy_models == "single"
    assert IlqrCandidateEvaluator(s, task, SINDy(s), sindy_models="table").sindy_models == "table"
    for bad in ("shape", "Table", None, 1):
        with pytest.raises(ValueError, match="sindy_models"):
            IlqrCandidateEvaluator(s, task, SINDy(s), sindy_models=bad)
    with pytest.raises(ValueError, match="one_plan"):
        IlqrCandidateEvaluator(s, task, SINDy(s), sindy_models="table", one_plan=False)


def test_prototype_of_the_new_entry():
    from ctypes import POINTER, c_int, c_void_p
    from autompc_amd import _lib
    assert _lib.SIGNATURES["ampc_ilqr_plan_set_sindy_models"] == (c_int, [c_void_p, c_int, POINTER(c_void_p)])
    assert hasattr(_lib.IlqrPlan, "set_sindy_models") and _lib.ILQR_TABLE_NO_FIT == -3


@pytest.mark.parametrize("name", sorted(C.PROBLEMS))
def test_the_body_every_entry_takes(name):
    system, ms, _, _ = M.models(name)
    assert tuple(ilqr_sindy_table_body(m) == "spread" for m in ms) == C.SPREAD[name]
    idx = C.model_index(name)
    assert set(idx.tolist()) == set(range(len(ms)))                 # every model is used ...
    assert min(np.bincount(idx)) >= 1 and max(np.bincount(idx)) >= 2   # ... and shared
    assert not np.all(np.diff(idx) >= 0)                            # non-monotonic
    assert int(C.horizons(name).max()) == C.PLAN_H and int(C.horizons(name).min()) == 2
    if name == "c1":
        for m, hyper in C.extra_models():
            assert ilqr_sindy_table_body(m) == "spread"
    if name == "pair":                                              # more than eight states; the unstaged program
        assert system.obs_dim > 8 and ms[1].library[0].shape[0] == 1081


@pytest.mark.parametrize("name", sorted(C.PROBLEMS))
def test_every_problem_is_finite_and_keeps_its_decisions_under_perturbation(name):
    """The oracle's solve of every listed problem: finite, the listed (converged, iterations), and under three 1e-13
    relative perturbations of the coefficients the same decisions, iteration count and flag, with trajectories that
    move by less than 1e-10 -- an amplification below 1000, so that rounding-level differences (1e-16) between two
    correct evaluations of one model stay four orders below the GPU tests' 1e-9."""
    _, ms, _, _ = M.models(name)
    idx = C.model_index(name)
    worst = 0.0
    for j, (tag, b, hz, conv, iters) in enumerate(C.PROBLEMS[name]):
        base = C.solves(name)[j]
        for key in ("states", "ctrls", "Ks", "ks"):
            assert np.all(np.isfinite(base[key])), (name, j, key)
        assert np.isfinite(base["obj"])
        assert (base["converged"], base["iters"]) == (conv, iters), (name, j, base["converged"], base["iters"])
        Xi = ms[int(idx[j])].coefficients
        for seed in range(3):
            rng = np.random.default_rng(100 * j + seed)
            pert = C.solve(name, j, Xi * (1.0 + 1e-13 * rng.uniform(-1.0, 1.0, size=Xi.shape)))
            assert pert["decisions"] == base["decisions"], (name, j, seed)
            assert (pert["converged"], pert["iters"]) == (base["converged"], base["iters"]), (name, j, seed)
            moved = max(float(np.max(np.abs(pert["states"] - base["states"]))),
                        float(np.max(np.abs(pert["ctrls"] - base["ctrls"]))))
            worst = max(worst, moved)
    print("%s: trajectories moved by at most %.2e under 1e-13 perturbations" % (name, worst))
    assert worst < 1e-10


def test_the_evaluators_batch_is_finite_on_the_cpu():
    S = C.batch()
    assert len({id(c["model"]) for c in S["cands"]}) == 5 and len(S["cands"]) == 6
    for kind in ("sindy", "mlp"):
        for loop in C.oracle_loops(kind):
            assert np.all(np.isfinite(loop["obs"])) and np.all(np.isfinite(loop["ctrls"])) and np.isfinite(loop["score"])
