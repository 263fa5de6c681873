"""The model-accuracy layer on the host: the reference's metrics over a pure-numpy model (the fallback every
model without a device path takes) and the holdout split, against tests/golden/kstep_*.npz."""
import json
import os

import numpy as np
import pytest

from helpers import make_system

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _trajs(system, g):
    from autompc_amd import Trajectory
    out, o = [], 0
    for L in g["lens"]:
        L = int(L)
        out.append(Trajectory(system, L, g["obs"][o:o + L].copy(), g["ctrls"][o:o + L].copy()))
        o += L
    return out


class NumpyLinear:
    """x' = A x + B u on the host (the generator's test double)."""

    def __init__(self, system, A, B):
        self.system, self.A, self.B = system, A, B

    def pred_batch(self, states, ctrls):
        return states @ self.A.T + ctrls @ self.B.T


def test_host_fallback_matches_reference_metrics():
    from autompc_amd.evaluation import get_model_rmse, get_model_rmsmens, model_errors
    g = np.load(os.path.join(GOLDEN, "kstep_numpy_linear.npz"))
    system = make_system(3, 2)
    trajs = _trajs(system, g)
    model = NumpyLinear(system, g["A"], g["B"])
    hs = [int(h) for h in g["horizons"]]
    rmse = np.array([get_model_rmse(model, trajs, horizon=h) for h in hs])
    rmsmens = np.array([get_model_rmsmens(model, trajs, horiz=h) for h in hs])
    np.testing.assert_allclose(rmse, g["rmse"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(rmsmens, g["rmsmens"], rtol=1e-12, atol=0)
    both = model_errors([model, model], trajs, hs, "rmse")
    assert both.shape == (2, len(hs))
    np.testing.assert_array_equal(both[0], rmse)
    np.testing.assert_array_equal(both[1], rmse)


def test_short_trajectories_contribute_nothing():
    from autompc_amd.evaluation import get_model_rmse, get_model_rmsmens
    g = np.load(os.path.join(GOLDEN, "kstep_numpy_linear.npz"))
    system = make_system(3, 2)
    trajs = _trajs(system, g)
    model = NumpyLinear(system, g["A"], g["B"])
    h = 20
    long_only = [t for t in trajs if len(t) > h]
    assert len(long_only) < len(trajs)
    assert get_model_rmse(model, trajs, h) == get_model_rmse(model, long_only, h)
    # (RMSMENS normalises by the increments of ALL given trajectories: same set, same value)
    assert np.isfinite(get_model_rmsmens(model, trajs, h))
    assert np.isnan(get_model_rmse(model, [t for t in trajs if len(t) <= h], h))


def test_rmsmens_refuses_a_model_whose_state_is_not_the_observation():
    from autompc_amd.evaluation import get_model_rmsmens, model_errors
    g = np.load(os.path.join(GOLDEN, "kstep_numpy_linear.npz"))
    system = make_system(3, 2)
    trajs = _trajs(system, g)
    model = NumpyLinear(system, g["A"], g["B"])
    model.traj_to_states = lambda traj: traj.obs
    with pytest.raises(ValueError):
        get_model_rmsmens(model, trajs, 1)
    with pytest.raises(ValueError):
        model_errors([model], trajs, [1], "mae")


def _holdout_evaluator(metric="rmse"):
    from autompc_amd.evaluation import HoldoutModelEvaluator
    g = np.load(os.path.join(GOLDEN, "kstep_holdout.npz"))
    system = make_system(int(g["nx"]), int(g["nu"]))
    trajs = _trajs(system, g)
    ev = HoldoutModelEvaluator(system, trajs, metric, np.random.default_rng(int(g["seed"])),
                               horizon=int(g["horizon"]), holdout_prop=float(g["holdout_prop"]))
    return ev, g, trajs


def test_holdout_split_matches_reference():
    ev, g, trajs = _holdout_evaluator()
    assert ev.holdout_indices == [int(i) for i in g["holdout_idx"]]
    assert all(h is trajs[i] for h, i in zip(ev.holdout, ev.holdout_indices))
    # the fixture's last trajectory equals (by value, not identity) a held-out one: excluded from training
    assert trajs[-1] is not trajs[2] and trajs[-1] == trajs[2] and 2 in ev.holdout_indices
    assert len(ev.training_set) == int(g["n_train"])
    assert all(not any(t is s for s in ev.training_set) for t in ev.holdout + [trajs[-1]])


def test_evaluator_metric_argument():
    ev, _, _ = _holdout_evaluator("rmsmens")
    assert ev.metric_name == "rmsmens"
    f = lambda model, trajs: 1.5                       # noqa: E731
    ev, _, _ = _holdout_evaluator(f)
    assert ev.metric is f and ev.metric_name is None
    for bad in ("mse", "RMSE", 3):
        with pytest.raises(ValueError):
            _holdout_evaluator(bad)


def test_holdout_configs_fixture_is_well_formed():
    g = np.load(os.path.join(GOLDEN, "kstep_holdout.npz"))
    cfgs = json.loads(str(g["cfgs"]))
    assert len(cfgs) == 3 == g["scores"].shape[0] and np.all(np.isfinite(g["scores"]))
