"""HoldoutModelEvaluator with MLPFactory against the reference's run (tests/golden/kstep_holdout.npz), and
BatchModelTuner against the evaluator called one configuration at a time.  Needs MI355X."""
import json

import numpy as np
import pytest

from conftest import golden
from helpers import make_system

pytestmark = pytest.mark.gpu


def _setup():
    from autompc_amd import MLPFactory, Trajectory
    from autompc_amd.evaluation import HoldoutModelEvaluator
    g = golden("kstep_holdout")
    system = make_system(int(g["nx"]), int(g["nu"]))
    trajs, o = [], 0
    for L in g["lens"]:
        L = int(L)
        trajs.append(Trajectory(system, L, g["obs"][o:o + L].copy(), g["ctrls"][o:o + L].copy()))
        o += L
    ev = HoldoutModelEvaluator(system, trajs, "rmse", np.random.default_rng(int(g["seed"])),
                               horizon=int(g["horizon"]), holdout_prop=float(g["holdout_prop"]))
    factory = MLPFactory(system, n_train_iters=int(g["n_train_iters"]), n_batch=int(g["n_batch"]))
    return system, ev, factory, g


def test_holdout_evaluator_reproduces_the_reference_run():
    """The MLP fits are pinned to the reference's at 1e-9 (mlpfit_*); the scores inherit that, hence 1e-7."""
    from autompc_amd.tuning import DictConfiguration
    _, ev, factory, g = _setup()
    assert ev.holdout_indices == [int(i) for i in g["holdout_idx"]]
    cfgs = [DictConfiguration(c) for c in json.loads(str(g["cfgs"]))]
    one = np.array([ev(factory, c) for c in cfgs])
    batch = ev.evaluate_batch(factory, cfgs)
    print("holdout scores: reference %s  one-by-one %s  batch %s" % (g["scores"], one, batch))
    np.testing.assert_allclose(one, g["scores"], rtol=1e-7, atol=0)
    np.testing.assert_allclose(batch, g["scores"], rtol=1e-7, atol=0)
    np.testing.assert_allclose(batch, one, rtol=1e-12, atol=0)


def test_batch_tuner_matches_one_configuration_at_a_time():
    from autompc_amd.evaluation import get_model_rmse
    from autompc_amd.tuning import BatchModelTuner
    system, ev, factory, _ = _setup()
    tuner = BatchModelTuner(system, ev, batch_size=8)
    tuner.add_model_factory(factory)
    model, res = tuner.run(np.random.default_rng(5), n_iters=16)
    assert len(res.cfgs) == 16 and len(res.costs) == 16
    single = []
    for c in res.cfgs:
        f, sub = tuner.model_config(c)
        s = float(ev(f, sub))
        single.append(s if np.isfinite(s) else float("inf"))
    print("tuner costs %s" % np.array(res.costs))
    np.testing.assert_allclose(res.costs, single, rtol=1e-12, atol=0)
    k = int(np.argmin(res.costs))
    assert res.inc_cfg is res.cfgs[k] and res.inc_costs[-1] == res.costs[k]
    # the incumbent trained on ALL trajectories
    _, sub = tuner.model_config(res.inc_cfg)
    ref = factory(sub, ev.trajs)
    assert model.hidden_sizes == ref.hidden_sizes and model.nonlintype == ref.nonlintype
    assert get_model_rmse(model, ev.holdout, 3) == get_model_rmse(ref, ev.holdout, 3)
