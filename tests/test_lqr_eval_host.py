"""LQR pipeline tuning without a GPU: configuration <-> candidate mapping, the samplers, the work weights and the
tuner's LQR dispatch (a fake evaluator stands in for the device)."""
import numpy as np
import pytest

from autompc_amd import ARXFactory, KoopmanFactory, QuadCost, System, Task
from autompc_amd.tuning import (BatchPipelineTuner, LqrCandidateEvaluator, candidate_work, lqr_candidate_from_config,
                                random_lqr_candidates, sample_arx_config, sample_koopman_config,
                                sample_lqr_pipeline_configs)
from autompc_amd.tuning import batch_tuner as bt
from autompc_amd.tuning.configs import DictConfiguration, candidate_from_config, config_from_candidate


def _system(no=3, nu=2):
    return System(["x%d" % i for i in range(no)], ["u%d" % i for i in range(nu)], dt=0.05)


def _gains(s, v=1.0):
    d = {"_cost:%s_Q" % n: v for n in s.observations}
    d.update({"_cost:%s_F" % n: 2 * v for n in s.observations})
    d.update({"_cost:%s_R" % n: 3 * v for n in s.controls})
    return d


def test_config_candidate_round_trip_finite_and_infinite():
    s = _system()
    fin = DictConfiguration(_gains(s), **{"_ctrlr:finite_horizon": "true", "_ctrlr:horizon": 250,
                                          "_model:history": 3})
    c = lqr_candidate_from_config(s, fin)
    assert c["controller"] == "lqr" and c["finite_horizon"] is True and c["horizon"] == 250
    assert c["model_cfg"] == {"history": 3}
    np.testing.assert_array_equal(c["Q"], np.ones(3))
    np.testing.assert_array_equal(c["R"], 3 * np.ones(2))
    assert config_from_candidate(s, c) is fin                        # reported back unchanged
    c.pop("cfg")
    assert dict(config_from_candidate(s, c)) == dict(fin)
    inf = DictConfiguration(_gains(s), **{"_ctrlr:finite_horizon": "false"})
    c = lqr_candidate_from_config(s, inf)
    assert c["finite_horizon"] is False and "horizon" not in c
    c.pop("cfg")
    back = config_from_candidate(s, c)
    assert dict(back) == dict(inf) and "_ctrlr:horizon" not in back
    # a bool works as the categorical's value; a finite configuration needs its horizon
    assert lqr_candidate_from_config(s, {**_gains(s), "_ctrlr:finite_horizon": True, "_ctrlr:horizon": 1})["horizon"] == 1
    with pytest.raises(KeyError, match="horizon"):
        lqr_candidate_from_config(s, {**_gains(s), "_ctrlr:finite_horizon": "true"})
    with pytest.raises(KeyError, match="finite_horizon"):
        lqr_candidate_from_config(s, {**_gains(s), "_ctrlr:horizon": 5})


def test_candidate_from_config_still_refuses_lqr():
    s = _system()
    with pytest.raises(NotImplementedError, match="finite_horizon"):
        candidate_from_config(s, {**_gains(s), "_ctrlr:finite_horizon": "true", "_ctrlr:horizon": 5})


def test_samplers_ranges_and_conditional_keys():
    rng = np.random.default_rng(0)
    arx = [sample_arx_config(rng)["history"] for _ in range(400)]
    assert min(arx) == 1 and max(arx) == 10
    seen = {"lstsq": 0, "lasso": 0}
    for _ in range(400):
        k = sample_koopman_config(rng)
        seen[k["method"]] += 1
        assert ("lasso_alpha" in k) == (k["method"] == "lasso")
        assert ("poly_degree" in k) == (k["poly_basis"] == "true")
        assert ("trig_freq" in k) == (k["trig_basis"] == "true")
        assert k["product_terms"] == "false"
        if "lasso_alpha" in k:
            assert 1e-10 <= k["lasso_alpha"] <= 1e2
        if "poly_degree" in k:
            assert 2 <= k["poly_degree"] <= 8
        if "trig_freq" in k:
            assert 1 <= k["trig_freq"] <= 8
    assert seen["lstsq"] > 0 and seen["lasso"] > 0            # never "stable"
    s = _system()
    for model, key in ((None, None), ("arx", "_model:history"), ("koopman", "_model:method")):
        cfgs = sample_lqr_pipeline_configs(s, 200, rng, model=model)
        hz = []
        for c in cfgs:
            assert c["_ctrlr:finite_horizon"] in ("true", "false")
            assert ("_ctrlr:horizon" in c) == (c["_ctrlr:finite_horizon"] == "true")
            if "_ctrlr:horizon" in c:
                hz.append(c["_ctrlr:horizon"])
            assert all(1e-3 <= c[k] <= 1e4 for k in c if k.startswith("_cost:"))
            assert len([k for k in c if k.startswith("_cost:")]) == 2 * s.obs_dim + s.ctrl_dim
            if key is None:
                assert not any(k.startswith("_model:") for k in c)
            else:
                assert key in c
        assert 1 <= min(hz) and max(hz) <= 1000 and max(hz) > 500
    with pytest.raises(ValueError):
        sample_lqr_pipeline_configs(s, 1, rng, model="mlp")
    cands = random_lqr_candidates(s, 300, seed=3)
    fin = [c for c in cands if c["finite_horizon"]]
    assert 0 < len(fin) < 300 and all("horizon" not in c for c in cands if not c["finite_horizon"])
    assert min(c["horizon"] for c in fin) >= 1 and max(c["horizon"] for c in fin) <= 1000
    assert all(c["controller"] == "lqr" for c in cands)


def test_lqr_work_weights():
    s = _system()

    class M:
        state_dim, system = 10, s
    c = {"controller": "lqr", "finite_horizon": True, "horizon": 8, "model": M()}
    assert candidate_work(c) == 10.0 * 100 * 12
    assert candidate_work({"controller": "lqr", "finite_horizon": "false"}) == 1.0
    # MPPI / iLQR weights unchanged
    assert candidate_work({"horizon": 7, "num_path": 100}) == 700.0
    assert candidate_work({"horizon": 7}) == 7.0


class _FakeLqr(LqrCandidateEvaluator):
    """The tuner-facing surface of LqrCandidateEvaluator with a host score: inf for infinite horizons, else the
    candidate's first Q gain (a model must have been fitted and attached)."""

    def __init__(self, system, task):
        self.system, self.task, self.model, self.surrogate, self.device = system, task, None, None, 0
        self.precision, self.goal = "f64", np.zeros(system.obs_dim)
        self.umin, self.umax = -np.ones(system.ctrl_dim), np.ones(system.ctrl_dim)
        self.last_lengths, self.host_fallbacks, self.seen = None, 0, []

    def evaluate(self, candidates, n_steps=None, seed=0, init_obs=None, return_trajectories=False, index_offset=0):
        self.seen.extend(candidates)
        out = []
        for c in candidates:
            assert c.get("model") is not None
            out.append(float(c["Q"][0]) if c["finite_horizon"] else float("inf"))
        return np.array(out)


def _task(s):
    t = Task(s)
    t.set_cost(QuadCost(s, np.eye(s.obs_dim), np.eye(s.ctrl_dim), np.eye(s.obs_dim)))
    t.set_num_steps(10)
    return t


def _trajs(s):
    from autompc_amd import Trajectory
    rng = np.random.default_rng(1)
    return [Trajectory(s, 30, rng.normal(size=(30, s.obs_dim)), rng.normal(size=(30, s.ctrl_dim))) for _ in range(3)]


def test_tuner_dispatch_samples_lqr_with_arx_models(monkeypatch):
    s = _system()
    ev = _FakeLqr(s, _task(s))

    def no_mlp(rng):
        raise AssertionError("sample_mlp_config must not be called for LQR pipelines")
    monkeypatch.setattr(bt, "sample_mlp_config", no_mlp)
    tuner = BatchPipelineTuner(s, ev, batch_size=8, model_factory=ARXFactory(s), trajs=_trajs(s), as_configs=True)
    inc, res = tuner.run(20, np.random.default_rng(0))
    assert len(res.costs) == 20 and len(ev.seen) == 20
    assert all(c["controller"] == "lqr" and set(c["model_cfg"]) == {"history"} for c in ev.seen)
    assert tuner.models_fitted == len({c["model_cfg"]["history"] for c in ev.seen})
    finite = [c for c in ev.seen if c["finite_horizon"]]
    assert 0 < len(finite) < 20
    for c, cost in zip(ev.seen, res.costs):
        assert cost == (float(c["Q"][0]) if c["finite_horizon"] else float("inf"))
    best = min(res.costs)
    assert res.inc_costs[-1] == best and np.isfinite(best)
    assert np.all(np.diff(res.inc_costs) <= 0)
    # the incumbent is reported as a configuration that maps back to an LQR candidate
    cand = lqr_candidate_from_config(s, inc)
    assert cand["finite_horizon"] and "_model:history" in inc and float(cand["Q"][0]) == best


def test_tuner_dispatch_koopman_and_configs():
    s = _system()
    ev = _FakeLqr(s, _task(s))
    tuner = BatchPipelineTuner(s, ev, batch_size=4, model_factory=KoopmanFactory(s), trajs=_trajs(s))
    cands = tuner.ask(6, np.random.default_rng(2))
    assert all(set(c["model_cfg"]) >= {"method", "poly_basis", "trig_basis"} for c in cands)
    cfgs = sample_lqr_pipeline_configs(s, 6, np.random.default_rng(3), model="arx")
    inc, res = BatchPipelineTuner(s, _FakeLqr(s, _task(s)), batch_size=4, model_factory=ARXFactory(s),
                                  trajs=_trajs(s)).run(6, np.random.default_rng(4), configs=cfgs)
    assert all(a is b for a, b in zip(res.cfgs, cfgs))
    assert any(inc is c for c in cfgs)
    assert lqr_candidate_from_config(s, inc)["controller"] == "lqr"


def test_tuner_without_lqr_evaluator_keeps_mlp_sampling(monkeypatch):
    calls = []
    real = bt.sample_mlp_config
    monkeypatch.setattr(bt, "sample_mlp_config", lambda rng: calls.append(1) or real(rng))

    class Ev:
        def evaluate(self, cands, **kw):
            return np.zeros(len(cands))
    s = _system()
    tuner = BatchPipelineTuner(s, Ev(), batch_size=4, model_factory=ARXFactory(s), trajs=_trajs(s))
    cands = tuner.ask(3, np.random.default_rng(0))
    assert len(calls) == 3 and all("num_path" in c for c in cands)
