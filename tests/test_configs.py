"""Pipeline configurations <-> evaluator candidates (tuning/configs.py), and the tuner's model axis
(``BatchPipelineTuner(model_factory=..., trajs=...)``: a model built and FITTED per configuration, as
``eval_cfg`` does through ``pipeline(cfg, task, trajs)``, pipeline.py:138-145).  CPU: host logic; the
evaluator is a stand-in that reads the candidate's fitted model."""
import json
import os

import numpy as np
import pytest

from autompc_amd import MLP, zeros
from autompc_amd.sysid.mlp import MLPFactory
from autompc_amd.tuning import (BatchPipelineTuner, DictConfiguration, candidate_from_config,
                                candidates_from_configs, config_from_candidate, random_candidates,
                                random_ilqr_candidates, sample_pipeline_configs)
from helpers import make_system


class _Configuration:
    """What the evaluators may rely on of ConfigSpace's Configuration: get_dictionary()."""

    def __init__(self, d):
        self._d = dict(d)

    def get_dictionary(self):
        return dict(self._d)


def test_512_sampled_configurations_round_trip_with_the_references_key_names():
    system = make_system(4, 2)
    cfgs = sample_pipeline_configs(system, 512, np.random.default_rng(0), model_axis=True)
    keys = set(cfgs[0])
    assert {"_ctrlr:horizon", "_ctrlr:sigma", "_ctrlr:lmda", "_ctrlr:num_path", "_cost:x0_Q", "_cost:x3_F",
            "_cost:u1_R", "_model:nonlintype", "_model:n_hidden_layers", "_model:hidden_size_1", "_model:lr"} <= keys
    cands = candidates_from_configs(system, [_Configuration(c) for c in cfgs])
    for cfg, c in zip(cfgs, cands):
        assert 5 <= c["horizon"] <= 30 and 100 <= c["num_path"] <= 1000 and 1e-4 <= c["sigma"] <= 2.0
        assert c["Q"].shape == (4,) and c["R"].shape == (2,) and np.all(c["Q"] >= 1e-3) and np.all(c["F"] <= 1e4)
        assert c["Q"][2] == cfg["_cost:x2_Q"] and c["R"][1] == cfg["_cost:u1_R"]
        depth = int(c["model_cfg"]["n_hidden_layers"])
        assert isinstance(c["model_cfg"]["n_hidden_layers"], str)           # the reference's categorical holds strings
        assert sorted(k for k in c["model_cfg"] if k.startswith("hidden_size")) == ["hidden_size_%d" % (i + 1) for i in range(depth)]
        # the candidate -> configuration direction, without the ride-along object
        back = config_from_candidate(system, {k: v for k, v in c.items() if k != "cfg"})
        assert back.get_dictionary() == dict(cfg)
    assert config_from_candidate(system, cands[3]) is cands[3]["cfg"]


def test_absent_gains_are_zero_and_ilqr_configurations_have_no_mppi_keys():
    system = make_system(3, 1)
    c = candidate_from_config(system, {"_ctrlr:horizon": 12, "_cost:x0_Q": 2.0, "_cost:u0_R": 0.5})
    assert "num_path" not in c and c["horizon"] == 12
    np.testing.assert_array_equal(c["Q"], [2.0, 0.0, 0.0])                 # quad_cost_factory.py:76-79
    np.testing.assert_array_equal(c["F"], [0.0, 0.0, 0.0])
    with pytest.raises(KeyError):
        candidate_from_config(system, {"_ctrlr:horizon": 12, "_ctrlr:sigma": 1.0})
    with pytest.raises(KeyError):
        candidate_from_config(system, {"_cost:x0_Q": 1.0})
    for cand in random_candidates(system, 5, seed=1) + random_ilqr_candidates(system, 5, seed=1):
        again = candidate_from_config(system, config_from_candidate(system, cand))
        for k in cand:
            np.testing.assert_array_equal(again[k], cand[k])
    with pytest.raises(ValueError):
        config_from_candidate(system, dict(horizon=5, Q=np.ones((3, 3)), R=np.ones(1), F=np.ones(3)))


class _ModelReadingEvaluator:
    """score = a statistic of the candidate's controller model (so a wrong / untrained model shows)."""

    def __init__(self, default):
        self.model, self.calls = default, []

    def evaluate(self, candidates, seed=0, index_offset=0):
        self.calls.append(index_offset)
        return np.array([float(sum(np.abs(w).sum() for w in (c.get("model") or self.model).weights))
                         + 1e-3 * c["horizon"] for c in candidates])


def _trajs(system, n=3, rows=40, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        t = zeros(system, rows)
        t.obs[:] = 0.1 * rng.normal(size=(rows, system.obs_dim)).cumsum(axis=0)
        t.ctrls[:] = rng.normal(size=(rows, system.ctrl_dim))
        out.append(t)
    return out


def test_tuner_runs_given_configurations_and_reports_them_back():
    system = make_system(3, 2)
    cfgs = [_Configuration(c) for c in sample_pipeline_configs(system, 512, np.random.default_rng(1))]
    ev = _ModelReadingEvaluator(MLP(system, n_hidden_layers=1, hidden_size=16))
    tuner = BatchPipelineTuner(system, ev, batch_size=64)
    assert tuner.balance is False              # a plain evaluator gets the documented integer index_offset
    best, res = tuner.run(512, np.random.default_rng(0), configs=cfgs)      # BASELINE config 5's 512 pipelines
    assert ev.calls == list(range(0, 512, 64))
    assert all(a is b for a, b in zip(res.cfgs, cfgs)) and best is cfgs[int(np.argmin(res.costs))]
    assert {"_ctrlr:horizon", "_ctrlr:num_path", "_cost:x0_Q", "_cost:u1_R"} <= set(best.get_dictionary())
    assert res.inc_cfgs[-1] is best and len(res.costs) == 512
    with pytest.raises(ValueError):
        tuner.run(513, np.random.default_rng(0), configs=cfgs)
    # sampled candidates reported as configurations on request
    t2 = BatchPipelineTuner(system, ev, batch_size=8, as_configs=True)
    best2, res2 = t2.run(8, np.random.default_rng(0))
    assert isinstance(best2, DictConfiguration) and set(best2) >= {"_ctrlr:num_path", "_cost:x1_F", "_cost:u0_R"}


def test_model_axis_fits_a_model_per_configuration_in_lockstep_groups_and_caches_them():
    system = make_system(3, 2)
    trajs = _trajs(system)
    cfgs = sample_pipeline_configs(system, 24, np.random.default_rng(2), model_axis=True)
    for c in cfgs[12:]:                         # the second half repeats the first half's models
        for k in [k for k in c if k.startswith("_model:")]:
            del c[k]
    for a, b in zip(cfgs[:12], cfgs[12:]):
        b.update({k: v for k, v in a.items() if k.startswith("_model:")})
    default = MLP(system, n_hidden_layers=1, hidden_size=16)
    ev = _ModelReadingEvaluator(default)
    factory = MLPFactory(system, n_train_iters=1, n_batch=32)
    tuner = BatchPipelineTuner(system, ev, batch_size=12, model_factory=factory, trajs=trajs)
    best, res = tuner.run(24, np.random.default_rng(0), configs=cfgs)
    assert tuner.models_fitted == 12 and tuner.fit_seconds > 0.0 and tuner.eval_seconds > 0.0
    # every score came from THE configuration's model, fitted as MLP(...).train(trajs) fits it
    for cfg, cost in list(zip(cfgs, res.costs))[::5]:
        c = candidate_from_config(system, cfg)
        m = factory(DictConfiguration(c["model_cfg"]), trajs)
        assert m.hidden_sizes == [int(c["model_cfg"]["hidden_size_%d" % (i + 1)]) for i in range(len(m.hidden_sizes))]
        want = float(sum(np.abs(w).sum() for w in m.weights)) + 1e-3 * c["horizon"]
        assert abs(cost - want) < 1e-9 * want
    assert "_model:lr" in best.get_dictionary()
    # the default sampler draws the model sub-configuration itself
    t2 = BatchPipelineTuner(system, ev, batch_size=6, model_factory=factory, trajs=trajs, as_configs=True)
    best2, res2 = t2.run(6, np.random.default_rng(3))
    assert t2.models_fitted == 6 and "_model:nonlintype" in best2
    with pytest.raises(ValueError):
        BatchPipelineTuner(system, ev, model_factory=factory)
    with pytest.raises(ValueError):
        BatchPipelineTuner(system, ev).run(4, np.random.default_rng(0), configs=cfgs[:4])


def test_configurations_mean_to_the_references_factories_what_they_mean_here():
    """The reference's REAL QuadCostFactory / MLPFactory called the way Pipeline.__call__ calls them
    (pipeline.py:138-166) on the sub-configurations of sampled configurations, as recorded in
    tests/golden/config_factories.json (gen_golden.gen_config_factories): the cost it built has the candidate's
    Q / R / F, the model it built has the candidate's layer sizes."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "config_factories.json")) as f:
        recorded = json.load(f)
    cfgs = sample_pipeline_configs(make_system(4, 2), 6, np.random.default_rng(5), model_axis=True)
    assert len(recorded) == len(cfgs) == 6
    for cfg, rec in zip(cfgs, recorded):
        assert dict(cfg) == rec["config"]                   # the configurations the reference was given
        cand = candidate_from_config(make_system(4, 2), cfg)
        np.testing.assert_array_equal(np.array(rec["Q"]), np.diag(cand["Q"]))
        np.testing.assert_array_equal(np.array(rec["R"]), np.diag(cand["R"]))
        np.testing.assert_array_equal(np.array(rec["F"]), np.diag(cand["F"]))
        ours = MLPFactory(make_system(4, 2))(DictConfiguration(cand["model_cfg"]), [], skip_train_model=True)
        assert rec["hidden_sizes"] == ours.hidden_sizes


def _axis_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    system = make_system(3, 2)
    trajs = _trajs(system)
    cfgs = sample_pipeline_configs(system, 10, np.random.default_rng(7), model_axis=True)
    ev = _ModelReadingEvaluator(MLP(system, n_hidden_layers=1, hidden_size=16))
    ev.accepts_global_ids = True                         # (it ignores index_offset: balanced shards are fine)
    tuner = BatchPipelineTuner(system, ev, batch_size=10, model_factory=MLPFactory(system, n_train_iters=1, n_batch=32),
                               trajs=trajs)
    best, res = tuner.run(10, np.random.default_rng(0), configs=cfgs)
    q.put((rank, list(res.costs), tuner.models_fitted, cfgs.index(best)))
    dist.destroy_process_group()


def test_two_ranks_fit_only_their_own_shards_models_and_agree_on_the_scores():
    """The model axis under torch.distributed (gloo, world 2): every rank builds and fits the models of ITS shard
    only (pipeline.py:138-145 runs inside the sharded evaluation), the all-gathered scores are the single-process
    scores."""
    import torch.multiprocessing as mp
    from test_sharded_eval import _free_port
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_axis_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = {r: (c, n, b) for r, c, n, b in (q.get(timeout=300) for _ in range(2))}
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    system = make_system(3, 2)
    trajs = _trajs(system)
    cfgs = sample_pipeline_configs(system, 10, np.random.default_rng(7), model_axis=True)
    ev = _ModelReadingEvaluator(MLP(system, n_hidden_layers=1, hidden_size=16))
    single = BatchPipelineTuner(system, ev, batch_size=10, model_factory=MLPFactory(system, n_train_iters=1, n_batch=32),
                                trajs=trajs)
    best, res = single.run(10, np.random.default_rng(0), configs=cfgs)
    assert single.models_fitted == 10
    for r in range(2):
        np.testing.assert_allclose(got[r][0], res.costs, rtol=1e-12)
        assert got[r][2] == cfgs.index(best)
    assert got[0][1] + got[1][1] == 10 and 3 <= got[0][1] <= 7       # each rank fitted its shard's models only
