"""BatchModelTuner bookkeeping with a stub evaluator (no GPU): result fields, incumbent trace, combined keys,
the final model, and sharding over two gloo ranks."""
import os
import socket

import numpy as np
import pytest

from helpers import make_system


class StubFactory:
    name = "MLP"

    def __init__(self):
        self.calls = []

    def __call__(self, cfg, trajs, silent=False, skip_train_model=False):
        self.calls.append((dict(cfg.get_dictionary()), list(trajs)))
        return ("model", dict(cfg.get_dictionary()), len(trajs))


class StubEvaluator:
    """Scores a configuration by a fixed table keyed by hidden_size_1; NaN for one."""

    def __init__(self, trajs, table):
        self.trajs, self.table, self.seen = trajs, table, []

    def __call__(self, factory, cfg):
        self.seen.append(dict(cfg))
        return self.table[int(cfg["hidden_size_1"])]


def _cfg(h):
    from autompc_amd.tuning import DictConfiguration
    return DictConfiguration({"model": "MLP", "_MLP:nonlintype": "relu", "_MLP:n_hidden_layers": "1",
                              "_MLP:hidden_size_1": h, "_MLP:lr": 1e-3})


def _tuner(batch_size=2):
    from autompc_amd.tuning import BatchModelTuner
    system = make_system(2, 1)
    table = {16: 5.0, 17: 3.0, 18: float("nan"), 19: 3.0, 20: 1.0, 21: 2.0}
    ev = StubEvaluator(["t0", "t1", "t2"], table)
    tuner = BatchModelTuner(system, ev, batch_size=batch_size)
    factory = StubFactory()
    tuner.add_model_factory(factory)
    return tuner, factory, ev


def test_result_fields_and_incumbent_trace():
    from autompc_amd.tuning import ModelTuneResult
    assert ModelTuneResult._fields == ("inc_cfg", "cfgs", "inc_cfgs", "costs", "inc_costs")
    tuner, factory, ev = _tuner()
    cfgs = [_cfg(h) for h in (16, 17, 18, 19, 20, 21)]
    model, res = tuner.run(np.random.default_rng(0), n_iters=6, configs=cfgs)
    assert res.costs == [5.0, 3.0, float("inf"), 3.0, 1.0, 2.0]           # NaN recorded as inf
    assert res.inc_costs == [5.0, 3.0, 3.0, 3.0, 1.0, 1.0]
    # strict improvement only: the tie at 19 keeps 17
    assert [c["_MLP:hidden_size_1"] for c in res.inc_cfgs] == [16, 17, 17, 17, 20, 20]
    assert res.inc_cfg is cfgs[4] and res.cfgs == cfgs
    # the sub-configurations reached the evaluator with the prefix stripped
    assert ev.seen[0] == {"nonlintype": "relu", "n_hidden_layers": "1", "hidden_size_1": 16, "lr": 1e-3}
    # final model: the incumbent's sub-configuration trained on ALL of evaluator.trajs
    assert model == ("model", ev.seen[4], 3)
    assert factory.calls[-1][1] == ["t0", "t1", "t2"]


def test_sampled_configurations_carry_the_combined_keys():
    from autompc_amd import MLPFactory
    from autompc_amd.tuning import BatchModelTuner
    system = make_system(2, 1)
    tuner = BatchModelTuner(system, StubEvaluator([], {}))
    tuner.add_model_factory(MLPFactory(system))
    cfgs = tuner.ask(5, np.random.default_rng(3))
    for c in cfgs:
        d = c.get_dictionary()
        assert d["model"] == "MLP"
        assert {"_MLP:nonlintype", "_MLP:n_hidden_layers", "_MLP:lr", "_MLP:hidden_size_1"} <= set(d)
        assert all(k == "model" or k.startswith("_MLP:") for k in d)
        factory, sub = tuner.model_config(c)
        assert factory.name == "MLP" and "model" not in sub


def test_default_sampler_needs_a_known_factory():
    from autompc_amd.tuning import BatchModelTuner

    class Other:
        name = "Other"
    tuner = BatchModelTuner(make_system(2, 1), StubEvaluator([], {}))
    tuner.add_model_factory(Other())
    with pytest.raises(ValueError):
        tuner.ask(1, np.random.default_rng(0))


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        tuner, _, ev = _tuner(batch_size=4)
        cfgs = [_cfg(h) for h in (16, 17, 18, 19, 20, 21)]
        _, res = tuner.run(np.random.default_rng(0), n_iters=6, configs=cfgs)
        q.put((rank, res.costs, res.inc_costs, len(ev.seen)))
    finally:
        dist.destroy_process_group()


def test_two_rank_gloo_matches_single_process():
    import multiprocessing as mp
    tuner, _, _ = _tuner(batch_size=4)
    _, ref = tuner.run(np.random.default_rng(0), n_iters=6, configs=[_cfg(h) for h in (16, 17, 18, 19, 20, 21)])
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    out = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    seen = 0
    for rank, costs, inc_costs, n_seen in out:
        assert costs == ref.costs and inc_costs == ref.inc_costs
        seen += n_seen
    assert seen == 6                                   # every configuration scored once, on one rank
