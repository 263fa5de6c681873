"""ampc_bo_propose (csrc/bo_kernels.hpp) against the long-double yardstick of tests/bo_cases.py: panel and tile edges
of the factorisation and the solve, dimension, pool and pick edges, the hyperparameter table's rules, duplicated and
tied data, one mid-size case for the multi-block paths, the limits, determinism, and the tuner end to end on the
device (needs MI355X)."""
import functools

import numpy as np
import pytest

import bo_cases as bc

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _device(name):
    from autompc_amd import _lib
    c = bc.CASES[name]
    return _lib.bo_propose(c["X"], c["z"], c["hyper_w"], c["hyper_noise"], c["pool"], c["q"])


@pytest.mark.parametrize("name", bc.SMALL_CASES)
def test_device_against_the_long_double_reference(name):
    """n in {1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100} (d = 9, G = 3, pool 70, q = 8); d in {1, 2, 64} (n = 33);
    m in {1, 63, 64, 65, 257} with q in {1, min(m, 16)} and m = q = 5; G in {1, 24, 64}; a declined row, twin rows,
    every row declined; duplicated X, tied z, a cluster of identical pool points."""
    bc.check_result(name, _device(name))


def test_hyperparameter_table_rules():
    a, b = _device("declined_between"), _device("declined_without")
    assert list(a["status"]) == [0, 1, 0] and np.isneginf(a["lml"][1])
    assert a["chosen"] == (0, 2)[b["chosen"]]
    for key in ("picks", "pick_ei", "pick_margin", "mu", "var"):      # the call without the declined row, bit for bit
        np.testing.assert_array_equal(a[key], b[key])
    np.testing.assert_array_equal(a["lml"][[0, 2]], b["lml"])
    twins = _device("twin_rows")
    assert twins["lml"][0] == twins["lml"][1] > twins["lml"][2] and twins["chosen"] == 0
    none = _device("all_declined")                                     # statuses, no picks, no fault
    assert list(none["status"]) == [1, 1] and none["chosen"] == -1 and np.all(none["picks"] == -1)
    assert np.all(np.isnan(none["mu"])) and np.all(np.isnan(none["pick_ei"]))
    assert sorted(_device("m5_q5")["picks"]) == [0, 1, 2, 3, 4]


def test_mid_size_case_and_determinism():
    """n = 513, d = 13, G = 24, m = 4096, q = 64: seventeen panels, 64 pool blocks, the default table; a second call
    gives the same bits in every output."""
    from autompc_amd import _lib
    first = _device("mid")
    bc.check_result("mid", first)
    c = bc.CASES["mid"]
    again = _lib.bo_propose(c["X"], c["z"], c["hyper_w"], c["hyper_noise"], c["pool"], c["q"])
    assert again["chosen"] == first["chosen"]
    for key in ("lml", "status", "picks", "pick_ei", "pick_margin", "mu", "var"):
        assert np.array_equal(first[key], again[key]), key


def test_limits_are_refused_with_a_message():
    from autompc_amd import _lib
    X, z, P = np.zeros((3, 2)), np.zeros(3), np.zeros((4, 2))
    w, s = np.ones((1, 2)), np.full(1, 0.1)
    for word, args in [("n ", (np.zeros((2049, 2)), np.zeros(2049), w, s, P, 1)),
                       ("d ", (np.zeros((3, 65)), z, np.ones((1, 65)), s, np.zeros((4, 65)), 1)),
                       ("n_hyper", (X, z, np.ones((65, 2)), np.full(65, 0.1), P, 1)),
                       ("m ", (X, z, w, s, np.zeros((65537, 2)), 1)),
                       ("q ", (X, z, w, s, np.zeros((300, 2)), 257)),
                       ("q ", (X, z, w, s, P, 5))]:
        with pytest.raises(_lib.AmpcError, match="ampc_bo_propose: " + word):
            _lib.bo_propose(*args)


@pytest.mark.parametrize("kind", ["mppi", "ilqr"])
def test_tuner_end_to_end_on_the_device(kind):
    """BatchPipelineTuner with a device GpProposer on the Pendulum-sized MLP workload, three batches of 16: candidates in
    range, a random batch and then GP batches, the result filled as without a proposer; a numpy-backend run on the same
    seed picks the same candidates wherever the reported pick margin exceeds the tolerance (as a ratio: twice the
    case's EI tolerance over the pick's EI)."""
    from autompc_amd.synthetic import make_workload
    from autompc_amd.tuning import (BatchPipelineTuner, CandidateEvaluator, GpProposer, IlqrCandidateEvaluator,
                                    PipelineTuneResult)
    system, task, model, _ = make_workload("c2")
    task.set_num_steps(8)
    ev = (CandidateEvaluator if kind == "mppi" else IlqrCandidateEvaluator)(system, task, model)

    class Recording(GpProposer):
        def propose(self, X, z, pool, q):
            res = GpProposer.propose(self, X, z, pool, q)
            self.calls.append((dict(X=X, z=z, hyper_w=self.hyper_w, hyper_noise=self.hyper_noise, pool=pool, q=q), res))
            return res

    runs = {}
    for backend in ("device", "numpy"):
        prop = Recording(system, kind, backend=backend, pool=512)
        prop.calls, paths = [], []
        tuner = BatchPipelineTuner(system, ev, batch_size=16, proposer=prop)
        rng = np.random.default_rng(9)
        orig = tuner.ask

        def ask(n, rng, orig=orig, prop=prop, paths=paths):
            out = orig(n, rng)
            paths.append(prop.last["path"])
            return out
        tuner.ask = ask
        best, res = tuner.run(48, rng, seed=3)
        runs[backend] = (prop, res)
        assert paths == ["random", "gp", "gp"] and prop.declined_batches == 0
        assert isinstance(res, PipelineTuneResult) and best is res.inc_cfg
        assert len(res.cfgs) == len(res.costs) == len(res.inc_cfgs) == len(res.inc_costs) == 48
        assert res.inc_costs == list(np.minimum.accumulate(res.costs)) and prop.scores == res.costs
        hi = 30 if kind == "mppi" else 25
        for c in res.cfgs:
            assert 5 <= c["horizon"] <= hi and type(c["horizon"]) is int
            if kind == "mppi":
                assert 100 <= c["num_path"] <= 1000 and 1e-4 <= c["sigma"] <= 2.0 and 0.1 <= c["lmda"] <= 2.0
            else:
                assert "num_path" not in c
            for key in ("Q", "R", "F"):
                assert np.all(c[key] >= 1e-3 * (1 - 1e-12)) and np.all(c[key] <= 1e4 * (1 + 1e-12))
    (dev, res_d), (host, res_h) = runs["device"], runs["numpy"]
    assert res_d.costs[:16] == res_h.costs[:16]                      # the random batch
    for b, ((case, rd), (case_h, rh)) in enumerate(zip(dev.calls, host.calls)):
        if not (np.array_equal(case["X"], case_h["X"]) and np.array_equal(case["pool"], case_h["pool"])):
            print("batch %d: the histories parted at an earlier near-tie; not compared" % (b + 1))
            break
        name = "e2e_%s_%d" % (kind, b)
        bc.CASES[name] = case
        _, _, _, tol, _ = bc.reference(name)
        bc.check_result(name, rd)
        if rd["chosen"] != rh["chosen"]:
            print("batch %d: two hyperparameter rows within tolerance; picks not compared" % (b + 1))
            break
        same = True
        for step in range(case["q"]):
            if rd["picks"][step] == rh["picks"][step]:
                continue
            need = 2 * tol["ei"] / rd["pick_ei"][step] if rd["pick_ei"][step] > 0 else np.inf
            assert rd["pick_margin"][step] <= need, (b, step, rd["pick_margin"][step], need)
            same = False
            break                                                    # (after a near-tie the sequences may part)
        if not same:
            break
