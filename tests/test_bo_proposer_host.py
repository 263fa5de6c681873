"""The Bayesian-optimisation proposer (autompc_amd/tuning/proposer.py) on the host: the encoder, the rank transform,
``gp_propose_host`` against the long-double yardstick of tests/bo_cases.py on the cases the GPU test runs, the
believer update against a GP refitted from scratch, the tuner's ``proposer`` keyword, and the search itself against
random search on a synthetic closed-loop-like cost."""
import math

import numpy as np
import pytest

import bo_cases as bc
from helpers import make_system


# ---- encoder ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mppi", "ilqr"])
def test_encoder_round_trip(kind):
    from autompc_amd.tuning import random_candidates, random_ilqr_candidates
    from autompc_amd.tuning.proposer import CandidateEncoder
    system = make_system(3, 2)
    enc = CandidateEncoder(system, kind)
    assert enc.d == (4 if kind == "mppi" else 1) + 3 + 2 + 3
    draw = random_candidates if kind == "mppi" else random_ilqr_candidates
    for c in draw(system, 40, seed=3):
        x = enc.encode(c)
        assert x.shape == (enc.d,) and np.all(x >= 0.0) and np.all(x <= 1.0)
        back = enc.decode(x)
        assert set(back) == set(c) and back["horizon"] == c["horizon"] and type(back["horizon"]) is int
        if kind == "mppi":
            assert back["num_path"] == c["num_path"] and type(back["num_path"]) is int
            assert back["sigma"] == pytest.approx(c["sigma"], rel=1e-12, abs=1e-15)
            assert back["lmda"] == pytest.approx(c["lmda"], rel=1e-12)
        for key in ("Q", "R", "F"):
            np.testing.assert_allclose(back[key], c[key], rtol=1e-12)
        np.testing.assert_allclose(enc.encode(back), x, rtol=0, atol=1e-14)
        np.testing.assert_allclose(enc.snap(x)[0], enc.encode(enc.decode(x)), rtol=0, atol=1e-14)


def test_encoder_snaps_integer_axes_and_clips():
    from autompc_amd.tuning.proposer import CandidateEncoder
    system = make_system(2, 1)
    enc = CandidateEncoder(system, "mppi")
    x = np.full(enc.d, 0.5)
    x[0] = (17.4 - 5) / 25          # horizon between grid points
    x[3] = (512.6 - 100) / 900      # num_path between grid points
    c = enc.decode(x)
    assert c["horizon"] == 17 and c["num_path"] == 513
    snapped = enc.encode(c)
    assert snapped[0] == pytest.approx(12 / 25) and snapped[3] == pytest.approx(413 / 900)
    np.testing.assert_allclose(enc.snap(x)[0], snapped, rtol=0, atol=1e-14)
    # out of range: clipped to the range's ends
    lo, hi = enc.decode(np.full(enc.d, -0.3)), enc.decode(np.full(enc.d, 1.7))
    assert lo["horizon"] == 5 and hi["horizon"] == 30 and lo["num_path"] == 100 and hi["num_path"] == 1000
    assert lo["sigma"] == 1e-4 and hi["sigma"] == 2.0 and lo["lmda"] == 0.1 and hi["lmda"] == 2.0
    np.testing.assert_allclose(lo["Q"], 1e-3)
    np.testing.assert_allclose(hi["F"], 1e4)
    wide = dict(horizon=99, sigma=7.0, lmda=0.0, num_path=5, Q=np.full(2, 1e9), R=np.full(1, 1e-9), F=np.ones(2))
    e = enc.encode(wide)
    assert e[0] == 1.0 and e[1] == 1.0 and e[2] == 0.0 and e[3] == 0.0 and e[4] == 1.0 and e[6] == 0.0
    ilqr = CandidateEncoder(system, "ilqr")
    assert ilqr.decode(np.ones(ilqr.d))["horizon"] == 25 and "num_path" not in ilqr.decode(np.ones(ilqr.d))


def test_encoder_model_axis_is_one_hot():
    from autompc_amd.tuning.proposer import CandidateEncoder
    system = make_system(2, 1)
    models = [object(), object(), object()]
    enc = CandidateEncoder(system, "ilqr", models=models)
    assert enc.d == 1 + 5 + 3
    for k in range(3):
        c = dict(horizon=9, Q=np.ones(2), R=np.ones(1), F=np.ones(2), model=models[k], model_index=k)
        x = enc.encode(c)
        assert list(x[-3:]) == [1.0 if i == k else 0.0 for i in range(3)]
        back = enc.decode(x)
        assert back["model"] is models[k] and back["model_index"] == k
    x = np.full(enc.d, 0.5)
    x[-3:] = [0.2, 0.9, 0.4]
    assert enc.decode(x)["model"] is models[1]
    assert list(enc.snap(x)[0][-3:]) == [0.0, 1.0, 0.0]


# ---- rank transform --------------------------------------------------------------------------------------------
def test_rank_transform_by_hand():
    from autompc_amd.tuning.proposer import rank_targets
    # ranks: 3.0 -> 3; the two 1.0 tie at (1 + 2) / 2 = 1.5; inf and nan tie at (4 + 5) / 2 = 4.5
    z = rank_targets([3.0, 1.0, np.inf, 1.0, np.nan])
    q20 = 0.8416212335729143                     # Phi^-1(0.8) = -Phi^-1(0.2)
    np.testing.assert_allclose(z, [0.0, -q20, q20, -q20, q20], rtol=0, atol=1e-15)
    # (rank - 1/2) / n of 1, 2, 3, 4 at n = 4: 1/8, 3/8, 5/8, 7/8
    z = rank_targets([10.0, -1.0, 1e9, 0.5])
    np.testing.assert_allclose(z, [0.3186393639643752, -1.1503493803760079, 1.1503493803760079, -0.3186393639643752],
                               rtol=0, atol=1e-15)
    assert rank_targets([5.0]).tolist() == [0.0]
    assert np.all(rank_targets([np.inf, np.inf, np.inf]) == 0.0)
    for seed in (1, 2):                          # the cases' own transform (plain loops) agrees
        s = np.random.default_rng(seed).integers(0, 6, size=30).astype(float)
        np.testing.assert_allclose(rank_targets(s), bc.rank_transform(s), rtol=0, atol=1e-15)


# ---- the host algorithm against the yardstick ---------------------------------------------------------------------
def _host(name, **kw):
    from autompc_amd.tuning.proposer import gp_propose_host
    c = bc.CASES[name]
    return gp_propose_host(c["X"], c["z"], c["hyper_w"], c["hyper_noise"], c["pool"], c["q"], **kw)


@pytest.mark.parametrize("name", bc.SMALL_CASES + ["mid"])
def test_host_algorithm_against_the_long_double_reference(name):
    bc.check_result(name, _host(name))


def test_host_hyperparameter_table_rules():
    a, b = _host("declined_between"), _host("declined_without")
    assert list(a["status"]) == [0, 1, 0] and np.isneginf(a["lml"][1])
    assert a["chosen"] == (0, 2)[b["chosen"]]
    for key in ("picks", "pick_ei", "pick_margin", "mu", "var"):
        np.testing.assert_array_equal(a[key], b[key])
    np.testing.assert_array_equal(a["lml"][[0, 2]], b["lml"])
    twins = _host("twin_rows")
    assert twins["lml"][0] == twins["lml"][1] > twins["lml"][2] and twins["chosen"] == 0
    none = _host("all_declined")
    assert list(none["status"]) == [1, 1] and none["chosen"] == -1 and np.all(none["picks"] == -1)
    assert np.all(np.isnan(none["mu"])) and np.all(np.isnan(none["pick_ei"]))
    five = _host("m5_q5")
    assert sorted(five["picks"]) == [0, 1, 2, 3, 4]


def test_host_limits():
    from autompc_amd.tuning.proposer import gp_propose_host
    X, z, P = np.zeros((3, 2)), np.zeros(3), np.zeros((4, 2))
    w, s = np.ones((1, 2)), np.full(1, 0.1)
    for args in [(np.zeros((2049, 2)), np.zeros(2049), w, s, P, 1), (np.zeros((3, 65)), z, np.ones((1, 65)), s,
                                                                      np.zeros((4, 65)), 1),
                 (X, z, np.ones((65, 2)), np.full(65, 0.1), P, 1), (X, z, w, s, np.zeros((65537, 2)), 1),
                 (X, z, w, s, np.zeros((300, 2)), 257), (X, z, w, s, P, 5), (X, z, w, s, P, 0)]:
        with pytest.raises(ValueError):
            gp_propose_host(*args)


def test_library_refuses_sizes_over_its_limits_before_it_needs_a_device():
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
    with pytest.raises(ValueError):
        _lib.bo_propose(X, z[:2], w, s, P, 1)


@pytest.mark.parametrize("name", ["n33", "pool_cluster", "dup_x"])
def test_believer_rows_equal_a_refit(name):
    """After t picks sigma^2 (and the mean, which the update leaves alone) is that of a long-double GP refitted from
    scratch on the n + t points, the picks' believed means as their targets.  Tolerance: as the case's, from the
    refit's own float64-vs-long-double difference."""
    case = bc.CASES[name]
    res = _host(name, full=True)
    ld, _, _, tol, _ = bc.reference(name)
    assert res["chosen"] == ld.chosen
    g, q = ld.chosen, case["q"]
    for t in (1, q // 2, q):
        picks = [int(j) for j in res["picks"][:t]]
        refit = {}
        for dtype in (bc.LD, np.float64):
            X = np.concatenate([case["X"], case["pool"][picks]]).astype(dtype)
            P = case["pool"].astype(dtype)
            w, noise = case["hyper_w"][g].astype(dtype), dtype(case["hyper_noise"][g])
            target = np.concatenate([case["z"].astype(dtype), np.asarray(ld.mu, dtype=dtype)[picks]])
            K = bc.kernel(X, X, w, dtype)
            K[np.diag_indices(X.shape[0])] += noise
            L = bc.cholesky(K)
            V = bc.forward(L, bc.kernel(X, P, w, dtype))
            refit[dtype] = (V.T @ bc.forward(L, target), np.maximum(1 - np.sum(V * V, axis=0), dtype(bc.VAR_FLOOR)))
        mu_tol = max(tol["mu"], 100 * float(np.max(np.abs(refit[bc.LD][0] - refit[np.float64][0]))) + bc.FLOOR)
        var_tol = max(tol["var"], 100 * float(np.max(np.abs(refit[bc.LD][1] - refit[np.float64][1]))) + bc.FLOOR)
        err_var = float(np.max(np.abs(res["var_picks"][t - 1].astype(bc.LD) - refit[bc.LD][1])))
        err_mu = float(np.max(np.abs(res["mu"].astype(bc.LD) - refit[bc.LD][0])))
        print("%s t=%d: var err %.2e (tol %.2e)  mean err %.2e (tol %.2e)" % (name, t, err_var, var_tol, err_mu, mu_tol))
        assert err_var <= var_tol and err_mu <= mu_tol


# ---- the tuner -------------------------------------------------------------------------------------------------
class _Bowl:
    """A fake evaluator: a fixed function of the ENCODED candidate -- a weighted quadratic bowl in the exponent (the
    score spans orders of magnitude) with a non-finite slab along the first axis."""

    def __init__(self, encoder):
        self.enc = encoder
        d = encoder.d
        self.centre = np.linspace(0.25, 0.65, d)
        self.weight = np.linspace(2.0, 0.4, d)

    def score(self, c):
        x = self.enc.encode(c)
        if x[0] > 0.8:
            return np.inf
        return float(10 ** (6.0 * np.sum(self.weight * (x - self.centre) ** 2)))

    def evaluate(self, candidates, seed=0, index_offset=0):
        return np.array([self.score(c) for c in candidates])


def _ilqr_bowl(encoder):
    from autompc_amd.tuning import IlqrCandidateEvaluator

    class _Ilqr(IlqrCandidateEvaluator, _Bowl):
        def __init__(self, enc):                  # (no device: only the type matters to the default sampler)
            _Bowl.__init__(self, enc)

        evaluate = _Bowl.evaluate
    return _Ilqr(encoder)


def _same_candidates(a, b):
    assert len(a) == len(b)
    for ca, cb in zip(a, b):
        assert set(ca) == set(cb)
        for k in ca:
            if k == "model":
                assert ca[k] is cb[k]
            else:
                assert np.array_equal(ca[k], cb[k]), k


def test_tuner_without_a_proposer_asks_what_it_asked_before():
    from autompc_amd.tuning import BatchPipelineTuner
    from autompc_amd.tuning.proposer import CandidateEncoder
    system = make_system(3, 2)
    models = [object(), object()]
    for ev, kw in ((_Bowl(CandidateEncoder(system, "mppi")), {}), (_ilqr_bowl(CandidateEncoder(system, "ilqr")), {}),
                   (_Bowl(CandidateEncoder(system, "mppi")), dict(models=models))):
        tuner = BatchPipelineTuner(system, ev, batch_size=8, proposer=None, **kw)
        assert tuner.proposer is None
        _same_candidates(tuner.ask(8, np.random.default_rng(11)), tuner._random_search(8, np.random.default_rng(11)))


def test_tuner_refuses_a_proposer_next_to_what_it_cannot_drive():
    from autompc_amd.tuning import BatchPipelineTuner, GpProposer, LqrCandidateEvaluator
    system = make_system(3, 2)
    prop = GpProposer(system, "mppi", backend="numpy")
    ev = _Bowl(prop.encoder)
    with pytest.raises(ValueError, match="sampler"):
        BatchPipelineTuner(system, ev, proposer=prop, sampler=lambda n, rng: [])
    with pytest.raises(ValueError, match="model_factory"):
        BatchPipelineTuner(system, ev, proposer=prop, model_factory=lambda *a, **k: None, trajs=[None])

    class _Lqr(LqrCandidateEvaluator):
        def __init__(self):
            pass
    with pytest.raises(ValueError, match="LQR"):
        BatchPipelineTuner(system, _Lqr(), proposer=prop)
    with pytest.raises(ValueError):
        GpProposer(system, "mppi", backend="cuda")
    with pytest.raises(ValueError):
        GpProposer(system, "lqr")


def test_tuner_drives_the_proposer_with_surrogate_scores():
    from autompc_amd.tuning import BatchPipelineTuner, GpProposer, PipelineTuneResult
    system = make_system(2, 1)
    models = [object(), object()]
    prop = GpProposer(system, "mppi", models=models, backend="numpy", pool=256)
    ev = _Bowl(prop.encoder)
    tuner = BatchPipelineTuner(system, ev, batch_size=12, models=models, proposer=prop, truedyn_noise="device")
    rng = np.random.default_rng(5)
    paths = []
    for _ in range(3):
        batch = tuner.ask(12, rng)
        paths.append(prop.last["path"])
        tuner.tell(batch, ev.evaluate(batch), truedyn_scores=[-1.0] * 12)      # (never seen by the proposer)
    assert paths == ["random", "gp", "gp"]
    assert prop.last["n"] == 24 and 0 <= prop.last["chosen"] < 24 and np.isfinite(prop.last["lml"])
    assert prop.last["min_margin"] == np.min(prop.last["pick_margin"]) and len(prop.last["picks"]) == 9
    assert len(prop.scores) == 36 and prop.scores == [float(s) for s in tuner.costs]
    res = tuner.result()
    assert isinstance(res, PipelineTuneResult) and len(res.cfgs) == len(res.costs) == len(res.inc_costs) == 36
    assert len(res.truedyn_costs) == 36
    for c in res.cfgs:
        assert 5 <= c["horizon"] <= 30 and 100 <= c["num_path"] <= 1000 and 1e-4 <= c["sigma"] <= 2.0
        assert 0.1 <= c["lmda"] <= 2.0 and c["model"] is models[c["model_index"]]
        for key in ("Q", "R", "F"):
            assert np.all(c[key] >= 1e-3 * (1 - 1e-12)) and np.all(c[key] <= 1e4 * (1 + 1e-12))
    # the same seed proposes the same batches
    prop2 = GpProposer(system, "mppi", models=models, backend="numpy", pool=256)
    tuner2 = BatchPipelineTuner(system, ev, batch_size=12, models=models, proposer=prop2)
    _, res2 = tuner2.run(36, np.random.default_rng(5))
    assert res2.costs == res.costs


def test_history_window_keeps_the_best_and_the_latest():
    from autompc_amd.tuning import GpProposer
    system = make_system(2, 1)
    prop = GpProposer(system, "ilqr", backend="numpy", max_points=8)
    cands = prop._random(20, np.random.default_rng(0))
    scores = [5.0, 1.0, 9.0, 1.0, 7.0, 0.5, 8.0, 6.0, 4.0, 3.0] + [20.0 + i for i in range(10)]
    prop.observe(cands, scores)
    # the four lowest (0.5 at 5; 1.0 at 1 and 3, earlier first; 3.0 at 9) and the latest four of the remainder
    assert prop._fit_set().tolist() == [1, 3, 5, 9, 16, 17, 18, 19]


def test_all_rows_declined_gives_a_random_batch():
    from autompc_amd.tuning import GpProposer
    system = make_system(2, 1)
    d = 1 + 2 + 1 + 2
    prop = GpProposer(system, "ilqr", backend="numpy", pool=64, n_init=4,
                      hypers=(np.full((1, d), 1.0 / (0.4 * math.sqrt(d))), np.zeros(1)))
    rng = np.random.default_rng(2)
    first = prop(4, rng)
    assert prop.last["path"] == "random" and prop.declined_batches == 0
    prop.observe([first[0]] + first, [3.0, 3.0, 1.0, 2.0, 5.0])          # X holds a duplicated point (rows 0 and 1)
    batch = prop(6, rng)
    assert prop.last["path"] == "declined" and prop.declined_batches == 1 and len(batch) == 6
    assert all(5 <= c["horizon"] <= 25 and "num_path" not in c for c in batch)
    # ... and it is the random batch the same generator state gives
    prop2 = GpProposer(system, "ilqr", backend="numpy", pool=64, n_init=4, hypers=(prop.hyper_w, prop.hyper_noise))
    rng2 = np.random.default_rng(2)
    prop2(4, rng2)
    rng2.random((32, d)), rng2.normal(0.0, 0.05, size=(32, d))            # the pool's draws
    _same_candidates(batch, prop2._random(6, rng2))


# ---- the search ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,no,nu,batches,batch,pool", [("ilqr", 2, 2, 4, 32, 2048), ("mppi", 3, 1, 5, 64, 4096)])
def test_search_beats_random_search(kind, no, nu, batches, batch, pool):
    """7-D (iLQR, 2 observations, 2 controls) with 4 batches of 32 and a pool of 2048; 11-D (MPPI, 3 observations, 1
    control) with 5 batches of 64 and a pool of 4096: over ten seeds the proposer's median incumbent is below random
    search's and it wins on at least 7 seeds."""
    from autompc_amd.tuning import BatchPipelineTuner, GpProposer
    from autompc_amd.tuning.proposer import CandidateEncoder
    system = make_system(no, nu)
    enc = CandidateEncoder(system, kind)
    assert enc.d == (7 if kind == "ilqr" else 11)
    ev = _ilqr_bowl(enc) if kind == "ilqr" else _Bowl(enc)
    got, rnd = [], []
    for seed in range(10):
        prop = GpProposer(system, kind, backend="numpy", pool=pool)
        tuner = BatchPipelineTuner(system, ev, batch_size=batch, proposer=prop)
        _, res = tuner.run(batches * batch, np.random.default_rng(seed))
        assert prop.declined_batches == 0 and prop.last["path"] == "gp"
        plain = BatchPipelineTuner(system, ev, batch_size=batch)
        _, base = plain.run(batches * batch, np.random.default_rng(seed))
        got.append(res.inc_costs[-1])
        rnd.append(base.inc_costs[-1])
    wins = sum(g < r for g, r in zip(got, rnd))
    print("%s %d-D: median incumbent proposer %.3f random %.3f, wins %d of 10, worst ratio %.2f"
          % (kind, enc.d, np.median(got), np.median(rnd), wins, max(g / r for g, r in zip(got, rnd))))
    assert np.median(got) < np.median(rnd) and wins >= 7
