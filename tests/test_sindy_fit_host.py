"""sysid.sindy_fit on the host: stlsq_gram_host (the device algorithm in numpy) against the models' own train(), the
grouping of fit_sindy_models, the models that go back to train(), the tie rule, and the evaluator's option.  No GPU.

Bound.  max|d| / max|coef| <= 1e-9 with equal support: about 150 x the largest error measured for the Gram route
against train() (6.4e-12 on the 115-feature continuous case, 4.8e-12 at 253 features), to allow for another BLAS's
summation order.
"""
import numpy as np
import pytest

from autompc_amd import SINDy, SINDyFactory
from autompc_amd.evaluation import HoldoutModelEvaluator
from autompc_amd.sysid import sindy_fit as SF
from autompc_amd.tuning.configs import DictConfiguration
from autompc_amd.sysid.linear_fit import PIVOT_EPS
from sindy_fit_cases import (ALPHAS, BOTH, CONFIGS, EDGE_KEPT, EDGE_SMALL, EDGE_WIDE, EDGES, ELIGIBLE, EXTREMES,
                             FEATURES, LIMITS, LONG, NEIGHBOURS, alpha_of, data, first_features, host_fit, new_model,
                             rel_err, request, same_support, trained)


def test_feature_counts():
    for (name, k), n in FEATURES.items():
        assert len(new_model(name, k).library[0]) == n


@pytest.mark.parametrize("name,k", ELIGIBLE + LONG)
def test_gram_route_matches_train(name, k):
    ref = trained(name, k)
    c, status, pivot, margin, iters = host_fit(name, k)
    err = rel_err(c, ref)
    print("stlsq_gram_host %s %d: %d features, err %.2e, pivot^2 %.2e, margin %.2e, %d solves, %d nonzero"
          % (name, k, ref.shape[1], err, pivot, margin, iters, int((ref != 0).sum())))
    assert status == 0 and margin >= 1e-5
    assert same_support(c, ref) and err <= 1e-9
    if k == 9:
        assert not ref.any() and iters == 1


# every case the GPU tests expect to be fitted (status 0), the caller's-xdot ones last: (data, case, xdot)
STATUS0 = ([c + (False,) for c in EDGE_SMALL + EDGE_WIDE + LIMITS + EDGES + EDGE_KEPT + ALPHAS + EXTREMES[:2]
            + [("small", "7d"), ("small", "dup")] + NEIGHBOURS[0.0] + NEIGHBOURS[1e-9]]
           + [("small", "7d", True), ("small", 7, True), ("wide", "trig1:240c", True)])


def _kept_counts(name, k):
    """Kept-feature counts of the second and later solves of a case: the nonzeros stlsq_gram leaves when max_iter
    ends its loop right after the drop before that solve."""
    (lens, obs, ctrls, designs, configs), kw = request(name, [k])
    G = SF.design_gram(np.asarray(lens), obs, ctrls, designs[0], kw.get("ycont"))
    nf, thr, counts = len(designs[0][0]), float(configs[0][2]), set()
    for j in range(obs.shape[1]):
        natural = SF.stlsq_gram(G, nf, nf + j, thr, alpha_of(k), 20)[4]
        for m in range(1, natural):
            counts.add(int(np.count_nonzero(SF.stlsq_gram(G, nf, nf + j, thr, alpha_of(k), m)[0])))
    return counts


def test_first_features_truncates_the_feature_arrays_only():
    lib = new_model("small", 6).library
    cut = first_features(lib, 20)
    assert [len(a) for a in cut[:4]] == [20] * 4 and all(np.array_equal(a, b[:20]) for a, b in zip(cut[:4], lib))
    assert cut[4] is lib[4] and cut[5] is lib[5] and len(lib[4]) > 0
    for (name, k), n in [(c, int(c[1].split(":")[1].rstrip("c"))) for c in EDGE_SMALL + EDGE_WIDE + LIMITS]:
        assert new_model(name, k).library[0].shape == (n,) and new_model(name, k).coefficients.shape[1] == n
    with pytest.raises(ValueError):
        first_features(lib, len(lib[0]) + 1)


@pytest.mark.parametrize("name,k,xdot", STATUS0)
def test_new_cases_cannot_hide_behind_a_decline(name, k, xdot):
    """What keeps a GPU test from passing by a decline: on the host restatement alone every new case is fitted with
    train()'s support, a smallest squared pivot >= 4 x the pivot line and a smallest margin >= 16 x the tie line."""
    ref = trained(name, k, xdot)
    c, status, pivot, margin, iters = host_fit(name, k, xdot)
    n = ref.shape[1]
    print("stlsq_gram_host %s %s%s: %d features, err %.2e, pivot^2 %.2e (%.1f x the line), margin %.2e, %d solves"
          % (name, k, " xdot" if xdot else "", n, rel_err(c, ref), pivot, pivot / (n * PIVOT_EPS), margin, iters))
    assert status == 0 and same_support(c, ref) and rel_err(c, ref) <= 1e-9
    assert pivot >= 4 * n * PIVOT_EPS and margin >= 16 * SF.TIE_MARGIN
    if (name, k) in ALPHAS:
        assert iters == {0.0: 2, 10.0: 3}[alpha_of(k)] and not np.array_equal(ref, trained(name, k[0]))


def test_later_solves_of_the_new_cases_keep_1_8_and_9_features():
    """The back substitution's degenerate case and both sides of the Cholesky panel width (8) are reached by solves
    on a gathered sub-matrix.  (Counted over the 3 / 1 cases; the union over all new cases only grows.)"""
    counts = set()
    for name, k in EDGE_SMALL + EDGE_KEPT + ALPHAS:
        counts |= _kept_counts(name, k)
    assert {1, 8, 9} <= counts
    assert 1 not in set().union(*(_kept_counts(*c) for c in EDGE_SMALL + ALPHAS))     # why EDGE_KEPT exists


def test_the_cases_that_must_decline_do_so_on_the_host():
    """Library D (a feature twice) is singular without the ridge: status 1 by a failed pivot at alpha 0 and by the
    pivot line at alpha 1e-9, and a fit at 0.05; an all-zero control column at alpha 0 is a zero diagonal entry."""
    for a in (0.0, 1e-9):
        ks = [NEIGHBOURS[a][0][1], ("dup", a), NEIGHBOURS[a][1][1]]
        args, kw = request("small", ks)
        c, status, pivot, margin, iters = SF.stlsq_gram_host(*args, **kw)
        assert list(status) == [1 if k[0] == "dup" else 0 for k in ks] and np.all(np.isnan(c[1]))
        assert np.array_equal(c[0], host_fit("small", ks[0])[0]) and np.array_equal(c[2], host_fit("small", ks[2])[0])
    assert iters[1] == 1 and 0 < pivot[1] < 13 * PIVOT_EPS                        # (the 1e-9 call)
    args, kw = request("small", [("states", 0.0), (1, 0.0), ("states_c", 0.0)])
    args = args[:2] + (np.zeros_like(args[2]),) + args[3:]
    c, status, pivot, margin, iters = SF.stlsq_gram_host(*args, **kw)
    assert list(status) == [0, 1, 0] and pivot[1] == 0.0 and iters[1] == 0 and np.all(np.isnan(c[1]))
    assert pivot[0] >= 4 * 3 * PIVOT_EPS and min(margin[0], margin[2]) >= 16 * SF.TIE_MARGIN
    m = new_model("small", ("dup", 1e-9))
    rep = SF.fit_sindy_models([m], data("small")[1], alpha=1e-9, backend="numpy")
    assert rep[0]["where"] == "host" and rep[0]["reason"] == "status 1" and rep[0]["iters"] == 1
    assert np.array_equal(m.coefficients, trained("small", ("dup", 1e-9)))


def test_both_target_sets_share_one_design():
    for name, kd, kc in BOTH:
        assert len(request(name, [kd, kc])[0][3]) == 1 and request(name, [kd, kc])[1]["ycont"] is not None


def test_models_of_two_libraries_share_two_designs():
    s, trajs = data("small")
    kws = [dict(CONFIGS[3]), dict(CONFIGS[3], threshold=0.05), dict(CONFIGS[3], time_mode="continuous"),
           dict(CONFIGS[5]), dict(CONFIGS[5], threshold=0.03), dict(CONFIGS[5], time_mode="continuous", threshold=0.1)]
    models = [SINDy(s, **kw) for kw in kws]
    rep = SF.fit_sindy_models(models, trajs, backend="numpy")
    assert rep.designs == 2 and rep.device_fits == 6 and rep.host_fits == 0
    for m, kw, r in zip(models, kws, rep):
        ref = SINDy(s, **kw)
        ref.train(trajs)
        assert r["where"] == "device" and r["reason"] is None and r["iters"] >= 1 and r["margin"] >= 1e-5
        assert same_support(m.coefficients, ref.coefficients) and rel_err(m.coefficients, ref.coefficients) <= 1e-9


def test_equal_configurations_are_fitted_once(monkeypatch):
    s, trajs = data("small")
    # method / lasso_alpha do not enter: train() ignores them
    models = [new_model("small", 3), new_model("small", 3, method="lasso", lasso_alpha=0.5), new_model("small", 2)]
    seen = []
    real = SF.stlsq_gram_host
    monkeypatch.setattr(SF, "stlsq_gram_host", lambda *a, **kw: seen.append(a[4]) or real(*a, **kw))
    rep = SF.fit_sindy_models(models, trajs, backend="numpy")
    assert len(seen) == 1 and len(seen[0]) == 2 and rep.device_fits == 2 and rep.designs == 2
    assert np.array_equal(models[0].coefficients, models[1].coefficients)
    assert same_support(models[2].coefficients, trained("small", 2))


class _Half(SINDy):
    def train(self, trajs, **kw):
        super().train(trajs, **kw)
        self.set_coefficients(0.5 * self.coefficients)


BIG = dict(poly_basis=True, poly_degree=8, trig_basis=True, trig_freq=3, threshold=0.03)     # 322 features on 17 / 6


def test_size_and_subclass_go_to_train():
    s, trajs = data("hc")
    kws = [BIG, CONFIGS[2], CONFIGS[2], CONFIGS[2]]
    models = [SINDy(s, **BIG), _Half(s, **CONFIGS[2]), new_model("hc", 2), _Half(s, **CONFIGS[2])]
    assert len(models[0].library[0]) == 322 > SF.MAX_FEATURES
    rep = SF.fit_sindy_models(models, trajs, max_iter=3, backend="numpy")
    assert [r["where"] for r in rep] == ["host", "host", "device", "host"]
    assert [r["reason"] for r in rep] == ["size", "subclass", None, "subclass"]
    assert rep.host_fits == 2 and rep.device_fits == 1 and rep.designs == 1
    for m, kw in zip(models, kws):
        ref = type(m)(s, **kw)
        ref.train(trajs, max_iter=3)
        if m is models[2]:
            assert same_support(m.coefficients, ref.coefficients) and rel_err(m.coefficients, ref.coefficients) <= 1e-9
        else:
            assert np.array_equal(m.coefficients, ref.coefficients) and ref.coefficients.any()


def test_configurations_4_and_6_are_size_host_fits_on_17_6(monkeypatch):
    """Their own train() is what fits them (2139 / 2599 features: one train() is 17 x up to 20 dense solves of that
    order, half a minute on the host, so the call is recorded here and not run; the size route with the real train()
    is test_size_and_subclass_go_to_train's 322-feature model)."""
    s, trajs = data("hc")
    calls = []

    def spy(self, trajs_, xdot=None, silent=False, alpha=0.05, max_iter=20):
        calls.append((self, trajs_, xdot, alpha, max_iter))
        self.set_coefficients(np.full(self.coefficients.shape, float(len(calls))))
    monkeypatch.setattr(SINDy, "train", spy)
    models = [new_model("hc", 4), new_model("hc", 6), new_model("hc", 4)]
    rep = SF.fit_sindy_models(models, trajs, alpha=0.1, max_iter=7, backend="numpy")
    assert [(r["where"], r["reason"], r["pivot"]) for r in rep] == [("host", "size", None)] * 3
    assert rep.host_fits == 2 and rep.device_fits == 0 and rep.designs == 0
    assert [c[0] for c in calls] == models[:2] and all(c[1:] == (trajs, None, 0.1, 7) for c in calls)
    assert np.array_equal(models[2].coefficients, models[0].coefficients) and models[1].coefficients[0, 0] == 2.0


def test_max_iter_ends_the_loop_right_after_a_drop():
    s, trajs = data("hc")
    assert host_fit("hc", 3)[4] == 7                       # the natural count
    m, ref = new_model("hc", 3), new_model("hc", 3)
    rep = SF.fit_sindy_models([m], trajs, max_iter=2, backend="numpy")
    ref.train(trajs, max_iter=2)
    assert rep[0]["where"] == "device" and rep[0]["iters"] == 2
    assert same_support(m.coefficients, ref.coefficients) and rel_err(m.coefficients, ref.coefficients) <= 1e-9
    assert not same_support(ref.coefficients, trained("hc", 3))
    with pytest.raises(ValueError):
        SF.stlsq_gram_host(*request("hc", [3])[0], max_iter=0)


def test_alpha_and_xdot_are_passed_through():
    s, trajs = data("small")
    rng = np.random.default_rng(1)
    xdot = [rng.normal(size=t.obs.shape) for t in trajs]
    m, ref = new_model("small", 7), new_model("small", 7)
    rep = SF.fit_sindy_models([m], trajs, xdot=xdot, alpha=0.5, backend="numpy")
    ref.train(trajs, xdot=xdot, alpha=0.5)
    assert rep[0]["where"] == "device"
    assert same_support(m.coefficients, ref.coefficients) and rel_err(m.coefficients, ref.coefficients) <= 1e-9
    assert not same_support(ref.coefficients, trained("small", 7))
    # continuous mode, a one-row trajectory and no xdot: np.gradient raises in train(), and here
    with pytest.raises(ValueError):
        SF.fit_sindy_models([new_model("long", 7)], data("long")[1], backend="numpy")


def test_a_near_tie_is_status_2_and_a_host_fit():
    s, trajs = data("small")
    (lens, obs, ctrls, designs, configs), kw = request("small", [3])
    # the first, all-features solve of target 0: threshold 0 drops nothing
    first = SF.stlsq_gram_host(lens, obs, ctrls, designs, [(0, False, 0.0)], max_iter=1)[0][0]
    w = np.sort(np.abs(first[0]))[len(first[0]) // 2]
    thr = float(w * (1.0 + 2.0 ** -24))
    _, status, _, margin, _ = SF.stlsq_gram_host(lens, obs, ctrls, designs, [(0, False, thr)])
    assert status[0] == 2 and margin[0] < SF.TIE_MARGIN
    m, ref = new_model("small", 3, threshold=thr), new_model("small", 3, threshold=thr)
    rep = SF.fit_sindy_models([m], trajs, backend="numpy")
    ref.train(trajs)
    assert rep[0]["where"] == "host" and rep[0]["reason"] == "status 2" and rep[0]["margin"] < SF.TIE_MARGIN
    assert rep.host_fits == 1 and rep.device_fits == 0
    assert np.array_equal(m.coefficients, ref.coefficients)


def test_wrong_arguments():
    s, trajs = data("small")
    with pytest.raises(ValueError, match="backend"):
        SF.fit_sindy_models([new_model("small", 1)], trajs, backend="cpu")
    with pytest.raises(TypeError):
        SF.fit_sindy_models([object()], trajs, backend="numpy")
    with pytest.raises(ValueError, match="share one system"):
        SF.fit_sindy_models([new_model("small", 1), new_model("hc", 1)], trajs, backend="numpy")


def test_sindy_fit_option_is_checked_and_the_default_never_calls_the_batched_fit(monkeypatch):
    from autompc_amd.tuning import BatchPipelineTuner
    s, trajs = data("small")
    with pytest.raises(ValueError, match="sindy_fit"):
        HoldoutModelEvaluator(s, trajs, "rmse", np.random.default_rng(0), sindy_fit="gpu")
    with pytest.raises(ValueError, match="sindy_fit"):
        BatchPipelineTuner(s, None, sindy_fit="gpu")
    assert BatchPipelineTuner(s, None).sindy_fit == "host" and BatchPipelineTuner(s, None).sindy_host_fits == 0
    assert HoldoutModelEvaluator(s, trajs, "rmse", np.random.default_rng(0), sindy_fit="device").sindy_fit == "device"

    def boom(*a, **kw):
        raise AssertionError("the default path must not call fit_sindy_models")
    monkeypatch.setattr(SF, "fit_sindy_models", boom)
    size = lambda model, test_trajs: float(np.abs(model.coefficients).sum())       # a metric that needs no device
    ev = HoldoutModelEvaluator(s, trajs, size, np.random.default_rng(0), holdout_prop=0.25)
    assert ev.sindy_fit == "host" and ev.last_sindy_fit is None
    cfgs = [DictConfiguration(trig_basis="true", trig_freq=1, threshold=0.02, time_mode="discrete"),
            DictConfiguration(threshold=0.05, time_mode="discrete")]
    scores = ev.evaluate_batch(SINDyFactory(s), cfgs)
    for sc, cfg in zip(scores, cfgs):
        ref = SINDyFactory(s)(cfg, ev.training_set)
        assert sc == float(np.abs(ref.coefficients).sum()) and sc > 0
    assert ev.last_sindy_fit is None
