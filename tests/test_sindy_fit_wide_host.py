"""The wide SINDy fit's cases on the host: every case tests/test_gpu_sindy_fit_wide.py holds to the rule is fitted by
the numpy restatement alone with reserve, the blocked factorisation the large cases use agrees with the plain one, and
fit_sindy_models' routing of libraries over 272 features (backend="numpy") and the evaluators' / tuners' keyword.  No
GPU."""
import numpy as np
import pytest

from autompc_amd import SINDyFactory
from autompc_amd import _lib
from autompc_amd.evaluation import HoldoutModelEvaluator
from autompc_amd.sysid import sindy_fit as SF
from autompc_amd.sysid.linear_fit import PIVOT_EPS
from autompc_amd.tuning import BatchModelTuner, BatchPipelineTuner
from autompc_amd.tuning.configs import DictConfiguration
from sindy_fit_wide_cases import (EDGE_ROWS, MIXED, SHRINK, SIZES, data, full_library, host_fit, library, new_model,
                                  rel_err, request, same_support, scaled_cholesky_blocked, support_of, trained, xdot)

CASES = [(name, n, None) for name, n in SIZES + MIXED + EDGE_ROWS] + SHRINK


def test_constants_and_entry():
    assert SF.MAX_FEATURES == 272 and SF.MAX_FEATURES_WIDE == 2048
    assert callable(_lib.sindy_fit_wide)
    assert _lib.SIGNATURES["ampc_sindy_fit_wide"] == _lib.SIGNATURES["ampc_sindy_fit"]
    assert hasattr(_lib.load(), "ampc_sindy_fit_wide") and _lib.load().ampc_version() == 114
    assert len(full_library("s")[0]) == 525 and len(full_library("big")[0]) == 2050


def test_blocked_factorisation_is_the_plain_one():
    (lens, obs, ctrls, designs, _), kw = request("s", 400)
    G = SF.design_gram(np.asarray(lens), obs, ctrls, designs[0], kw["ycont"])
    S, b = G[:400, :400] + 0.05 * np.eye(400), G[:400, 400 + 2]
    w0, p0 = SF._scaled_cholesky_1(S, b)
    for nb in (32, 64, 400):
        w1, p1 = scaled_cholesky_blocked(S, b, nb)
        assert np.max(np.abs(w1 - w0)) <= 1e-12 * np.max(np.abs(w0)) and abs(p1 - p0) <= 1e-12 * p0
    bad = S.copy()
    bad[7, 7] = 0.0
    assert scaled_cholesky_blocked(bad, b)[0] is None and scaled_cholesky_blocked(bad, b)[1] == 0.0


@pytest.mark.parametrize("name,n,kept", CASES)
def test_host_restatement_fits_every_case_with_reserve(name, n, kept):
    """4 x over the pivot line, 16 x over the tie line, the planned number of solves and train()'s support."""
    coef, status, pivot, margin, iters = host_fit(name, n, kept)
    ref = trained(name, n, kept)
    idx = support_of(n, kept)
    print("wide host %s %d kept %s: pivot^2 %.3e (line %.3e), margin %.3e, %d solves, vs train() %.2e"
          % (name, n, kept, pivot, n * PIVOT_EPS, margin, iters, rel_err(coef, ref)))
    assert status == 0 and pivot >= 4 * n * PIVOT_EPS and margin >= 16 * SF.TIE_MARGIN
    assert iters == (1 if len(idx) == n else 2)
    assert same_support(coef, ref) and np.array_equal(np.nonzero(coef[0])[0], idx)
    assert rel_err(coef, ref) <= 1e-9


def _models(name, ns):
    return [new_model(name, library(name, n)) for n in ns]


def test_default_sends_273_features_to_train_and_wide_takes_the_gram_route(monkeypatch):
    trajs, xd = data("s")[1], xdot("s", 273)
    m, = _models("s", [273])
    rep = SF.fit_sindy_models([m], trajs, xdot=xd, backend="numpy")
    assert rep[0]["where"] == "host" and rep[0]["reason"] == "size" and rep[0]["route"] is None
    assert rep.host_fits == 1 and rep.device_fits == 0 and rep.designs == 0
    assert np.array_equal(m.coefficients, trained("s", 273))
    m, = _models("s", [273])
    monkeypatch.setattr(SF.SINDy, "train", lambda *a, **k: pytest.fail("train() called"))
    rep = SF.fit_sindy_models([m], trajs, xdot=xd, backend="numpy", wide="device")
    assert rep[0]["where"] == "device" and rep[0]["route"] == "wide" and rep[0]["iters"] == 2
    assert rep.host_fits == 0 and rep.device_fits == 1 and rep.designs == 1
    ref = trained("s", 273)
    assert same_support(m.coefficients, ref) and rel_err(m.coefficients, ref) <= 1e-9
    with pytest.raises(ValueError, match="wide must be"):
        SF.fit_sindy_models([m], trajs, xdot=xd, backend="numpy", wide="gpu")


def test_2049_features_still_go_to_train():
    s, trajs = data("big")
    m = new_model("big", library("big", 2049))
    assert SF._host_reason(m, SF.MAX_FEATURES_WIDE) == "size" and SF._host_reason(m) == "size"
    assert SF._host_reason(new_model("big", library("big", 2048)), SF.MAX_FEATURES_WIDE) is None
    calls = []
    m.train = lambda *a, **k: calls.append(k)            # (the fit itself is train()'s: not repeated here)
    rep = SF.fit_sindy_models([m], trajs, xdot=xdot("big", 2048), backend="numpy", wide="device")
    assert len(calls) == 1 and rep[0]["where"] == "host" and rep[0]["reason"] == "size" and rep[0]["route"] is None


def test_a_mixed_batch_makes_the_two_groups(monkeypatch):
    trajs, xd = data("s")[1], xdot("s", 273)
    models = _models("s", [17, 273, 272, 400, 273])
    calls = []
    real = SF.stlsq_gram_host
    monkeypatch.setattr(SF, "stlsq_gram_host",
                        lambda *a, **k: calls.append([len(d[0]) for d in a[3]]) or real(*a, **k))
    rep = SF.fit_sindy_models(models, trajs, xdot=xd, backend="numpy", wide="device")
    assert calls == [[17, 272], [273, 400]]
    assert [r["route"] for r in rep] == ["narrow", "wide", "narrow", "wide", "wide"]
    assert all(r["where"] == "device" for r in rep)
    assert rep.designs == 4 and rep.device_fits == 4 and rep.host_fits == 0
    assert np.array_equal(models[1].coefficients, models[4].coefficients)
    for m, n in zip(models, [17, 273, 272, 400, 273]):
        ref = new_model("s", library("s", n))
        ref.train(trajs, xdot=xd)
        assert same_support(m.coefficients, ref.coefficients) and rel_err(m.coefficients, ref.coefficients) <= 1e-9


def test_the_keyword_is_validated_and_passed_through(monkeypatch):
    s, trajs = data("s")
    rng = np.random.default_rng(0)
    with pytest.raises(ValueError, match="sindy_wide_fit must be 'host' or 'device'"):
        HoldoutModelEvaluator(s, trajs, "rmse", rng, sindy_wide_fit="gpu")
    with pytest.raises(ValueError, match="sindy_wide_fit must be 'host' or 'device'"):
        BatchPipelineTuner(s, None, sindy_wide_fit="gpu")
    ev = HoldoutModelEvaluator(s, trajs, "rmse", rng)
    with pytest.raises(ValueError, match="sindy_wide_fit must be 'host' or 'device'"):
        BatchModelTuner(s, ev, sindy_wide_fit="gpu")
    assert ev.sindy_wide_fit == "host" and BatchPipelineTuner(s, None).sindy_wide_fit == "host"
    assert BatchModelTuner(s, ev).evaluator.sindy_wide_fit == "host"
    assert BatchModelTuner(s, ev, sindy_wide_fit="device").evaluator.sindy_wide_fit == "device"
    seen = []

    def fake(models, trajs_, **kw):
        seen.append(kw)
        for m in models:
            m.train(trajs_, silent=True)
        return SF.SindyFitReport()
    monkeypatch.setattr(SF, "fit_sindy_models", fake)
    size = lambda model, test_trajs: float(np.abs(model.coefficients).sum())       # a metric that needs no device
    cfgs = [DictConfiguration(threshold=0.05, time_mode="discrete")]
    for wide in ("host", "device"):
        ev = HoldoutModelEvaluator(s, trajs, size, np.random.default_rng(0), holdout_prop=0.25, sindy_fit="device",
                                   sindy_wide_fit=wide)
        ev.evaluate_batch(SINDyFactory(s), cfgs)
        tuner = BatchPipelineTuner(s, None, model_factory=SINDyFactory(s), trajs=trajs, sindy_fit="device",
                                   sindy_wide_fit=wide)
        tuner.fit_models([{"model": None, "model_cfg": dict(threshold=0.05, time_mode="discrete")}])
    assert seen == [{"wide": "host"}] * 2 + [{"wide": "device"}] * 2
