"""sysid.lasso_fit on the host: lasso_fit_host (the device algorithm in numpy) against sklearn's Lasso and the
reference's goldens, the models fit_linear_models sends there and the ones it hands back to train(), and the option
that switches the route on.

Tolerances.  Coefficients: max|dcoef| / max|coef| <= 10 x the error recorded for the case when the goldens were made
(lassofit_cases.HOST_ERR; all below 1e-9: the same sklearn, another BLAS summation order at most).  Sweep counts and
bitwise claims are exact."""
import functools
import warnings

import numpy as np
import pytest

from autompc_amd import ARX, Koopman
from autompc_amd.evaluation import HoldoutModelEvaluator
from autompc_amd.sysid import lasso_fit as LS
from autompc_amd.sysid import linear_fit as LF
from autompc_amd.tuning import BatchPipelineTuner
from lassofit_cases import CASES, FITTED, HOST_ERR, basis, data, new_model, reference, rel_err, trajs
from linfit_cases import model_params


@functools.lru_cache(maxsize=None)
def host(name):
    lens, obs, ctrls = data(name)
    return LS.lasso_fit_host(lens, obs, ctrls, [basis(name)], [(0, a) for a in CASES[name]["alphas"]],
                             per_target=True)


def _train(m, tr):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                       # sklearn's ConvergenceWarning at the sweep cap
        m.train(tr, silent=True)
    return m


@pytest.mark.parametrize("name", FITTED)
def test_restatement_takes_sklearns_sweeps_and_reaches_its_coefficients(name):
    from sklearn.linear_model import Lasso
    lens, obs, ctrls = data(name)
    F, Y = LF.koopman_design(lens, obs, ctrls, basis(name))
    coeffs, status, margin, sweeps, per = host(name)
    for k, alpha in enumerate(CASES[name]["alphas"]):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            clf = Lasso(alpha=alpha).fit(F, Y)
        ref, n_iter = reference(name, k)
        err, gerr = rel_err(coeffs[k], clf.coef_), rel_err(coeffs[k], ref)
        print("%s alpha %g: sweeps %d..%d, error against sklearn %.1e, against the golden %.1e, margins %s"
              % (name, alpha, per[k].min(), per[k].max(), err, gerr, margin[k]))
        assert status[k] == 0
        assert np.array_equal(per[k], np.atleast_1d(clf.n_iter_)) and np.array_equal(per[k], n_iter)
        assert sweeps[k] == n_iter.max()
        assert err <= 10 * HOST_ERR[name] and gerr <= 10 * HOST_ERR[name] < 1e-9


def test_recorded_errors_are_the_goldens_and_the_named_sweep_counts_hold():
    from lassofit_cases import gold
    for name in FITTED:
        assert float(gold(name)["host_err"]) <= HOST_ERR[name] <= 1.2 * float(gold(name)["host_err"])
    coeffs, _, _, sweeps, per = host("n13")
    assert sweeps[0] == 1 and not np.any(coeffs[0])           # alpha 1e2: every coefficient 0 after one sweep
    assert np.all(per[3] == 1000)                             # alpha 1e-6: every target runs the cap


def test_untouched_column_keeps_coefficient_zero_and_constant_column_is_status_1():
    coeffs, status, _, _, _ = host("zero")
    assert status[0] == 0 and not np.any(coeffs[0][:, -1]) and np.any(coeffs[0][:, :-1])
    coeffs, status, margin, sweeps, _ = host("const")
    assert status[0] == 1 and sweeps[0] == 0 and np.all(np.isnan(coeffs[0]))


def test_no_case_is_a_tie_and_a_constructed_tie_is_status_2():
    for name in FITTED:
        _, status, margin, _, _ = host(name)
        assert np.all(status == 0)
        assert np.all(margin[:, 0] > LS.TIE) and np.all(margin[:, 1] > LS.RATIO_TIE)
    lens, obs, ctrls = data("n13")
    margin = host("n13")[2][2]                                # alpha 1e-2
    for kw in (dict(tie=1.01 * margin[0]), dict(ratio_tie=1.01 * margin[1])):
        _, status, m2, _ = LS.lasso_fit_host(lens, obs, ctrls, [basis("n13")], [(0, 1e-2)], **kw)
        assert status[0] == 2 and np.array_equal(m2[0], margin)
    assert LS.TIE == 100 * LS.GAP_FORM_ERROR and LS.RATIO_TIE == 100 * LS.RATIO_FORM_ERROR


def _mixed(s):
    dup = dict(poly_basis=True, poly_degree=3, trig_basis=True)
    return [ARX(s, history=2), Koopman(s), new_model(s, "n13", 1e-2), Koopman(s, method="lasso", lasso_alpha=1e-1, **dup),
            new_model(s, "n13", 1e-2), new_model(s, "n13", 1.0),
            Koopman(s, method="lasso", lasso_alpha=1e-2, product_terms=True)]


def test_fit_linear_models_sends_lasso_models_to_the_gram_route_only_when_asked(monkeypatch):
    s, tr = trajs("n13")
    models = _mixed(s)
    calls = []
    real = LS.lasso_fit_host
    monkeypatch.setattr(LS, "lasso_fit_host", lambda *a, **k: calls.append((len(a[3]), len(a[4]))) or real(*a, **k))
    rep = LF.fit_linear_models(models, tr, backend="numpy", lasso="device")
    assert calls == [(2, 3)]                                  # two bases, three distinct (basis, alpha)
    assert [(r["where"], r["reason"]) for r in rep] == [("device", None)] * 6 + [("host", "product_terms")]
    assert rep.device_fits == 5 and rep.host_fits == 1
    for i in (2, 3, 4, 5):
        assert set(rep[i]) == {"where", "reason", "pivot", "sweeps", "margin"}
        assert rep[i]["sweeps"] >= 1 and rep[i]["margin"] > 0 and rep[i]["pivot"] is None
    assert set(rep[0]) == set(rep[1]) == set(rep[6]) == {"where", "reason", "pivot"}
    assert rep[2] == rep[4] and np.array_equal(model_params(models[2]), model_params(models[4]))
    for m, fresh in zip(models, _mixed(s)):
        ref = _train(fresh, tr)
        # the lasso models: the recorded restatement error of this data set's case; the basis with duplicates is
        # not a recorded case: the 1e-9 every measured case stays under
        dup = isinstance(m, Koopman) and len(set(m.basis)) != len(m.basis)
        tol = 1e-9 if dup else max(10 * HOST_ERR["n13"], 1e-12)
        assert rel_err(model_params(m), model_params(ref)) <= tol
    assert np.array_equal(model_params(models[6]), model_params(_train(_mixed(s)[6], tr)))
    # the default: today's report, lasso models to train()
    models = _mixed(s)
    rep = LF.fit_linear_models(models, tr, backend="numpy")
    assert calls == [(2, 3)]
    assert [(r["where"], r["reason"]) for r in rep] == ([("device", None)] * 2 + [("host", "method")] * 5)
    assert all(set(r) == {"where", "reason", "pivot"} for r in rep)
    assert np.array_equal(model_params(models[2]), model_params(_train(_mixed(s)[2], tr)))


def test_status_1_and_status_2_models_are_fitted_by_train_bit_for_bit(monkeypatch):
    s, tr = trajs("const")
    m = new_model(s, "const", 1e-3)
    rep = LF.fit_linear_models([m], tr, backend="numpy", lasso="device")
    assert (rep[0]["where"], rep[0]["reason"]) == ("host", "status 1") and rep.host_fits == 1
    assert np.array_equal(model_params(m), model_params(_train(new_model(s, "const", 1e-3), tr)))
    s, tr = trajs("n13")
    monkeypatch.setattr(LS, "lasso_fit_host", functools.partial(LS.lasso_fit_host, ratio_tie=1.0))
    m = new_model(s, "n13", 1e-2)
    rep = LF.fit_linear_models([m], tr, backend="numpy", lasso="device")
    assert (rep[0]["where"], rep[0]["reason"]) == ("host", "status 2") and rep[0]["sweeps"] == 1000
    assert np.array_equal(model_params(m), model_params(_train(new_model(s, "n13", 1e-2), tr)))


def test_lasso_options_are_checked_and_default_to_host():
    s, tr = trajs("n13")
    with pytest.raises(ValueError, match="lasso"):
        LF.fit_linear_models([new_model(s, "n13", 1.0)], tr, backend="numpy", lasso="gpu")
    with pytest.raises(ValueError, match="lasso_fit"):
        HoldoutModelEvaluator(s, tr, "rmse", np.random.default_rng(0), lasso_fit="gpu")
    with pytest.raises(ValueError, match="lasso_fit"):
        BatchPipelineTuner(s, None, lasso_fit="gpu")
    assert BatchPipelineTuner(s, None).lasso_fit == "host"
    assert HoldoutModelEvaluator(s, tr, "rmse", np.random.default_rng(0)).lasso_fit == "host"
    assert HoldoutModelEvaluator(s, tr, "rmse", np.random.default_rng(0), linear_fit="device",
                                 lasso_fit="device").lasso_fit == "device"
