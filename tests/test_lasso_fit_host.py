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
from lassofit_cases import (CASES, FITTED, HOST_ERR, NO_GOLDEN, TIES, basis, data, host, new_model, reference,
                            rel_err, trajs, zero_columns)
from linfit_cases import model_params


@functools.lru_cache(maxsize=None)
def sklearn_fit(name, k):
    """(coef_, n_iter_ per target) of sklearn's Lasso on the case's design at its k-th alpha, computed once."""
    from sklearn.linear_model import Lasso
    F, Y = LF.koopman_design(*data(name), basis(name))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        clf = Lasso(alpha=CASES[name]["alphas"][k]).fit(F, Y)
    return clf.coef_, np.atleast_1d(clf.n_iter_)


def _train(m, tr):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                       # sklearn's ConvergenceWarning at the sweep cap
        m.train(tr, silent=True)
    return m


@pytest.mark.parametrize("name", FITTED)
def test_restatement_takes_sklearns_sweeps_and_reaches_its_coefficients(name):
    coeffs, status, margin, sweeps, per = host(name)
    for k, alpha in enumerate(CASES[name]["alphas"]):
        coef, sk_iter = sklearn_fit(name, k)
        ref, n_iter = reference(name, k)                      # no golden: lasso_fit_host's own, the sklearn side decides
        err, gerr = rel_err(coeffs[k], coef), rel_err(coeffs[k], ref)
        print("%s alpha %g: sweeps %d..%d, error against sklearn %.1e, against the golden %.1e, margins %s"
              % (name, alpha, per[k].min(), per[k].max(), err, gerr, margin[k]))
        assert status[k] == (2 if (name, k) in TIES else 0)
        assert np.array_equal(per[k], sk_iter) and np.array_equal(per[k], n_iter)
        assert sweeps[k] == n_iter.max()
        assert err <= 10 * HOST_ERR[name] and gerr <= 10 * HOST_ERR[name]
        # near: the centring leaves 4.1e-8 of its jittered control's sum of squares (2.7 x 2^-26), so 8 of the 16
        # digits of that column's coefficient are gone in any Gram form; every other case stays below 1e-9
        assert name == "near" or 10 * HOST_ERR[name] < 1e-9


def test_recorded_errors_are_the_goldens_and_the_named_sweep_counts_hold():
    from lassofit_cases import gold
    for name in FITTED:
        if name in NO_GOLDEN:                                 # the figure the parametrised test prints
            x = rel_err(host(name)[0][0], sklearn_fit(name, 0)[0])
        else:
            x = float(gold(name)["host_err"])
        assert x <= HOST_ERR[name] <= 1.2 * x, (name, x)
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
        ties = np.array([(name, k) in TIES for k in range(len(status))])
        assert np.array_equal(status, np.where(ties, 2, 0))
        # the named ones are ties by their gap margin alone
        assert np.array_equal(margin[:, 0] <= LS.TIE, ties) and np.all(margin[:, 1] > LS.RATIO_TIE)
    lens, obs, ctrls = data("n13")
    margin = host("n13")[2][2]                                # alpha 1e-2
    for kw in (dict(tie=1.01 * margin[0]), dict(ratio_tie=1.01 * margin[1])):
        _, status, m2, _ = LS.lasso_fit_host(lens, obs, ctrls, [basis("n13")], [(0, 1e-2)], **kw)
        assert status[0] == 2 and np.array_equal(m2[0], margin)
    assert LS.TIE == 100 * LS.GAP_FORM_ERROR and LS.RATIO_TIE == 100 * LS.RATIO_FORM_ERROR


@pytest.mark.parametrize("name", ["s15", "s63", "s65", "zeroobs", "zeroedge", "near"])
def test_centred_gram_is_the_extended_precision_gram_within_its_rounding_bound(name):
    """centred_gram (what every device comparison rests on) against the same sums and centring in long double.
    The bound is derived: an ordered sum of design_rows products grows by at most design_rows eps of its size, the
    centring adds three roundings (the mean's division, the product, the subtraction), so per entry
    |d| <= 4 design_rows 2^-53 (|raw| + m |mu_a mu_b|).  Long double must carry more than 53 bits for this."""
    LD = np.longdouble
    assert np.finfo(LD).eps <= 2.0 ** -63
    lens, obs, ctrls = data(name)
    G, Q, yy, fraw, yraw, m = LS.centred_gram(lens, obs, ctrls, tuple(tuple(x) for x in basis(name)))
    F, Y = LF.koopman_design(lens, obs, ctrls, basis(name))
    nf = F.shape[1]
    assert m == len(F) == 597
    D = np.concatenate([np.ones((m, 1)), F, Y], axis=1).astype(LD)
    raw = D[:, :1 + nf].T @ D
    yraw_x = np.sum(D[:, 1 + nf:] * D[:, 1 + nf:], axis=0)
    mu = raw[0, 1:] / LD(m)
    centre = LD(m) * np.multiply.outer(mu[:nf], mu)
    exact = raw[1:, 1:] - centre
    c = 4 * m * 2.0 ** -53
    worst = 0.0
    for label, got, ex, size in (("G", G, exact[:, :nf], np.abs(raw[1:, 1:1 + nf]) + np.abs(centre[:, :nf])),
                                 ("Q", Q, exact[:, nf:], np.abs(raw[1:, 1 + nf:]) + np.abs(centre[:, nf:])),
                                 ("yy", yy, yraw_x - LD(m) * mu[nf:] ** 2, yraw_x + LD(m) * mu[nf:] ** 2)):
        d, bound = np.abs(got - ex), c * size
        assert np.all(d[bound == 0] == 0)
        ratio = float(np.max(d[bound > 0] / bound[bound > 0]))
        print("%s %s: largest |d| / bound %.2e" % (name, label, ratio))
        worst = max(worst, ratio)
    assert worst <= 1.0
    zf, zt = zero_columns(name)
    for i in zf:
        assert not np.any(G[i]) and not np.any(G[:, i]) and not np.any(Q[i]) and fraw[i] == 0
    for t in zt:
        assert not np.any(Q[:, t]) and yy[t] == 0 and yraw[t] == 0
    assert np.array_equal(np.nonzero(np.diagonal(G) == 0)[0], zf) and np.array_equal(np.nonzero(yy == 0)[0], zt)


def test_tie63_is_a_tie_by_its_gap_margin_alone():
    coeffs, status, margin, sweeps, per = host("tie63")
    print("tie63: margins %s against TIE %.1e, RATIO_TIE %.1e" % (margin[0], LS.TIE, LS.RATIO_TIE))
    assert status[0] == 2 and margin[0][0] <= LS.TIE and margin[0][1] > LS.RATIO_TIE
    assert np.array_equal(per[0], reference("tie63", 0)[1]) and np.all(np.isfinite(coeffs[0]))


def test_a_column_past_the_digit_line_is_status_1_and_one_short_of_it_is_fitted():
    coeffs, status, margin, sweeps, per = host("past")
    assert status[0] == 1 and sweeps[0] == 0 and np.all(np.isnan(coeffs[0])) and not np.any(per[0])
    coeffs, status, margin, sweeps, per = host("near")
    assert status[0] == 0 and np.all(np.isfinite(coeffs[0])) and sweeps[0] >= 1
    for name, side in (("near", 1.0), ("past", -1.0)):        # and by a factor of two at least, either side
        G, _, _, fraw, _, _ = LS.centred_gram(*data(name), tuple(tuple(x) for x in basis(name)))
        ratio = (np.diagonal(G) / fraw)[-1]
        print("%s: centred / raw %.2e (2^-26 = %.2e)" % (name, ratio, LF.PIVOT_EPS))
        assert side * (np.log2(ratio) + 26) > 1.0


def _residual_gap(F, y, w, alpha):
    """sklearn's duality gap of one target in its residual form (centred data), as gen_golden_lassofit.py has it."""
    R = y - F @ w
    dn, r2 = np.max(np.abs(F.T @ R)), R @ R
    c = alpha / dn if dn > alpha else 1.0
    gap = 0.5 * (r2 + r2 * c * c) if dn > alpha else r2
    return gap + alpha * np.sum(np.abs(w)) - c * (R @ y)


def test_the_gap_form_difference_of_the_column_that_lost_its_digits_stays_inside_the_tie_margin():
    """near's control keeps 4.1e-8 of its sum of squares, so its Gram-form gap departs from the residual form by
    more than GAP_FORM_ERROR (the largest of the well-conditioned cases).  A status-0 decision lies more than TIE from
    its threshold, so it is safe while the departure stays below TIE: held here with a factor of 10 to spare."""
    lens, obs, ctrls = data("near")
    F, Y = LF.koopman_design(lens, obs, ctrls, basis("near"))
    Fc, Yc = F - F.mean(0), Y - Y.mean(0)
    log = []
    LS.lasso_fit_host(lens, obs, ctrls, [basis("near")], [(0, 1e-6)], gap_log=log)
    worst = max(abs(g - _residual_gap(Fc, Yc[:, t], w, 1e-6 * len(F))) / tol for _, t, w, g, tol in log)
    print("near: gap form difference %.2e of tol_t (GAP_FORM_ERROR %.1e, TIE %.1e)" % (worst, LS.GAP_FORM_ERROR, LS.TIE))
    assert len(log) >= 6 and LS.GAP_FORM_ERROR < worst <= LS.TIE / 10
    # the sweep test on the same case: its coefficients depart from sklearn's by HOST_ERR["near"] of max|w|, a ratio
    # at the decision therefore by that over 1e-4 of itself (3.8e-4, far above RATIO_TIE); near's closest sweep decision
    # lies 10 times further than that from its threshold, so none of its decisions can go the other way
    ratio_margin = host("near")[2][0][1]
    print("near: sweep-test margin %.2e against %.2e" % (ratio_margin, HOST_ERR["near"] / LS.TOL))
    assert ratio_margin >= 10 * HOST_ERR["near"] / LS.TOL


@pytest.mark.parametrize("name", ["zeroobs", "zeroedge"])
def test_zero_columns_keep_zero_coefficients_and_zero_targets_run_the_cap(name):
    zf, zt = zero_columns(name)
    coeffs, status, margin, sweeps, per = host(name)
    live = np.setdiff1d(np.arange(len(per[0])), zt)
    assert status[0] == 0 and sweeps[0] == 1000
    assert np.all(per[0][zt] == 1000) and np.array_equal(per[0], reference(name, 0)[1])
    assert not np.any(coeffs[0][zt]) and not np.any(coeffs[0][:, zf]) and np.all(np.isfinite(coeffs[0]))
    assert np.all(np.any(coeffs[0][live] != 0, axis=1))
    G, Q, yy, _, _, m = LS.centred_gram(*data(name), tuple(tuple(x) for x in basis(name)))
    _, its, mg = LS.coordinate_descent(G, Q, yy, CASES[name]["alphas"][0] * m)
    assert np.array_equal(its, per[0])
    assert np.all(np.isinf(mg[zt, 0])) and np.all(np.isfinite(mg[live, 0])) and margin[0][0] == mg[live, 0].min()


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
