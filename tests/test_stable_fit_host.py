"""sysid.stable_fit on the host: stabilize_host (the reference's stabilize_discrete restated) and stable_fit_host (the
device's Gram form in numpy) against the reference's goldens (tests/golden/gen_golden_stablefit.py), and the routing
of fit_linear_models(..., stable="device").

Tolerances come from the goldens, never from the code under test.  stabilize_host: 100 x the error recorded for it
against the reference when the goldens were made (the same algorithm, eigh for the reference's eig).  stable_fit_host:
100 x the larger of that and the case's recorded roundoff_response -- the change of the fit when every Gram entry is
perturbed by one rounding: another, equally valid eigensolver or summation order perturbs at that level.  Iteration and
trial counts must equal the reference's.  The size sweep (stablefit_cases.SWEEP) goes through the LAPACK route only.
"""
import numpy as np
import pytest

from autompc_amd import ARX, Koopman
from autompc_amd.evaluation import HoldoutModelEvaluator
from autompc_amd.sysid import linear_fit as LF
from autompc_amd.sysid import stable_fit as SF
from autompc_amd.tuning import BatchPipelineTuner, sample_koopman_config, sample_lqr_pipeline_configs

from stablefit_cases import (CASES, FITTED, SWEEP, SWEEP_FITTED, SWEEP_TIED, basis, data, declined_data, gold,
                             new_model, reference, rel_err, tolerance, trajs, without_lone_rows)


@pytest.mark.parametrize("name", FITTED)
def test_stabilize_host_matches_the_reference(name):
    g = gold(name)
    stats = {}
    A, B, error = SF.stabilize_host(*SF.koopman_rows(*data(name), basis(name)), stats=stats)
    assert (stats["iterations"], stats["trials"]) == (int(g["iterations"]), int(g["trials"]))
    err = rel_err(np.hstack([A, B]), reference(name))
    print(name, "stabilize_host against the reference", err, "recorded", float(g["host_err"]))
    assert err <= 100.0 * float(g["host_err"])
    assert abs(error - float(g["error"])) <= 100.0 * float(g["host_err"]) * float(g["error"])
    assert stats["margin"] > SF.TIE


@pytest.mark.parametrize("name", FITTED + SWEEP_FITTED)
def test_gram_form_matches_the_reference(name):
    g = gold(name)
    coeffs, status, error, its, trials, margin = SF.stable_fit_host(*data(name), [basis(name)])
    assert status[0] == 0
    assert (int(its[0]), int(trials[0])) == (int(g["iterations"]), int(g["trials"]))
    tol = tolerance(name)
    err = rel_err(coeffs[0], reference(name))
    print(name, "stable_fit_host against the reference", err, "tolerance", tol)
    assert err <= tol
    n = coeffs[0].shape[0]
    mod, ref_mod = (np.sort(np.abs(np.linalg.eigvals(M))) for M in (coeffs[0][:, :n], g["A"]))
    assert np.max(np.abs(mod - ref_mod)) <= tol * max(1.0, float(np.max(np.abs(g["A"]))))
    assert float(g["rho"]) <= 1.0 + 1e-9 and mod[-1] <= 1.0 + 1e-9
    assert margin[0] > SF.TIE and float(g["error_form_error"]) <= SF.ERROR_FORM_ERROR
    if name != "inactive":
        assert float(g["rho_lstsq"]) > 1.0                  # the constraint is active


def test_error_form_constant_is_the_measured_one():
    worst = max(float(gold(name)["error_form_error"]) for name in FITTED + SWEEP_FITTED)
    assert worst <= SF.ERROR_FORM_ERROR <= 2.0 * worst and SF.TIE == 100.0 * SF.ERROR_FORM_ERROR


@pytest.mark.parametrize("name", SWEEP_TIED)
def test_one_lifted_state_ties(name):
    """n = 1: status 2 with finite coefficients, as recorded when the golden was made."""
    g = gold(name)
    coeffs, status, error, its, trials, margin = SF.stable_fit_host(*data(name), [basis(name)])
    assert status[0] == 2 == int(g["status"]) and margin[0] <= SF.TIE
    assert np.all(np.isfinite(coeffs[0])) and np.isfinite(error[0])
    assert abs(np.linalg.eigvals(coeffs[0][:, :1])[0]) <= 1.0 + 1e-9


def test_the_sweep_is_the_table_the_issue_asked_for():
    sizes = {(c["no"], c["nu"]) for name, c in SWEEP.items() if name != "sweep_ragged"}
    assert sizes == {(n, nu) for n in (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 62, 63, 64) for nu in (1, 16)}
    for name in SWEEP:
        lens, obs, ctrls = data(name)
        assert np.array_equal(lens, SWEEP[name]["lengths"]) and obs.shape == (lens.sum(), SWEEP[name]["no"])
    lens = np.asarray(SWEEP["sweep_ragged"]["lengths"])
    ends = np.cumsum(lens) - 1
    assert 511 in ends and lens[list(ends).index(511) + 1] == 1       # a row split ends a trajectory; a lone row follows


def test_zero_successor_is_declined_by_the_polar_factor():
    """One observation whose successor is always exactly zero: the scaled Cholesky accepts the Gram, row 2 of W0 is
    exactly zero, so M'M of the first polar factor is singular and the Gram route declines -- status 1, no iteration,
    no trial, NaN coefficients."""
    lens, obs, ctrls = declined_data()
    b = ([0], [1.0])
    G, Q, yy = SF.design_gram(lens.astype(np.int64), obs, ctrls, ((0,), (1.0,)))
    nf, n = Q.shape
    W0, bad, _ = LF.solve_scaled_cholesky(np.concatenate([G, Q], axis=1), np.arange(nf), nf, n)
    assert not bad and np.all(W0[2] == 0.0) and np.all(np.isfinite(W0))
    with pytest.raises(SF.NotFitted, match="polar"):
        SF._gram_polar(W0[:, :n], "lapack")
    coeffs, status, error, its, trials, margin = SF.stable_fit_host(lens, obs, ctrls, [b])
    assert status[0] == 1 and its[0] == 0 and trials[0] == 0
    assert np.all(np.isnan(coeffs[0])) and np.isnan(error[0]) and margin[0] == np.inf


def test_length_one_trajectories_add_nothing_to_the_gram():
    """The ragged case without its length-1 trajectories (stablefit_cases.without_lone_rows: one of the four stays as
    padding, so that the rows of the second row split stay there): no design row goes, the Grams are equal."""
    lens, obs, ctrls = data("sweep_ragged")
    l2, o2, c2 = without_lone_rows(lens, obs, ctrls)
    assert list(l2) == [2, 509, 1, 30, 2, 40]
    key = ((0,), (1.0,))
    for a, b in zip(SF.design_gram(lens.astype(np.int64), obs, ctrls, key),
                    SF.design_gram(l2.astype(np.int64), o2, c2, key)):
        assert np.array_equal(a, b)


def test_duplicate_basis_is_declined():
    coeffs, status, error, its, trials, margin = SF.stable_fit_host(*data("dup"), [basis("dup")])
    assert status[0] == 1 and np.all(np.isnan(coeffs[0])) and its[0] == 0 and trials[0] == 0


@pytest.mark.parametrize("n", [1, 2, 5, 12])
def test_jacobi_eigh_is_an_eigendecomposition(n):
    rng = np.random.default_rng(n)
    A = rng.normal(size=(n, n))
    A = (A + A.T) / 2
    lam, V, sweeps = SF.jacobi_eigh(A)
    assert sweeps <= 10
    assert np.max(np.abs(V.T @ V - np.identity(n))) <= 1e-14
    assert np.max(np.abs((V * lam) @ V.T - A)) <= 1e-14 * max(1.0, np.max(np.abs(A))) * n
    assert np.max(np.abs(np.sort(lam) - np.linalg.eigvalsh(A))) <= 1e-14 * n * np.max(np.abs(A))
    for r in range(max(n + (n & 1) - 1, 0)):                # every round: disjoint pairs covering all indices
        p, q = SF.jacobi_pairs(n + (n & 1), r)
        assert sorted(np.concatenate([p, q])) == list(range(n + (n & 1))) and np.all(p < q)


@pytest.mark.parametrize("name", ["n2", "n12"])
def test_jacobi_route_gives_the_same_fit(name):
    g = gold(name)
    coeffs, status, _, its, trials, _ = SF.stable_fit_host(*data(name), [basis(name)], eig="jacobi")
    assert status[0] == 0 and (int(its[0]), int(trials[0])) == (int(g["iterations"]), int(g["trials"]))
    assert rel_err(coeffs[0], reference(name)) <= tolerance(name)


def _mixed(s):
    n68 = Koopman(s, method="stable", strict_reference=False, poly_basis=True, poly_degree=2, trig_basis=True,
                  trig_freq=1)                              # 17 observations x 4 functions = 68 > 64
    return [ARX(s, history=2), Koopman(s), Koopman(s, method="lasso", lasso_alpha=1e-2), new_model(s, "n51"),
            new_model(s, "n51"), n68]


def test_fit_linear_models_routes_stable_models(monkeypatch):
    s, tr = trajs("n51")
    models = _mixed(s)
    assert models[-1].state_dim == 68 > SF.MAX_N
    calls = []
    real = SF.stabilize_host
    monkeypatch.setattr(SF, "stabilize_host", lambda *a, **k: calls.append(a[0].shape[0]) or real(*a, **k))
    rep = LF.fit_linear_models(models, tr, backend="numpy", stable="device")
    assert [r["where"] for r in rep] == ["device", "device", "host", "device", "device", "host"]
    assert [r["reason"] for r in rep] == [None, None, "method", None, None, "size"]
    assert calls == [68]                                    # the over-size model, by stabilize_host
    assert (rep.device_fits, rep.host_fits) == (3, 2)
    for r in rep[3:]:
        assert {"iterations", "trials", "margin", "error"} <= set(r)
    g = gold("n51")
    assert rep[3]["iterations"] == int(g["iterations"]) and rep[3]["trials"] == int(g["trials"])
    assert rel_err(np.hstack([models[3].A, models[3].B]), reference("n51")) <= tolerance("n51")
    assert np.array_equal(models[3].A, models[4].A)         # equal configurations share one fit
    assert np.all(np.isfinite(models[5].A)) and np.max(np.abs(np.linalg.eigvals(models[5].A))) <= 1.0 + 1e-9
    # a duplicated basis function: status 1 on the Gram route, fitted by stabilize_host
    s, tr = trajs("dup")
    m = new_model(s, "dup")
    rep = LF.fit_linear_models([m], tr, backend="numpy", stable="device")
    assert (rep[0]["where"], rep[0]["reason"]) == ("host", "status 1") and calls == [68, 6]
    assert np.max(np.abs(np.linalg.eigvals(m.A))) <= 1.0 + 1e-9


def test_a_tie_sends_the_model_to_stabilize_host(monkeypatch):
    import functools
    s, tr = trajs("n2")
    margin = float(SF.stable_fit_host(*data("n2"), [basis("n2")])[5][0])
    calls = []
    real = SF.stabilize_host
    monkeypatch.setattr(SF, "stabilize_host", lambda *a, **k: calls.append(a[0].shape[0]) or real(*a, **k))
    monkeypatch.setattr(SF, "stable_fit_host", functools.partial(SF.stable_fit_host, tie=1.01 * margin))
    m = new_model(s, "n2")
    rep = LF.fit_linear_models([m], tr, backend="numpy", stable="device")
    assert (rep[0]["where"], rep[0]["reason"]) == ("host", "status 2") and calls == [2]
    assert (rep[0]["iterations"], rep[0]["trials"]) == (int(gold("n2")["iterations"]), int(gold("n2")["trials"]))
    assert rel_err(np.hstack([m.A, m.B]), reference("n2")) <= 100.0 * float(gold("n2")["host_err"])


def test_stable_defaults_to_host_and_is_checked():
    s, tr = trajs("n2")
    with pytest.raises(NotImplementedError):
        LF.fit_linear_models([new_model(s, "n2")], tr, backend="numpy")
    with pytest.raises(ValueError, match="stable"):
        LF.fit_linear_models([new_model(s, "n2")], tr, backend="numpy", stable="gpu")
    with pytest.raises(NotImplementedError):                # product terms: refused as by train()
        LF.fit_linear_models([Koopman(s, method="stable", product_terms=True)], tr, backend="numpy", stable="device")


# sample_koopman_config(default_rng(7)) five times, as the commit before the stable route drew them
PARENT_DRAWS = [
    {'method': 'lasso', 'lasso_alpha': 5.842054600678725, 'poly_basis': 'false', 'trig_basis': 'false',
     'product_terms': 'false'},
    {'method': 'lasso', 'lasso_alpha': 5.0406469457668977e-08, 'poly_basis': 'true', 'poly_degree': 4,
     'trig_basis': 'true', 'trig_freq': 7, 'product_terms': 'false'},
    {'method': 'lasso', 'lasso_alpha': 0.7157164853602431, 'poly_basis': 'true', 'poly_degree': 2,
     'trig_basis': 'false', 'product_terms': 'false'},
    {'method': 'lstsq', 'poly_basis': 'true', 'poly_degree': 7, 'trig_basis': 'true', 'trig_freq': 3,
     'product_terms': 'false'},
    {'method': 'lstsq', 'poly_basis': 'false', 'trig_basis': 'true', 'trig_freq': 8, 'product_terms': 'false'},
]


def test_sample_koopman_config_default_draws_are_unchanged_and_stable_can_be_asked_for():
    rng = np.random.default_rng(7)
    assert [sample_koopman_config(rng) for _ in range(5)] == PARENT_DRAWS
    rng = np.random.default_rng(8)
    draws = [sample_koopman_config(rng, methods=("lstsq", "lasso", "stable")) for _ in range(60)]
    stable = [d for d in draws if d["method"] == "stable"]
    assert stable and all("lasso_alpha" not in d for d in stable)
    assert {d["method"] for d in draws} == {"lstsq", "lasso", "stable"}
    with pytest.raises(ValueError):
        sample_koopman_config(rng, methods=("ridge",))
    s, _ = trajs("n2")
    cfgs = sample_lqr_pipeline_configs(s, 40, np.random.default_rng(9), model="koopman",
                                       koopman_methods=("lstsq", "lasso", "stable"))
    assert any(c.get_dictionary()["_model:method"] == "stable" for c in cfgs)


def test_stable_fit_options_are_checked_and_default_to_host():
    s, tr = trajs("n2")
    with pytest.raises(ValueError, match="stable_fit"):
        HoldoutModelEvaluator(s, tr, "rmse", np.random.default_rng(0), stable_fit="gpu")
    with pytest.raises(ValueError, match="stable_fit"):
        BatchPipelineTuner(s, None, stable_fit="gpu")
    assert BatchPipelineTuner(s, None).stable_fit == "host"
    assert HoldoutModelEvaluator(s, tr, "rmse", np.random.default_rng(0)).stable_fit == "host"
    assert HoldoutModelEvaluator(s, tr, "rmse", np.random.default_rng(0), linear_fit="device",
                                 stable_fit="device").stable_fit == "device"
