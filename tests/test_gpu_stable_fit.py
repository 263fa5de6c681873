"""Stable fits of Koopman models on the device (ampc_stable_fit, sysid/stable_fit.py) against the reference's goldens
(tests/golden/gen_golden_stablefit.py), the numpy form of the same recursion, themselves in other batches, and through
fit_linear_models.

Tolerance (stablefit_cases.tolerance, from the golden alone): max|d[A | B]| / max|[A | B]| <= 100 x the larger of the
restatement's recorded error against the reference and the case's recorded roundoff_response.  The device's Gram sums
differ from numpy's in the last bits and its eigensolver is Jacobi where numpy's is LAPACK's: equally valid, and
perturbing at the level of one rounding, which roundoff_response measures.  Iteration and trial counts are integers
and must equal the reference's.

The size sweep (stablefit_cases.SWEEP: every lifted size around the multiples of 16 at 1 and 16 controls, and a
ragged-rows case) adds, per case, the kernel's error against the residual of the matrices it returned, formed from the
data in extended precision, within TIE.  Every fitted sweep case ran the full 29 iterations in the reference: the two
early exits of the iteration (a second line-search failure in a row, the convergence test) stay unreached.
"""
import warnings

import numpy as np
import pytest

from autompc_amd import ARX, Koopman, KoopmanFactory, QuadCost, Task, Trajectory, _lib
from autompc_amd.evaluation import HoldoutModelEvaluator
from autompc_amd.evaluation.model_metrics import get_model_rmse
from autompc_amd.sysid import linear_fit as LF
from autompc_amd.sysid import stable_fit as SF
from autompc_amd.tuning import BatchPipelineTuner, LqrCandidateEvaluator, sample_lqr_pipeline_configs
from autompc_amd.tuning.configs import DictConfiguration

from stablefit_cases import (CASES, DECLINED, FITTED, MIXED, MIXED_BASES, SWEEP_FITTED, SWEEP_TIED, basis, data,
                             declined_data, gold, make_data, new_model, perturbation, reference, rel_err, residual,
                             tolerance, trajs, two_valued_data, without_lone_rows)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(CASES))
def test_device_fit_matches_the_reference_and_the_numpy_form(name):
    g = gold(name)
    lens, obs, ctrls = data(name)
    coeffs, status, error, its, trials, margin = _lib.stable_fit(lens, obs, ctrls, [basis(name)])
    if name == "dup":
        assert status[0] == 1 and np.all(np.isnan(coeffs[0])) and its[0] == 0 and trials[0] == 0
        return
    assert status[0] == 0
    assert (int(its[0]), int(trials[0])) == (int(g["iterations"]), int(g["trials"]))
    tol = tolerance(name)
    err = rel_err(coeffs[0], reference(name))
    host = SF.stable_fit_host(lens, obs, ctrls, [basis(name)])
    herr = rel_err(coeffs[0], host[0][0])
    print(name, "device against the reference", err, "against stable_fit_host", herr, "tolerance", tol)
    assert err <= tol and herr <= tol
    assert abs(error[0] - float(g["error"])) <= tol * float(g["error"])
    assert margin[0] > SF.TIE and abs(margin[0] - host[5][0]) <= 1e-3 * host[5][0] + tol
    n = coeffs[0].shape[0]
    assert np.max(np.abs(np.linalg.eigvals(coeffs[0][:, :n]))) <= 1.0 + 1e-9


def test_a_basis_gives_the_same_bits_alone_in_a_batch_permuted_and_repeated():
    lens, obs, ctrls = data("n12")                          # three bases of one data set: 3, 6 and 12 lifted states
    s = trajs("n12")[0]
    bases = [Koopman(s, method="stable").device_lift(),
             Koopman(s, method="stable", strict_reference=False, poly_basis=True, poly_degree=2).device_lift(),
             basis("n12")]
    batch = _lib.stable_fit(lens, obs, ctrls, bases)
    again = _lib.stable_fit(lens, obs, ctrls, bases)
    perm = _lib.stable_fit(lens, obs, ctrls, bases[::-1])
    for k, b in enumerate(bases):
        alone = _lib.stable_fit(lens, obs, ctrls, [b])
        for other, j in ((alone, 0), (again, k), (perm, 2 - k)):
            assert np.array_equal(batch[0][k], other[0][j])
            for f in (1, 4, 5):                             # status, trials, min_margin
                assert np.array_equal(batch[f][k], other[f][j])
    # the 3-state basis comes within 4.7e-11 of a line-search decision, on the host form as here: a tie (status 2) since
    # TIE is 1.3e-10 (the size sweep's error-form differences); the two larger ones are fitted
    host = SF.stable_fit_host(lens, obs, ctrls, bases)
    assert list(batch[1]) == [2, 0, 0] == list(host[1]) and np.all(np.isfinite(batch[0][0]))
    assert 3.5e-12 < batch[5][0] <= SF.TIE and abs(batch[5][0] - host[5][0]) <= 1e-3 * host[5][0]


@pytest.mark.parametrize("name", SWEEP_FITTED)
def test_sweep_device_fit_matches_the_reference_and_its_own_residual(name):
    """One device call per size of stablefit_cases.SWEEP (and its ragged-rows case): status, counts, the matrices
    against the reference and against stable_fit_host, and the kernel's error against the residual of the matrices it
    returned, formed from the data in extended precision.  That last difference is the one TIE (100 x the recorded
    error-form error) is the project's margin for; the residual is Lipschitz in the coefficients, so the bound holds
    for the exact algorithm."""
    g = gold(name)
    lens, obs, ctrls = data(name)
    b = basis(name)
    coeffs, status, error, its, trials, margin = _lib.stable_fit(lens, obs, ctrls, [b])
    assert status[0] == 0
    assert (int(its[0]), int(trials[0])) == (int(g["iterations"]), int(g["trials"]))
    tol = tolerance(name)
    err = rel_err(coeffs[0], reference(name))
    herr = rel_err(coeffs[0], SF.stable_fit_host(lens, obs, ctrls, [b])[0][0])
    res = residual(coeffs[0], lens, obs, ctrls, b)
    rerr = abs(error[0] - res) / res
    print(name, "device against the reference", err, "against stable_fit_host", herr, "tolerance", tol,
          "error against the residual", rerr, "TIE", SF.TIE)
    assert err <= tol and herr <= tol
    n = coeffs[0].shape[0]
    assert np.max(np.abs(np.linalg.eigvals(coeffs[0][:, :n]))) <= 1.0 + 1e-9
    assert rerr <= SF.TIE


@pytest.mark.parametrize("name", SWEEP_TIED)
def test_sweep_one_lifted_state_ties_on_the_device(name):
    lens, obs, ctrls = data(name)
    coeffs, status, error, its, trials, margin = _lib.stable_fit(lens, obs, ctrls, [basis(name)])
    host = SF.stable_fit_host(lens, obs, ctrls, [basis(name)])
    assert status[0] == 2 == host[1][0] == int(gold(name)["status"])
    assert np.all(np.isfinite(coeffs[0])) and np.isfinite(error[0])


def test_the_kernel_declines_a_singular_polar_factor():
    """stablefit_cases.DECLINED: the Cholesky accepts, the first polar factor inside stable_fgm_kernel does not."""
    lens, obs, ctrls = declined_data()
    coeffs, status, error, its, trials, margin = _lib.stable_fit(lens, obs, ctrls, [([0], [1.0])])
    assert status[0] == 1 and its[0] == 0 and trials[0] == 0
    assert coeffs[0].shape == (4, 6) and np.all(np.isnan(coeffs[0])) and np.isnan(error[0]) and margin[0] == np.inf


def test_a_declined_basis_leaves_its_neighbours_in_the_launch_alone():
    """Identity, identity + x^2, identity again on stablefit_cases.two_valued_data: x^2 of the 0 / 1 observation
    duplicates it, the middle basis is declined (status 1, by the Cholesky or by the polar factor) and the two good
    ones give the bits they give alone."""
    lens, obs, ctrls = two_valued_data()
    good, bad = ([0], [1.0]), ([0, 1], [1.0, 2.0])
    coeffs, status, error, its, trials, margin = _lib.stable_fit(lens, obs, ctrls, [good, bad, good])
    alone = _lib.stable_fit(lens, obs, ctrls, [good])
    assert list(status) == [0, 1, 0] and alone[1][0] == 0
    assert coeffs[1].shape == (8, 10) and np.all(np.isnan(coeffs[1])) and np.isnan(error[1])
    assert its[1] == 0 and trials[1] == 0 and margin[1] == np.inf
    for k in (0, 2):
        assert np.array_equal(coeffs[k], alone[0][0]) and np.all(np.isfinite(coeffs[k]))
        for f, other in zip((error, its, trials, margin), alone[2:]):
            assert np.array_equal(f[k], other[0])
    assert its[0] > 0 and trials[0] > 0


@pytest.fixture(scope="module")
def mixed():
    """stablefit_cases.MIXED: the data, stable_fit_host's fits of the three bases and their round-off responses."""
    lens, obs, ctrls = make_data(MIXED)
    host = SF.stable_fit_host(lens, obs, ctrls, MIXED_BASES)
    pert = SF.stable_fit_host(lens, obs, ctrls, MIXED_BASES, perturb=perturbation(MIXED["seed"]))
    assert np.all(host[1] == 0) and np.all(pert[1] == 0)
    assert np.array_equal(host[3], pert[3]) and np.array_equal(host[4], pert[4])
    return (lens, obs, ctrls), host, [rel_err(p, c) for p, c in zip(pert[0], host[0])]


def test_a_large_basis_gives_the_same_bits_alone_in_a_batch_permuted_and_repeated(mixed):
    """n = 21, 42 and 63 lifted states at 16 controls in one launch: three workgroups of different odd and even sizes
    against the same fits run alone, repeated and permuted, bit for bit; and against stable_fit_host at 100 x the
    round-off response, computed here from the host form alone."""
    (lens, obs, ctrls), host, response = mixed
    bases = MIXED_BASES
    batch = _lib.stable_fit(lens, obs, ctrls, bases)
    again = _lib.stable_fit(lens, obs, ctrls, bases)
    perm = _lib.stable_fit(lens, obs, ctrls, bases[::-1])
    for k, b in enumerate(bases):
        alone = _lib.stable_fit(lens, obs, ctrls, [b])
        for other, j in ((alone, 0), (again, k), (perm, 2 - k)):
            assert np.array_equal(batch[0][k], other[0][j])
            for f in (1, 2, 3, 4, 5):                       # status, error, iterations, trials, min_margin
                assert np.array_equal(batch[f][k], other[f][j])
    assert [c.shape for c in batch[0]] == [(21, 37), (42, 58), (63, 79)]
    assert np.all(batch[1] == 0)
    assert np.array_equal(batch[3], host[3]) and np.array_equal(batch[4], host[4])
    for k in range(3):
        err = rel_err(batch[0][k], host[0][k])
        print("mixed n", batch[0][k].shape[0], "device against stable_fit_host", err, "response", response[k])
        assert err <= 100.0 * response[k]


def test_length_one_trajectories_change_no_bit():
    """The ragged case without its length-1 trajectories (stablefit_cases.without_lone_rows: the rows that remain keep
    their row split and their order, one lone row staying as padding at the end of the first split): the same design
    rows in the same splits, so the coefficients are equal, bit for bit."""
    lens, obs, ctrls = data("sweep_ragged")
    l2, o2, c2 = without_lone_rows(lens, obs, ctrls)
    assert len(l2) < len(lens) and list(l2).count(1) == 1
    a = _lib.stable_fit(lens, obs, ctrls, [basis("sweep_ragged")])
    b = _lib.stable_fit(l2, o2, c2, [basis("sweep_ragged")])
    assert a[1][0] == 0
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x, y)
    assert np.array_equal(a[0][0], b[0][0])


def test_refusals():
    lens, obs, ctrls = data("n12")
    with pytest.raises(_lib.AmpcError, match="1..64 states"):
        _lib.stable_fit(lens, obs, ctrls, [([0] * 22, [1.0] * 22)])                     # 66 lifted states
    with pytest.raises(_lib.AmpcError, match="ctrl_dim"):
        _lib.stable_fit(lens, obs, np.zeros((len(obs), 17)), [basis("n12")])
    with pytest.raises(_lib.AmpcError, match="no trajectory has two rows"):
        _lib.stable_fit(np.ones(3, dtype=np.int32), obs[:3], ctrls[:3], [basis("n12")])
    with pytest.raises(_lib.AmpcError, match="no basis"):
        _lib.stable_fit(lens, obs, ctrls, [])
    assert _lib.load().ampc_version() == 114               # the entry is detected by its symbol, not by a bump


def test_tie_margin_turns_status_2():
    lens, obs, ctrls = data("n2")
    _, status, _, _, _, margin = _lib.stable_fit(lens, obs, ctrls, [basis("n2")])
    assert status[0] == 0
    c2, s2, _, _, _, m2 = _lib.stable_fit(lens, obs, ctrls, [basis("n2")], tie=1.01 * margin[0])
    assert s2[0] == 2 and m2[0] == margin[0] and np.all(np.isfinite(c2[0]))


def test_fit_linear_models_device_route_matches_the_numpy_route():
    s, tr = trajs("n51")
    n68 = dict(method="stable", strict_reference=False, poly_basis=True, poly_degree=2, trig_basis=True, trig_freq=1)

    def models():
        return [ARX(s, history=2), Koopman(s), new_model(s, "n51"), Koopman(s, **n68)]
    dev, host = models(), models()
    rd = LF.fit_linear_models(dev, tr, stable="device")
    rh = LF.fit_linear_models(host, tr, backend="numpy", stable="device")
    assert [(r["where"], r["reason"]) for r in rd] == [(r["where"], r["reason"]) for r in rh]
    assert [(r["where"], r["reason"]) for r in rd][2:] == [("device", None), ("host", "size")]
    assert (rd[2]["iterations"], rd[2]["trials"]) == (rh[2]["iterations"], rh[2]["trials"])
    assert rel_err(np.hstack([dev[2].A, dev[2].B]), reference("n51")) <= tolerance("n51")
    assert np.array_equal(dev[3].A, host[3].A)              # both by stabilize_host
    with pytest.raises(NotImplementedError):                # the default: train(), which refuses
        LF.fit_linear_models([new_model(s, "n51")], tr)


# the n51 case as KoopmanFactory builds it (strict-reference trig basis of poly_degree 1 = x, sin x, cos x)
N51_CFG = dict(method="stable", poly_basis="false", trig_basis="true", trig_freq=1, product_terms="false")


def test_evaluator_scores_a_device_fitted_stable_model_as_the_golden_matrices():
    """The k-step RMSE of the model fitted through ModelEvaluator(linear_fit="device", stable_fit="device") against
    the score of the golden's A, B, within the case tolerance, relative: the prediction is linear in [A | B] step by
    step, rho(A) <= 1 and the horizon is short, so the score moves by no larger a fraction than the matrices do."""
    s, tr = trajs("n51")
    g = gold("n51")
    horizon = 5
    holdout = [Trajectory(s, 30, t.obs[:30].copy(), t.ctrls[:30].copy()) for t in tr[:3]]      # equal to no training one
    ev = HoldoutModelEvaluator(s, tr, "rmse", np.random.default_rng(0), horizon=horizon, holdout_set=holdout,
                               linear_fit="device", stable_fit="device")
    assert len(ev.training_set) == len(tr) and ev.stable_fit == "device"
    cfgs = [DictConfiguration(N51_CFG), DictConfiguration(method="lstsq", poly_basis="false", trig_basis="false",
                                                          product_terms="false")]
    scores = np.asarray(ev.evaluate_batch(KoopmanFactory(s), cfgs))
    assert [(r["where"], r["reason"]) for r in ev.last_linear_fit] == [("device", None)] * 2
    assert ev.last_linear_fit[0]["trials"] == int(g["trials"])
    ref_model = new_model(s, "n51", method="lstsq")
    ref_model._set_matrices(g["A"], g["B"])
    want = get_model_rmse(ref_model, holdout, horizon=horizon)
    tol = tolerance("n51")
    diff = abs(scores[0] - want) / want
    print("evaluator: rmse %.12g, from the golden's matrices %.12g, relative difference %.2e (tolerance %.2e)"
          % (scores[0], want, diff, tol))
    assert np.all(np.isfinite(scores)) and diff <= tol
    # the default: the stable model goes to train(), which refuses
    host = HoldoutModelEvaluator(s, tr, "rmse", np.random.default_rng(0), horizon=horizon, holdout_set=holdout,
                                 linear_fit="device")
    with pytest.raises(NotImplementedError):
        host.evaluate_batch(KoopmanFactory(s), cfgs[:1])
    with pytest.raises(ValueError, match="stable_fit"):
        HoldoutModelEvaluator(s, tr, "rmse", np.random.default_rng(0), stable_fit="gpu")


def test_pipeline_tuner_lqr_batch_with_stable_draws_matches_the_host_fits(monkeypatch):
    """A batch of 8 LQR pipelines drawn from the reference's full Koopman space, fitted on the device, against the same
    batch with every stable model fitted by stabilize_host (the device call answered "status 1").  The drawn stable
    models within the device's size limit are kept as drawn; on 17 observations each of them lifts to the basis of the
    n51 golden (the strict-reference trig basis does not depend on trig_freq), so both fits lie within tolerance("n51")
    of the reference, and the costs are asserted at that tolerance, relative."""
    STEPS = 15
    s, tr = trajs("n51")
    NO, NU = s.obs_dim, s.ctrl_dim
    sur = ARX(s, history=1)
    sur.train(tr)
    task = Task(s)
    task.set_cost(QuadCost(s, np.eye(NO), 0.1 * np.eye(NU), np.eye(NO), goal=np.zeros(NO)))
    task.set_ctrl_bounds(-np.ones(NU), np.ones(NU))
    task.set_init_obs(np.full(NO, 0.3))
    task.set_num_steps(STEPS)
    factory = KoopmanFactory(s)
    small = [dict(method="lstsq", poly_basis="false", trig_basis="false", product_terms="false"),
             dict(method="lasso", lasso_alpha=1e-3, poly_basis="false", trig_basis="false", product_terms="false")]
    draws = sample_lqr_pipeline_configs(s, 8, np.random.default_rng(5), model="koopman",
                                        koopman_methods=("lstsq", "lasso", "stable"))
    cfgs, stable = [], []
    for i, c in enumerate(draws):
        d = c.get_dictionary()
        drawn = {k[len("_model:"):]: v for k, v in d.items() if k.startswith("_model:")}
        lift = factory(DictConfiguration(drawn), tr, skip_train_model=True).device_lift()
        if drawn["method"] == "stable" and len(lift[0]) * NO <= SF.MAX_N:
            stable.append(i)                                # kept as drawn
            assert all(np.array_equal(x, y) for x, y in zip(lift, basis("n51")))
        else:                                               # the other draws (up to 204 lifted states): two small models
            d = {k: v for k, v in d.items() if not k.startswith("_model:")}
            d.update({"_model:" + k: v for k, v in small[i % 2].items()})
        # finite horizons only: the infinite-horizon controller is out of scope here and scores inf whatever the model
        d["_ctrlr:finite_horizon"] = "true"
        # ... and short ones: the Riccati recursion on a lifted model with rho(A) at 1 amplifies a difference of the
        # matrices with every step (at the drawn horizons of up to 1000 two fits 1e-10 apart score 60 % apart)
        d["_ctrlr:horizon"] = 3 + i
        cfgs.append(DictConfiguration(d))
    assert len(stable) >= 2 and len({cfgs[i].get_dictionary()["_model:trig_freq"] for i in stable}) >= 2
    others = [i for i in range(8) if i not in stable]
    costs, fits = {}, {}
    real = _lib.stable_fit

    def declined(*a, **k):
        c, st, err, it, trn, mg = real(*a, **k)
        return c, np.ones_like(st), err, it, trn, mg
    for mode in ("device", "host"):
        if mode == "host":
            monkeypatch.setattr(_lib, "stable_fit", declined)
        ev = LqrCandidateEvaluator(s, task, surrogate=sur)
        tuner = BatchPipelineTuner(s, ev, batch_size=8, model_factory=factory, trajs=tr, linear_fit="device",
                                   lasso_fit="device", stable_fit="device")
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _, res = tuner.run(8, np.random.default_rng(2), configs=cfgs)
        costs[mode], fits[mode] = np.asarray(res.costs), tuner.linear_host_fits
    assert fits == {"device": 0, "host": 1}                 # the drawn stable models share one basis: fitted once
    a, b = costs["host"], costs["device"]
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(b))
    tol = tolerance("n51")
    diff = np.abs(a - b) / np.abs(a)
    print("tuner: stable draws %s, costs %s; max relative difference %.2e (tolerance %.2e)"
          % (stable, np.array2string(b, precision=4), diff.max(), tol))
    assert diff.max() <= tol
    assert np.array_equal(a[others], b[others])             # the lstsq and lasso models: the same fits
    with pytest.raises(ValueError, match="stable_fit"):
        BatchPipelineTuner(s, None, stable_fit="gpu")
    assert BatchPipelineTuner(s, None).stable_fit == "host"
