"""Lasso fits of Koopman models on the device (ampc_lasso_fit, sysid/lasso_fit.py) against the reference's goldens
(tests/golden/gen_golden_lassofit.py), the numpy form of the same algorithm, themselves in other batches, and through
fit_linear_models, the evaluator and the tuner.  Needs MI355X.

Tolerances.  Coefficients: max|dcoef| / max|coef| <= 100 x the error recorded for lasso_fit_host against the reference
on that case (lassofit_cases.tolerance): the device's Gram sums differ from numpy's in the last bits, and that
difference is carried through up to 1000 sweeps of a non-expansive map.  Sweep counts equal the golden's.  Scores:
10 x the coefficient tolerance x the horizon.  Bitwise claims are exact."""
import warnings

import numpy as np
import pytest

from autompc_amd import ARX, Koopman, KoopmanFactory, QuadCost, Task
from autompc_amd import _lib
from autompc_amd.evaluation import HoldoutModelEvaluator
from autompc_amd.sysid import lasso_fit as LS
from autompc_amd.sysid import linear_fit as LF
from autompc_amd.tuning import BatchPipelineTuner, LqrCandidateEvaluator, sample_lqr_pipeline_configs
from autompc_amd.tuning.configs import DictConfiguration
from lassofit_cases import (CASES, FOUR, HOST_ERR, SWEEP, TWO, basis, data, host, new_model, reference, rel_err,
                            tolerance, trajs, without_lone_rows, zero_columns)
from linfit_cases import make_trajs, model_params, system

pytestmark = pytest.mark.gpu


def _fit(name, alphas=None, bases=None, configs=None):
    lens, obs, ctrls = data(name)
    alphas = CASES[name]["alphas"] if alphas is None else alphas
    return _lib.lasso_fit(lens, obs, ctrls, bases or [basis(name)], configs or [(0, a) for a in alphas])


@pytest.mark.parametrize("name", ["n13", "dup", "n74", "big", "zero"])
def test_device_fit_matches_the_reference_and_takes_its_sweeps(name):
    coeffs, status, margin, sweeps = _fit(name)
    for k, alpha in enumerate(CASES[name]["alphas"]):
        ref, n_iter = reference(name, k)
        err = rel_err(coeffs[k], ref)
        print("%s alpha %g: device error %.2e (tolerance %.2e), sweeps %d (golden %d), margins %s"
              % (name, alpha, err, tolerance(name), sweeps[k], n_iter.max(), margin[k]))
        assert status[k] == 0 and sweeps[k] == n_iter.max()
        assert err <= tolerance(name)
    if name == "zero":
        assert not np.any(coeffs[0][:, -1])                   # the untouched column: exactly 0


def _same(a, b, i, j=0):
    """Configuration i of fit a and configuration j of fit b: coefficients, status, margins and sweeps, bit for bit."""
    return (np.array_equal(a[0][i], b[0][j], equal_nan=True) and a[1][i] == b[1][j]
            and np.array_equal(a[2][i], b[2][j]) and a[3][i] == b[3][j])


@pytest.mark.parametrize("name", list(SWEEP))
def test_sweep_device_fit_matches_the_reference_at_every_slot_edge(name):
    """Feature counts on both sides of each 64-lane slot edge and of a 16-column tile edge, on 606 ragged rows in two
    row splits (length-1 trajectories at a split's first and the data's last row, a trajectory ending on row 511)."""
    coeffs, status, margin, sweeps = _fit(name)
    ref, n_iter = reference(name, 0)
    hc, hs, hm, hw, _ = host(name)
    err = rel_err(coeffs[0], ref)
    print("%s: device error %.2e (tolerance %.2e), against the numpy form %.2e, sweeps %d (reference %d), margins %s"
          % (name, err, tolerance(name), rel_err(coeffs[0], hc[0]), sweeps[0], n_iter.max(), margin[0]))
    assert status[0] == 0 and sweeps[0] == n_iter.max()
    assert status[0] == hs[0] and sweeps[0] == hw[0]
    assert err <= tolerance(name)


def test_lone_rows_behind_the_split_boundary_do_not_change_a_bit():
    """s65 without the two length-1 trajectories after data row 511 (the one that opens split 1 and the one that
    closes the data): those rows contribute exact zeros, m is unchanged and every design row stays in its split, so
    coefficients, margins and sweeps are equal bit for bit.  Removing the lone rows at data rows 0 and 41 as well moves
    two design rows across the boundary; the partial sums then regroup (the numpy form differs by 8e-15 of the fit
    there too), so that twin is held to the coefficient tolerance only."""
    lens, obs, ctrls = data("s65")
    full = _fit("s65")
    tl, to, tc = without_lone_rows(lens, obs, ctrls, after=512)
    assert list(tl) == [1, 40, 1, 200, 270, 90, 2] and len(to) == 604
    twin = _lib.lasso_fit(tl, to, tc, [basis("s65")], [(0, 1e-1)])
    assert _same(full, twin, 0)
    tl, to, tc = without_lone_rows(lens, obs, ctrls)
    assert list(tl) == [40, 200, 270, 90, 2] and len(to) == 602
    moved = _lib.lasso_fit(tl, to, tc, [basis("s65")], [(0, 1e-1)])
    err = rel_err(moved[0][0], full[0][0])
    print("s65 with the boundary two design rows later: %.2e of the fit (tolerance %.2e), bits equal: %s"
          % (err, tolerance("s65"), _same(full, moved, 0)))
    assert moved[1][0] == 0 and moved[3][0] == full[3][0] and err <= tolerance("s65")


def test_a_real_tie_is_status_2_with_the_hosts_margins():
    coeffs, status, margin, sweeps = _fit("tie63")
    hc, hs, hm, hw, _ = host("tie63")
    ref, n_iter = reference("tie63", 0)
    print("tie63: device margins %s, host %s, error %.2e (tolerance %.2e)"
          % (margin[0], hm[0], rel_err(coeffs[0], ref), tolerance("tie63")))
    assert status[0] == 2 == hs[0] and margin[0][0] <= LS.TIE and margin[0][1] > LS.RATIO_TIE
    assert np.all(np.abs(margin[0] - hm[0]) <= 1e-6 * hm[0])
    assert sweeps[0] == n_iter.max() and rel_err(coeffs[0], ref) <= tolerance("tie63")


@pytest.mark.parametrize("name", ["zeroobs", "zeroedge"])
def test_zero_features_and_zero_targets_stay_zero_and_run_the_cap(name):
    zf, zt = zero_columns(name)
    coeffs, status, margin, sweeps = _fit(name)
    hc, hs, hm, hw, _ = host(name)
    ref, n_iter = reference(name, 0)
    err = rel_err(coeffs[0], ref)
    print("%s: device error %.2e (tolerance %.2e), margins %s, host %s" % (name, err, tolerance(name), margin[0], hm[0]))
    assert status[0] == 0 and sweeps[0] == 1000 == n_iter.max()
    assert np.all(np.isfinite(coeffs[0]))
    assert not np.any(coeffs[0][zt]) and not np.any(coeffs[0][:, zf])
    assert err <= tolerance(name)
    assert np.all(np.isfinite(margin[0])) and np.all(np.abs(margin[0] - hm[0]) <= 1e-6 * hm[0])


def test_the_digit_line_is_drawn_where_the_host_draws_it():
    coeffs, status, margin, sweeps = _fit("near")
    ref, n_iter = reference("near", 0)
    err = rel_err(coeffs[0], ref)
    print("near: device error %.2e (tolerance %.2e), sweeps %d" % (err, tolerance("near"), sweeps[0]))
    assert status[0] == 0 == host("near")[1][0] and sweeps[0] == n_iter.max() and err <= tolerance("near")
    coeffs, status, margin, sweeps = _fit("past")
    assert status[0] == 1 == host("past")[1][0] and sweeps[0] == 0 and np.all(np.isnan(coeffs[0]))
    assert np.all(np.isinf(margin[0]))


X_ONLY = ([0], [1.0])


def _alone_equals_batch(lens, obs, ctrls, bases, configs, bad=()):
    """Fits the batch, then every configuration alone with only its basis in the call: equal bits.  Returns the
    batch's status."""
    allf = _lib.lasso_fit(lens, obs, ctrls, bases, configs)
    for i, (b, a) in enumerate(configs):
        one = _lib.lasso_fit(lens, obs, ctrls, [bases[b]], [(0, a)])
        assert _same(allf, one, i), (i, b, a)
        assert (allf[1][i] == 1) == (b in bad)
        if b in bad:
            assert np.all(np.isnan(allf[0][i])) and allf[3][i] == 0
        else:
            assert np.all(np.isfinite(allf[0][i])) and allf[3][i] >= 1
    return allf[1]


def test_one_launch_of_unlike_designs_equals_each_design_alone():
    """Designs of 65, 33 and 129 features (ldp 128, 64, 192) and an unused basis between them in one
    call: lasso_centre_kernel's early return for the small ones, design_slot and the d.used skip."""
    lens, obs, ctrls = data("s129")
    bases = [TWO, X_ONLY, ([0, 1, 2, 3], [1.0, 3.0, 2.0, 2.0]), FOUR]          # basis 2 is never named
    configs = [(3, 1e-1), (0, 1e-1), (1, 1e-2), (3, 1.0), (1, 1e-1), (0, 1e-2)]
    status = _alone_equals_batch(lens, obs, ctrls, bases, configs)
    assert not np.any(status == 1)
    # the four-lift design alone is the sweep case
    assert _same(_lib.lasso_fit(lens, obs, ctrls, bases, configs), _fit("s129"), 0)
    # the control is a feature of every design: held at 0.75 it takes them all to status 1
    held = np.array(ctrls)
    held[:, 0] = 0.75
    coeffs, status, margin, sweeps = _lib.lasso_fit(lens, obs, held, bases, configs)
    assert np.all(status == 1) and not np.any(sweeps) and all(np.all(np.isnan(c)) for c in coeffs)


def test_a_bad_design_between_two_good_ones_is_the_only_status_1():
    """cos 0x is the constant 1: its centred sum of squares is 0 of a raw 597, bad for that design only (one flag
    per design).  zeroedge's data: the neighbours carry zero features on lanes 31 and 63 and a zero control."""
    lens, obs, ctrls = data("zeroedge")
    bases = [X_ONLY, ([0, 3], [1.0, 0.0]), TWO]
    configs = [(0, 1e-1), (1, 1e-1), (2, 1e-1), (1, 1e-2), (0, 1e-2)]
    _alone_equals_batch(lens, obs, ctrls, bases, configs, bad=(1,))
    assert _same(_lib.lasso_fit(lens, obs, ctrls, bases, configs), _fit("zeroedge"), 2)


def test_device_fit_matches_the_numpy_form():
    for name in ("n13", "zero", "dup"):
        lens, obs, ctrls = data(name)
        cfg = [(0, a) for a in CASES[name]["alphas"]]
        hc, hs, hm, hw = LS.lasso_fit_host(lens, obs, ctrls, [basis(name)], cfg)
        dc, ds, dm, dw = _fit(name)
        assert np.array_equal(hs, ds) and np.array_equal(hw, dw)
        for k in range(len(cfg)):
            print("%s alpha %g: device against numpy %.2e" % (name, cfg[k][1], rel_err(dc[k], hc[k])))
            assert rel_err(dc[k], hc[k]) <= tolerance(name)


def test_constant_column_comes_back_status_1():
    coeffs, status, margin, sweeps = _fit("const")
    assert status[0] == 1 and sweeps[0] == 0 and np.all(np.isnan(coeffs[0]))


def test_a_configuration_does_not_depend_on_the_batch():
    bases = [basis("n13"), ([0], [1.0]), ([0, 2, 3], [1.0, 1.0, 1.0])]
    configs = [(0, 1e2), (0, 1.0), (1, 1e-2), (0, 1e-2), (2, 1e-3), (0, 1e-6), (1, 1.0)]
    allc, st, mg, sw = _fit("n13", bases=bases, configs=configs)
    again = _fit("n13", bases=bases, configs=configs)
    assert all(np.array_equal(a, b) for a, b in zip(allc, again[0])) and np.array_equal(mg, again[2])
    perm = [4, 6, 0, 5, 2, 1, 3]
    pc, ps, pm, pw = _fit("n13", bases=bases[::-1], configs=[(2 - configs[i][0], configs[i][1]) for i in perm])
    for j, i in enumerate(perm):
        assert np.array_equal(pc[j], allc[i]) and ps[j] == st[i] and np.array_equal(pm[j], mg[i]) and pw[j] == sw[i]
    for i, (b, a) in enumerate(configs):
        oc, os_, om, ow = _fit("n13", bases=[bases[b]], configs=[(0, a)])
        assert np.array_equal(oc[0], allc[i]) and os_[0] == st[i] and np.array_equal(om[0], mg[i]) and ow[0] == sw[i]
    for part in (configs[:3], configs[3:]):
        sc, ss, sm, swp = _fit("n13", bases=bases, configs=part)
        for j, cfg in enumerate(part):
            i = configs.index(cfg)
            assert np.array_equal(sc[j], allc[i]) and ss[j] == st[i] and np.array_equal(sm[j], mg[i]) and swp[j] == sw[i]


def test_a_constructed_tie_is_status_2_and_bad_arguments_are_refused():
    lens, obs, ctrls = data("n13")
    _, status, margin, _ = _fit("n13", alphas=[1e-2])
    assert status[0] == 0
    _, s2, m2, _ = _lib.lasso_fit(lens, obs, ctrls, [basis("n13")], [(0, 1e-2)], ratio_tie=1.01 * margin[0][1])
    assert s2[0] == 2 and np.array_equal(m2, margin)
    with pytest.raises(_lib.AmpcError, match="alpha"):
        _lib.lasso_fit(lens, obs, ctrls, [basis("n13")], [(0, -1.0)])
    with pytest.raises(_lib.AmpcError, match="256 states"):
        _lib.lasso_fit(lens, obs, ctrls, [([0] * 86, [1.0] * 86)], [(0, 1.0)])
    with pytest.raises(_lib.AmpcError, match="ctrl_dim"):
        _lib.lasso_fit(lens, obs, np.zeros((len(obs), 17)), [basis("n13")], [(0, 1.0)])
    assert _lib.load().ampc_version() == 114


def _mixed(s):
    dup = dict(poly_basis=True, poly_degree=3, trig_basis=True)
    return [ARX(s, history=2), Koopman(s), new_model(s, "n13", 1e-2), Koopman(s, method="lasso", lasso_alpha=1e-1, **dup),
            new_model(s, "n13", 1e-2), new_model(s, "n13", 1.0)]


def test_fit_linear_models_device_route_matches_the_numpy_backend():
    s, tr = trajs("n13")
    dev, host = _mixed(s), _mixed(s)
    rd = LF.fit_linear_models(dev, tr, lasso="device")
    rh = LF.fit_linear_models(host, tr, backend="numpy", lasso="device")
    assert [(r["where"], r["reason"]) for r in rd] == [("device", None)] * 6 == [(r["where"], r["reason"]) for r in rh]
    assert rd.device_fits == 5 and rd.host_fits == 0
    for i in (2, 3, 4, 5):
        assert rd[i]["sweeps"] == rh[i]["sweeps"] and rd[i]["margin"] > 0
    for i, (a, b) in enumerate(zip(dev, host)):
        err = rel_err(model_params(a), model_params(b))
        print("mixed batch model %d: device against numpy %.2e" % (i, err))
        assert err <= (1e-9 if i == 3 else max(tolerance("n13"), 1e-13))     # 3: the basis with duplicates
    rep = LF.fit_linear_models(_mixed(s), tr)                                   # the default: lasso models to train()
    assert [(r["where"], r["reason"]) for r in rep] == [("device", None)] * 2 + [("host", "method")] * 4


# the largest recorded error of the cases on unaltered data (near, a column that lost its digits on purpose, apart)
WORST_ERR = max(HOST_ERR[n] for n in ("n13", "dup", "n74", "big", "zero"))
LASSO_CFGS = [dict(method="lasso", lasso_alpha=a, poly_basis=p, poly_degree=2, trig_basis="false", product_terms="false")
              for a, p in ((1e-1, "false"), (1e-2, "true"), (1e-3, "false"), (1e-2, "true"))]


def test_holdout_evaluator_device_lasso_fit_matches_the_host_fit():
    s = system(3, 1)
    tr = make_trajs(s, [60] * 12, 11)
    cfgs = [DictConfiguration({k: v for k, v in c.items() if k != "poly_degree" or c["poly_basis"] == "true"})
            for c in LASSO_CFGS] + [DictConfiguration(method="lstsq", poly_basis="false", trig_basis="false",
                                                      product_terms="false")]
    horizon = 5
    kw = dict(horizon=horizon, holdout_prop=0.25, linear_fit="device")
    host = HoldoutModelEvaluator(s, tr, "rmse", np.random.default_rng(3), **kw)
    dev = HoldoutModelEvaluator(s, tr, "rmse", np.random.default_rng(3), lasso_fit="device", **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = np.asarray(host.evaluate_batch(KoopmanFactory(s), cfgs))
    b = np.asarray(dev.evaluate_batch(KoopmanFactory(s), cfgs))
    assert [(r["where"], r["reason"]) for r in host.last_linear_fit] == [("host", "method")] * 4 + [("device", None)]
    assert all(r["where"] == "device" for r in dev.last_linear_fit) and dev.last_linear_fit.host_fits == 0
    assert all("sweeps" in r for r in dev.last_linear_fit[:4])
    tol = 10 * 100 * WORST_ERR * horizon
    diff = np.abs(a - b) / np.abs(a)
    print("evaluator: scores %s; max relative score difference %.2e (tolerance %.2e)"
          % (np.array2string(b, precision=4), diff.max(), tol))
    assert np.all(np.isfinite(a)) and diff.max() <= tol
    assert a[4] == b[4] and b[1] == b[3]


def test_pipeline_tuner_lqr_batch_device_lasso_fit_matches_the_host_fit():
    NO, NU, STEPS = 3, 1, 15
    s = system(NO, NU)
    tr = make_trajs(s, [60] * 8, 21)
    sur = ARX(s, history=2)
    sur.train(tr)
    task = Task(s)
    task.set_cost(QuadCost(s, np.eye(NO), 0.1 * np.eye(NU), np.eye(NO), goal=np.zeros(NO)))
    task.set_ctrl_bounds(-np.ones(NU), np.ones(NU))
    task.set_init_obs(np.full(NO, 0.3))
    task.set_num_steps(STEPS)
    cfgs = []
    for i, c in enumerate(sample_lqr_pipeline_configs(s, 16, np.random.default_rng(4), model="koopman")):
        d = {k: v for k, v in c.get_dictionary().items() if not k.startswith("_model:")}
        d.update({"_model:" + k: v for k, v in LASSO_CFGS[i % 4].items()
                  if k != "poly_degree" or LASSO_CFGS[i % 4]["poly_basis"] == "true"})
        cfgs.append(DictConfiguration(d))
    costs, fits = {}, {}
    for mode in ("host", "device"):
        ev = LqrCandidateEvaluator(s, task, surrogate=sur)
        tuner = BatchPipelineTuner(s, ev, batch_size=16, model_factory=KoopmanFactory(s), trajs=tr, linear_fit="device",
                                   lasso_fit=mode)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _, res = tuner.run(16, np.random.default_rng(2), configs=cfgs)
        costs[mode], fits[mode] = np.asarray(res.costs), tuner.linear_host_fits
    assert fits == {"host": 3, "device": 0}
    a, b = costs["host"], costs["device"]
    assert np.array_equal(np.isfinite(a), np.isfinite(b)) and np.isfinite(a).sum() >= 4
    f = np.isfinite(a)
    tol = 10 * 100 * WORST_ERR * STEPS
    diff = np.abs(a[f] - b[f]) / np.abs(a[f])
    print("tuner: max relative score difference %.2e (tolerance %.2e)" % (diff.max(), tol))
    assert diff.max() <= tol
