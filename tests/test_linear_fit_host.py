"""sysid.linear_fit on the host: gram_fit_host (the device algorithm in numpy) against the reference's goldens
(tests/golden/gen_golden_linfit.py), the sub-matrix property, the models that go back to train(), and the model
tuner's sampler.  No GPU."""
import numpy as np
import pytest

from autompc_amd import ARX, ARXFactory, Koopman, KoopmanFactory
from autompc_amd.sysid import linear_fit as LF
from autompc_amd.tuning.model_tuner import BatchModelTuner
from linfit_cases import (CASES, SHAPES, gold, gold_trajs, make_trajs, model_params, new_model, reference_coeffs,
                          rel_err, split_request, system, tolerance)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_gram_fit_host_matches_the_reference(name):
    g = gold(name)
    tags = [t for n, t in CASES if n == name]
    hist, bases = split_request(tags)
    coeffs, status, pivot = LF.gram_fit_host(g["traj_len"], g["obs"], g["ctrls"], hist, bases)
    order = [t for t in tags if t.startswith("arx")] + [t for t in tags if t.startswith("koop_")]
    for tag, c, st, p in zip(order, coeffs, status, pivot):
        ref = reference_coeffs(g, tag)
        err = rel_err(c, ref)
        print("%s %s: host error %.2e (recorded %.2e), pivot %.2e" % (name, tag, err, float(g["host_err_" + tag]), p))
        assert st == 0 and p >= c.shape[1] * LF.PIVOT_EPS
        assert c.shape == ref.shape and err <= tolerance(g, tag)


def test_history_k_is_a_submatrix_of_the_longest_history():
    """With the rows added in the same order an entry of the Gram does not depend on the design's other columns:
    history k cut from the history-10 Gram is history k's own Gram, and so are the coefficients, bit for bit."""
    g = gold("small")
    lens, obs, ctrls = g["traj_len"], g["obs"], g["ctrls"]
    F10, Y = LF.arx_design(lens, obs, ctrls, 10)
    G10 = LF.host_gram(F10, Y, ordered=True)
    together = LF.gram_fit_host(lens, obs, ctrls, [1, 2, 5, 10], ordered=True)[0]
    for i, k in enumerate((1, 2, 5, 10)):
        Fk, Yk = LF.arx_design(lens, obs, ctrls, k)
        idx = LF.arx_columns(k, 10, 3, 1)
        assert np.array_equal(Fk, F10[:, idx]) and np.array_equal(Yk, Y)
        Gk = LF.host_gram(Fk, Yk, ordered=True)
        assert np.array_equal(Gk[:, :len(idx)], G10[np.ix_(idx, idx)])
        assert np.array_equal(Gk[:, len(idx):], G10[idx, F10.shape[1]:])
        alone = LF.gram_fit_host(lens, obs, ctrls, [k], ordered=True)[0][0]
        assert np.array_equal(alone, together[i])


def test_design_rows_are_the_models_own():
    """arx_design / koopman_design build what ARX.train / Koopman.train regress on (ragged lengths, 1 and 2 included)."""
    s, trajs = gold_trajs("small")
    lens, obs, ctrls = LF.concat_trajs(trajs)
    m = ARX(s, history=5)
    F, Y = LF.arx_design(lens, obs, ctrls, 5)
    assert np.array_equal(F, np.concatenate([m._get_all_feature_vectors(t)[:-1] for t in trajs]))
    assert np.array_equal(Y, np.concatenate([t.obs[1:] for t in trajs]))
    k = Koopman(s, poly_basis=True, poly_degree=2)
    F, Y = LF.koopman_design(lens, obs, ctrls, k.device_lift())
    Z = [k._transform_observations(t.obs) for t in trajs]
    assert np.array_equal(F, np.concatenate([np.hstack([z[:-1], t.ctrls[:-1]]) for z, t in zip(Z, trajs)]))
    assert np.array_equal(Y, np.concatenate([z[1:] for z in Z]))


def test_fit_linear_models_numpy_backend_sets_the_models():
    s, trajs = gold_trajs("small")
    g = gold("small")
    tags = [t for n, t in CASES if n == "small"]
    models = [new_model(s, t) for t in tags] + [ARX(s, history=5)]          # (a repeated configuration)
    rep = LF.fit_linear_models(models, trajs, backend="numpy")
    assert [r["where"] for r in rep] == ["device"] * len(models) and rep.host_fits == 0
    assert rep.device_fits == len(tags)                                     # equal configurations are fitted once
    for m, tag in zip(models, tags + ["arx5"]):
        assert rel_err(model_params(m), reference_coeffs(g, tag)) <= tolerance(g, tag)
        ref = new_model(s, tag)
        ref.train(trajs)
        assert rel_err(model_params(m), model_params(ref)) <= tolerance(g, tag)
        assert m.A.shape == ref.A.shape and m.B.shape == ref.B.shape
    assert np.array_equal(models[-1].coeffs, models[tags.index("arx5")].coeffs)


def _same_as_train(m, trajs):
    ref = type(m)(m.system, **({"history": m.k} if isinstance(m, ARX) else dict(
        method=m.method, lasso_alpha=m.lasso_alpha, poly_basis=m.poly_basis, poly_degree=m.poly_degree,
        trig_basis=m.trig_basis, trig_freq=m.trig_freq, strict_reference=m.strict_reference)))
    ref.train(trajs)
    return np.array_equal(model_params(m), model_params(ref))


def test_models_the_gram_route_declines_go_to_train():
    s, trajs = gold_trajs("small")
    dup_poly = Koopman(s, poly_basis=True, poly_degree=3)                   # strict: x**3 twice
    dup_trig = Koopman(s, trig_basis=True, poly_degree=2)                   # strict: sin 2x, cos 2x twice
    lasso = Koopman(s, method="lasso", lasso_alpha=1e-4)
    ok = Koopman(s, poly_basis=True, poly_degree=3, strict_reference=False)  # x, x**2, x**3: no duplicate
    rep = LF.fit_linear_models([dup_poly, dup_trig, lasso, ok], trajs, backend="numpy")
    assert [(r["where"], r["reason"]) for r in rep] == [("host", "duplicate basis"), ("host", "duplicate basis"),
                                                        ("host", "method"), ("device", None)]
    assert rep.host_fits == 3
    for m in (dup_poly, dup_trig, lasso):
        assert _same_as_train(m, trajs)
    big = system(30, 2)
    rep = LF.fit_linear_models([ARX(big, history=10)], make_trajs(big, [40] * 12, 5), backend="numpy")
    assert rep[0]["where"] == "host" and rep[0]["reason"] == "size"


def test_rank_deficient_data_is_status_1_and_equals_train():
    """A control column held constant is the constant feature times a number: Cholesky cannot give lstsq's
    minimum-norm solution, so the solve declines and the model is fitted by train()."""
    s = system(3, 2)
    trajs = make_trajs(s, [30, 25, 40], 7)
    for t in trajs:
        t.ctrls[:, 1] = 0.75
    lens, obs, ctrls = LF.concat_trajs(trajs)
    _, status, pivot = LF.gram_fit_host(lens, obs, ctrls, [1, 3])
    assert list(status) == [1, 1] and np.all(pivot < 1e-12)          # (rounding-level pivots, or none)
    models = [ARX(s, history=3), ARX(s, history=1)]
    rep = LF.fit_linear_models(models, trajs, backend="numpy")
    assert [(r["where"], r["reason"]) for r in rep] == [("host", "status 1")] * 2 and rep.host_fits == 2
    assert all(_same_as_train(m, trajs) for m in models)


def test_model_tuner_default_sampler_draws_linear_configurations():
    s = system(3, 1)
    tuner = BatchModelTuner(s, evaluator=None)
    tuner.add_model_factory(ARXFactory(s))
    tuner.add_model_factory(KoopmanFactory(s))
    cfgs = tuner.ask(40, np.random.default_rng(0))
    seen = set()
    for c in cfgs:
        factory, sub = tuner.model_config(c)
        seen.add(factory.name)
        m = factory(sub, None, skip_train_model=True)
        if factory.name == "ARX":
            assert 1 <= m.k <= 10
        else:
            assert m.method in ("lstsq", "lasso") and 1 <= len(m.basis)
    assert seen == {"ARX", "Koopman"}


def test_linear_fit_option_is_checked():
    from autompc_amd.evaluation import HoldoutModelEvaluator
    s, trajs = gold_trajs("small")
    with pytest.raises(ValueError):
        HoldoutModelEvaluator(s, trajs, "rmse", np.random.default_rng(0), linear_fit="gpu")
    ev = HoldoutModelEvaluator(s, trajs, "rmse", np.random.default_rng(0))
    assert ev.linear_fit == "host"
