"""Thresholded SINDy fits on the device (ampc_sindy_fit, sysid/sindy_fit.py) against the models' own train(), the
numpy form of the same algorithm, themselves in other batches, and through the evaluator.  Needs MI355X.

Tolerance (DESIGN 6d's rule): the device may be at most 100 x as far from train() as stlsq_gram_host is on that case,
floor 1e-13, both computed here on the host; the support must be equal.  No case may decline: the smallest threshold
margin of the cases is 2.2e-5, the smallest squared pivot 1.1e-6 n.
"""
import numpy as np
import pytest

from autompc_amd import ARXFactory, SINDy, SINDyFactory
from autompc_amd import _lib
from autompc_amd.evaluation import HoldoutModelEvaluator
from autompc_amd.sysid import sindy_fit as SF
from autompc_amd.tuning.configs import DictConfiguration
from linfit_cases import make_trajs, system
from sindy_fit_cases import ELIGIBLE, LONG, data, host_fit, new_model, rel_err, request, same_support, trained

pytestmark = pytest.mark.gpu


def _fit(name, ks, **extra):
    args, kw = request(name, ks)
    return _lib.sindy_fit(*args, **dict(kw, **extra))


@pytest.mark.parametrize("name,k", ELIGIBLE)
def test_device_matches_train(name, k):
    ref = trained(name, k)
    host = host_fit(name, k)
    coeffs, status, pivot, margin, iters = _fit(name, [k])
    tol = max(100.0 * rel_err(host[0], ref), 1e-13)
    err = rel_err(coeffs[0], ref)
    print("sindy fit %s %d (%d features): device vs train() %.2e, stlsq_gram_host vs train() %.2e, device vs "
          "stlsq_gram_host %.2e, tolerance %.2e; pivot^2 %.2e, margin %.2e, %d solves"
          % (name, k, ref.shape[1], err, rel_err(host[0], ref), rel_err(coeffs[0], host[0]), tol, pivot[0], margin[0],
             iters[0]))
    assert status[0] == 0
    assert same_support(coeffs[0], ref) and err <= tol
    assert iters[0] == host[4] and same_support(coeffs[0], host[0])


@pytest.mark.parametrize("name", ["small", "hc"])
def test_a_configuration_has_the_same_bits_in_any_batch(name):
    ks = [k for n, k in ELIGIBLE if n == name]
    full = _fit(name, ks)
    again = _fit(name, ks)
    perm = ks[::-1][2:] + ks[::-1][:2]
    permuted = _fit(name, perm)
    assert np.all(full[1] == 0)
    for i, k in enumerate(ks):
        alone = _fit(name, [k])
        j = perm.index(k)
        for other, slot in ((again, i), (permuted, j), (alone, 0)):
            assert np.array_equal(full[0][i], other[0][slot])
            assert full[2][i] == other[2][slot] and full[3][i] == other[3][slot] and full[4][i] == other[4][slot]


@pytest.mark.parametrize("name,k", LONG)
def test_three_row_splits(name, k):
    ref = trained(name, k)
    coeffs, status, pivot, margin, iters = _fit(name, [k])
    host = host_fit(name, k)
    assert status[0] == 0 and same_support(coeffs[0], ref)
    assert rel_err(coeffs[0], ref) <= max(100.0 * rel_err(host[0], ref), 1e-13)


def test_near_tie_and_max_iter_on_the_device():
    (lens, obs, ctrls, designs, _), _ = request("small", [3])
    first = _lib.sindy_fit(lens, obs, ctrls, designs, [(0, False, 0.0)], max_iter=1)
    assert first[1][0] == 0 and first[4][0] == 1 and np.isinf(first[3][0])
    w = np.sort(np.abs(first[0][0][0]))[len(first[0][0][0]) // 2]
    thr = float(w * (1.0 + 2.0 ** -24))
    _, status, _, margin, _ = _lib.sindy_fit(lens, obs, ctrls, designs, [(0, False, thr), (0, False, 0.02)])
    assert list(status) == [2, 0] and margin[0] < SF.TIE_MARGIN
    m = new_model("small", 3, threshold=thr)
    rep = SF.fit_sindy_models([m], data("small")[1])
    ref = new_model("small", 3, threshold=thr)
    ref.train(data("small")[1])
    assert rep[0]["reason"] == "status 2" and rep.host_fits == 1 and np.array_equal(m.coefficients, ref.coefficients)
    # max_iter ends the loop right after a drop (natural count 7)
    m2, ref2 = new_model("hc", 3), new_model("hc", 3)
    rep = SF.fit_sindy_models([m2], data("hc")[1], max_iter=2)
    ref2.train(data("hc")[1], max_iter=2)
    assert rep[0]["where"] == "device" and rep[0]["iters"] == 2 and same_support(m2.coefficients, ref2.coefficients)
    assert rel_err(m2.coefficients, ref2.coefficients) <= 1e-9


def test_refusals():
    (lens, obs, ctrls, designs, configs), kw = request("small", [3])
    with pytest.raises(_lib.AmpcError, match="max_iter < 1"):
        _lib.sindy_fit(lens, obs, ctrls, designs, configs, max_iter=0)
    with pytest.raises(_lib.AmpcError, match="needs continuous targets"):
        _lib.sindy_fit(lens, obs, ctrls, designs, [(0, True, 0.1)])
    s17 = system(17, 6)
    big = SINDy(s17, poly_basis=True, poly_degree=8, trig_basis=True, trig_freq=3)
    a, _ = request("hc", [1])
    with pytest.raises(_lib.AmpcError, match="1..272 features"):
        _lib.sindy_fit(a[0], a[1], a[2], [big.library], [(0, False, 0.01)])
    wide = np.zeros((len(obs), 65))
    with pytest.raises(_lib.AmpcError, match="obs_dim must be in 1..64"):
        _lib.sindy_fit(lens, wide, ctrls, designs, configs)
    bad = tuple(np.array(x) for x in designs[0])
    bad[1][0] = 4                                               # a variable past [obs | ctrls]
    with pytest.raises(_lib.AmpcError, match="variable out of range"):
        _lib.sindy_fit(lens, obs, ctrls, [bad], configs)


class _MixedFactory:
    """SINDy configurations and, for ``family == "arx"``, an ARX model: one ``evaluate_batch`` with both."""
    name = "mixed"

    def __init__(self, s):
        self.sindy, self.arx = SINDyFactory(s), ARXFactory(s)

    def __call__(self, cfg, train_trajs, silent=False, skip_train_model=False):
        d = dict(cfg.get_dictionary())
        family = d.pop("family")
        return (self.arx if family == "arx" else self.sindy)(DictConfiguration(d), train_trajs, silent=silent,
                                                              skip_train_model=skip_train_model)


def test_holdout_evaluator_fits_a_batch_in_one_call_and_agrees_with_the_host_fit(monkeypatch):
    s = system(3, 1)
    trajs = make_trajs(s, [60] * 12, 11)
    trig = dict(family="sindy", trig_basis="true", trig_freq=1)
    poly = dict(family="sindy", poly_basis="true", poly_degree=3)
    kws = [dict(trig, threshold=0.02, time_mode="discrete"), dict(poly, threshold=0.01, time_mode="discrete"),
           dict(family="arx", history=2),
           dict(trig, threshold=0.05, time_mode="continuous"), dict(poly, threshold=0.03, time_mode="discrete")]
    cfgs = [DictConfiguration(kw) for kw in kws]
    horizon = 5
    kw = dict(horizon=horizon, holdout_prop=0.25, sindy_kstep="device")
    host = HoldoutModelEvaluator(s, trajs, "rmse", np.random.default_rng(3), **kw)
    dev = HoldoutModelEvaluator(s, trajs, "rmse", np.random.default_rng(3), sindy_fit="device", **kw)
    calls = []
    real = _lib.sindy_fit
    monkeypatch.setattr(_lib, "sindy_fit", lambda *a, **k: calls.append(len(a[4])) or real(*a, **k))
    a = np.asarray(host.evaluate_batch(_MixedFactory(s), cfgs))
    assert calls == [] and host.last_sindy_fit is None
    b = np.asarray(dev.evaluate_batch(_MixedFactory(s), cfgs))
    rep = dev.last_sindy_fit
    assert calls == [4] and len(rep) == 4 and rep.host_fits == 0 and rep.device_fits == 4 and rep.designs == 2
    assert all(r["where"] == "device" for r in rep)
    # coefficient tolerance of the batch: the rule above on the training set, the largest of its four configurations
    ctol = 0.0
    for kw_ in kws:
        if kw_["family"] != "sindy":
            continue
        d = {k: v for k, v in kw_.items() if k != "family"}
        m, ref = SINDyFactory(s)(DictConfiguration(d), dev.training_set, skip_train_model=True), None
        ref = SINDyFactory(s)(DictConfiguration(d), dev.training_set)
        SF.fit_sindy_models([m], dev.training_set, backend="numpy")
        ctol = max(ctol, 100.0 * rel_err(m.coefficients, ref.coefficients), 1e-13)
    tol = 10 * ctol * horizon
    diff = np.abs(a - b) / np.abs(a)
    print("evaluator: scores %s; max relative score difference %.2e (tolerance %.2e)"
          % (np.array2string(b, precision=4), diff.max(), tol))
    assert np.all(np.isfinite(a)) and diff.max() <= tol
    assert a[2] == b[2]                                         # the ARX model is fitted and scored as before
