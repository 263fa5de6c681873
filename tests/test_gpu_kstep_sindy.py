"""k-step accuracy of SINDy models on the MI355X (ampc_kstep_errors_sindy, csrc/kstep_sindy_kernels.hpp) through
``model_errors(..., sindy_kstep="device")``: the reference's get_model_rmse / get_model_rmsmens of its own SINDy
(tests/golden/kstep_sindy_*.npz), the host loop over the same handle's pred_batch, mixed batches against single
calls, f32, a diverging model, the evaluator, and the refusals.  Needs MI355X.

Tolerances.  1e-9 relative against the reference and against the host loop, the bound test_gpu_model_metrics.py and
test_gpu_kstep_linear.py hold this quantity to: the numpy composition reproduces the reference to 9e-16
(gen_golden_kstep_sindy.py prints it) and a 4-ulp perturbation of every feature at every step moves the RMSE by
2.2e-15 at most, so all of it is rounding allowance.  Bitwise claims are exact.
"""
import ctypes

import numpy as np
import pytest

from autompc_amd import MLP, MLPFactory, SINDy, SINDyFactory
from autompc_amd import _lib
from autompc_amd.evaluation import HoldoutModelEvaluator, model_errors
from autompc_amd.evaluation import model_metrics as MM
from autompc_amd.tuning.configs import DictConfiguration
from helpers import golden_params
from kstep_sindy_cases import CASES, sindy_model, system

pytestmark = pytest.mark.gpu


def _score(models, trajs, hs, metric="rmse"):
    rep = MM.KstepReport()
    out = model_errors(models, trajs, hs, metric, sindy_kstep="device", report=rep)
    assert rep.host_fallbacks == 0 and rep.sindy_models == len(models) and rep.sindy_calls == 1, rep
    return out


@pytest.mark.parametrize("tag", sorted(CASES))
def test_goldens_against_the_reference_and_the_host_loop(tag):
    m, trajs, g = sindy_model(tag)
    hs = [int(h) for h in g["horizons"]]
    for metric in ("rmse", "rmsmens"):
        dev = _score([m], trajs, hs, metric)[0]
        host = model_errors([m], trajs, hs, metric)[0]                          # the default: the host loop
        assert MM.last_report.host_fallbacks == 1 and MM.last_report.sindy_models == 0
        print("kstep sindy %s %s: largest relative deviation from the reference %.2e (host loop %.2e), device vs "
              "host loop %.2e" % (tag, metric, np.max(np.abs(dev / g[metric] - 1)),
                                  np.max(np.abs(host / g[metric] - 1)), np.max(np.abs(dev / host - 1))))
        np.testing.assert_allclose(dev, g[metric], rtol=1e-9, atol=0)
        np.testing.assert_allclose(dev, host, rtol=1e-9, atol=0)


def _mixed_batch():
    """The 3 / 2 cases on ONE data set (cross3's): discrete + continuous, product table + direct evaluation."""
    a, trajs, _ = sindy_model("cross3")
    b, c = sindy_model("poly3_trig2_cont")[0], sindy_model("cross5")[0]
    d = SINDy(a.system, poly_basis=True, poly_degree=3, poly_cross_terms=True, time_mode="continuous")
    d.set_coefficients(a.coefficients - 1.9 * np.eye(3, a.coefficients.shape[1]))   # cross3's terms, continuous
    models = [a, b, c, d]
    assert [MM.sindy_program_sizes(m)[5] > 0 for m in models] == [True, True, False, True]
    assert [m.time_mode for m in models] == ["discrete", "continuous", "discrete", "continuous"]
    return models, trajs


@pytest.mark.parametrize("delta", [False, True])
def test_mixed_batch_equals_single_calls_in_any_order_and_repeats(delta):
    models, trajs = _mixed_batch()
    kmax = 20
    pick = (lambda r: r[1]) if delta else (lambda r: r[0])
    S1 = pick(MM.kstep_sums_sindy(models, trajs, kmax, delta=delta))
    S2 = pick(MM.kstep_sums_sindy(models, trajs, kmax, delta=delta))
    assert np.array_equal(S1, S2) and np.all(np.isfinite(S1))                  # run to run
    perm = [2, 0, 3, 1]
    Sp = pick(MM.kstep_sums_sindy([models[i] for i in perm], trajs, kmax, delta=delta))
    for pos, i in enumerate(perm):
        assert np.array_equal(Sp[pos], S1[i])                                   # any order
    for i, m in enumerate(models):
        S = pick(MM.kstep_sums_sindy([m], trajs, kmax, delta=delta))
        assert np.array_equal(S[0], S1[i]), i                                   # one call of four = four calls
    assert len({S1[i, 3] for i in range(4)}) == 4
    if not delta:
        out = _score(models, trajs, [1, 4, 20])
        N = MM.row_counts(trajs, kmax)
        np.testing.assert_array_equal(out, np.sqrt(S1 / N)[:, [0, 3, 19]])


def test_f32_handles_agree_with_f64():
    """test_gpu_model_metrics.py's reasoning: an f32 model carries about 1e-7 relative error per step in its state
    (f32 coefficients, features and state), growing roughly linearly over 20 steps of a map whose Jacobian is near
    0.9 I, and the RMSE compares states with a spread of ~1: 1e-4 relative bounds it with margin while any indexing
    or precision-mixing slip gives O(1) differences."""
    hs = list(range(1, 11)) + [20]
    for tag in ("c1_trig", "hc_trig", "cross5"):
        m64, trajs, _ = sindy_model(tag)
        m32, _, _ = sindy_model(tag, precision="f32")
        a, b = _score([m64], trajs, hs)[0], _score([m32], trajs, hs)[0]
        print("kstep sindy %s f32 vs f64: max rel %.2e" % (tag, np.max(np.abs(b / a - 1))))
        np.testing.assert_allclose(b, a, rtol=1e-4)
        assert not np.array_equal(a, b)
        host32 = model_errors([m32], trajs, hs, "rmse")[0]
        np.testing.assert_allclose(b, host32, rtol=1e-9, atol=0)                # the f32 host loop takes the same steps


def test_diverging_model_overflows_alone():
    """x' = 1.5 x + x^3 from |x| ~ 0.5 squares its exponent every step once past 1: f64 overflows after about nine
    steps.  Until then the rollout amplifies a rounding difference by 3 per step at most (3^9 * 1e-16 << 1e-9)."""
    good, trajs, _ = sindy_model("cross3")
    bad = SINDy(good.system, poly_basis=True, poly_degree=3)
    xi = np.zeros_like(bad.coefficients)                           # features: 5 identities, 5 squares, 5 cubes
    assert xi.shape == (3, 15)
    xi[:, :3] = 1.5 * np.eye(3)
    xi[:, 10:13] = np.eye(3)
    bad.set_coefficients(xi)
    hs = list(range(1, 21))
    for metric in ("rmse", "rmsmens"):
        with np.errstate(all="ignore"):
            host = model_errors([bad], trajs, hs, metric)[0]
            dev = _score([good, bad], trajs, hs, metric)
        fin = np.isfinite(host)
        print("kstep sindy diverging %s: host finite to horizon %d, device to %d"
              % (metric, int(np.sum(fin)), int(np.sum(np.isfinite(dev[1])))))
        assert fin[:3].all() and not fin[-1] and not np.any(fin[np.argmin(fin):])
        np.testing.assert_allclose(dev[1][fin], host[fin], rtol=1e-9, atol=0)
        assert not np.any(np.isfinite(dev[1][~fin]))
        assert np.array_equal(dev[0], _score([good], trajs, hs, metric)[0]) and np.all(np.isfinite(dev[0]))


class _MixedFactory:
    """SINDy configurations and, for ``family == "mlp"``, an MLP: one ``evaluate_batch`` with both families."""
    name = "mixed"

    def __init__(self, s):
        self.sindy, self.mlp = SINDyFactory(s), MLPFactory(s, n_train_iters=2, n_batch=64)

    def __call__(self, cfg, train_trajs, silent=False, skip_train_model=False):
        d = dict(cfg.get_dictionary())
        family = d.pop("family")
        return (self.mlp if family == "mlp" else self.sindy)(DictConfiguration(d), train_trajs, silent=silent,
                                                              skip_train_model=skip_train_model)


def test_holdout_evaluator_routes_sindy_to_one_call_and_agrees_with_the_host_loop():
    _, trajs, _ = sindy_model("c1_trig")
    trajs = [t for t in trajs if len(t) >= 19]                     # six trajectories, two held out
    s = trajs[0].system
    trig = dict(family="sindy", trig_basis="true", trig_freq=1, trig_interaction="true", time_mode="discrete")
    poly = dict(family="sindy", poly_basis="true", poly_degree=3, time_mode="discrete")
    cfgs = [DictConfiguration(dict(trig, threshold=1e-2)), DictConfiguration(dict(poly, threshold=1e-2)),
            DictConfiguration(family="mlp", n_hidden_layers="1", hidden_size_1=16, nonlintype="tanh", lr=1e-3),
            DictConfiguration(dict(trig, threshold=1e-1)), DictConfiguration(dict(poly, threshold=1e-3))]
    kw = dict(horizon=5, holdout_prop=0.34)
    host = HoldoutModelEvaluator(s, trajs, "rmse", np.random.default_rng(3), **kw)
    dev = HoldoutModelEvaluator(s, trajs, "rmse", np.random.default_rng(3), sindy_kstep="device", **kw)
    assert len(dev.holdout) == 2
    a = np.asarray(host.evaluate_batch(_MixedFactory(s), cfgs))
    b = np.asarray(dev.evaluate_batch(_MixedFactory(s), cfgs))
    rep = dev.last_kstep
    print("evaluator: scores %s; max relative score difference %.2e; %r; host evaluator %r"
          % (np.array2string(b, precision=4), np.max(np.abs(b / a - 1)), rep, host.last_kstep))
    assert rep.sindy_calls == 1 and rep.host_fallbacks == 0 and rep.sindy_models == 4 and rep.device_models == 1
    assert host.last_kstep.host_fallbacks == 4 and host.last_kstep.sindy_calls == 0
    assert np.all(np.isfinite(a))
    np.testing.assert_allclose(b, a, rtol=1e-9, atol=0)


def test_refusals():
    a, trajs, _ = sindy_model("c1_trig")
    s = a.system
    p = golden_params(4, 1, [16], "relu", 5)
    mlp = MLP(s, n_hidden_layers=1, nonlintype="relu", hidden_size_1=16)
    mlp.jit_kernels = False
    mlp.weights, mlp.biases = [w.copy() for w in p["weights"]], [b.copy() for b in p["biases"]]
    mlp.xu_means, mlp.xu_std, mlp.dy_means, mlp.dy_std = p["xu_means"], p["xu_std"], p["dy_means"], p["dy_std"]
    for batch in ([mlp], [a, mlp]):
        with pytest.raises(_lib.AmpcError, match="SINDy models only"):
            MM.kstep_sums_sindy(batch, trajs, 3)
    with pytest.raises(_lib.AmpcError, match="share ctrl_dim"):
        MM.kstep_sums_sindy([a, SINDy(system(4, 2))], trajs, 3)
    with pytest.raises(_lib.AmpcError, match="share the state dim"):
        MM.kstep_sums_sindy([a, SINDy(system(3, 1))], trajs, 3)
    with pytest.raises(_lib.AmpcError, match="one device and one precision"):
        MM.kstep_sums_sindy([a, sindy_model("c1_trig", precision="f32")[0]], trajs, 3)
    with pytest.raises(_lib.AmpcError, match="obs_dim must be the models' state dim"):
        MM.kstep_sums_sindy([a], sindy_model("cross3")[1], 3)                   # data of a 3 / 2 system
    # the old entry keeps refusing SINDy models, in its own words
    hp = (ctypes.c_void_p * 1)(a._dev()._h.value)
    lens, obs, ctrls = MM._concat(trajs)
    S = np.empty((1, 3))
    with pytest.raises(_lib.AmpcError, match="MLP models and linear models of at most 64 states only"):
        _lib.check(a._dev().lib.ampc_kstep_errors(hp, 1, len(trajs), _lib.iptr(lens), 4, _lib.dptr(obs),
                                                  _lib.dptr(ctrls), None, 3, None, _lib.dptr(S), None))
    # and after the refusals the entry still scores
    assert np.all(np.isfinite(MM.kstep_sums_sindy([a], trajs, 3)[0]))
