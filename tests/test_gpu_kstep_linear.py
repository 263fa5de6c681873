"""k-step accuracy of wide linear models on the MI355X (ampc_kstep_errors_linear, csrc/kstep_linear_kernels.hpp)
through ``model_errors(..., linear_kstep="device")``: the reference's get_model_rmse / get_model_rmsmens of ARX and
Koopman models it trained (tests/golden/kstep_wide_*.npz), mixed batches against single calls, the device sums
against the host composition over the same handle's pred_batch, f32, the evaluator, and the refusals.  Needs MI355X.

Tolerances.  1e-9 relative against the reference and against the host composition, the bound
test_gpu_model_metrics.py holds this quantity to: the host algorithm reproduces the reference to 2.2e-16
(gen_golden_kstep_wide.py prints it), so all of it is rounding allowance.  Bitwise claims are exact.
"""
import numpy as np
import pytest

from autompc_amd import ARX, ARXFactory, Koopman, MLP
from autompc_amd import _lib
from autompc_amd.evaluation import HoldoutModelEvaluator, model_errors
from autompc_amd.evaluation import model_metrics as MM
from autompc_amd.tuning.configs import DictConfiguration
from conftest import golden
from helpers import golden_params
from kstep_wide_cases import WIDE, RowsARX, ragged_trajs, system, trajs_of, wide_model

pytestmark = pytest.mark.gpu


def _score(models, trajs, hs, metric="rmse"):
    rep = MM.KstepReport()
    out = model_errors(models, trajs, hs, metric, linear_kstep="device", report=rep)
    assert rep.host_fallbacks == 0 and rep.wide_models == len(models) and rep.wide_calls == 1, rep
    return out


@pytest.mark.parametrize("tag", sorted(WIDE))
def test_wide_goldens_against_the_reference(tag):
    m, trajs, g = wide_model(tag)
    hs = [int(h) for h in g["horizons"]]
    out = _score([m], trajs, hs)[0]
    print("kstep wide %s (%d states): largest relative deviation from the reference's RMSE %.2e"
          % (tag, m.A.shape[0], np.max(np.abs(out / g["rmse"] - 1))))
    np.testing.assert_allclose(out, g["rmse"], rtol=1e-9, atol=0)
    if "rmsmens" in g.files:
        outm = _score([m], trajs, hs, "rmsmens")[0]
        print("kstep wide %s: largest relative deviation from the reference's RMSMENS %.2e"
              % (tag, np.max(np.abs(outm / g["rmsmens"] - 1))))
        np.testing.assert_allclose(outm, g["rmsmens"], rtol=1e-9, atol=0)
    else:
        with pytest.raises(ValueError):
            model_errors([m], trajs, [1], "rmsmens", linear_kstep="device")     # the state is not the observation


def test_existing_wide_arx_golden_through_the_new_path():
    g = golden("kstep_lin_arx4_wide")
    s = system(int(g["nx"]), int(g["nu"]))
    m = ARX(s, history=4)
    m.A, m.B = g["A"].copy(), g["B"].copy()
    trajs = trajs_of(s, g)
    hs = [int(h) for h in g["horizons"]]
    out = _score([m], trajs, hs)[0]
    print("kstep_lin_arx4_wide on the device: largest relative deviation from the reference %.2e"
          % np.max(np.abs(out / g["rmse"] - 1)))
    np.testing.assert_allclose(out, g["rmse"], rtol=1e-9, atol=0)
    host = model_errors([m], trajs, hs, "rmse")[0]                              # the default: the host loop
    assert MM.last_report.host_fallbacks == 1 and MM.last_report.wide_models == 0
    np.testing.assert_allclose(out, host, rtol=1e-9, atol=0)


def _mixed_batch():
    """ARX 4 / 7 / 10, two Koopman lifts and a rule-0 model on ONE data set (arx4_hc's, 17 / 6)."""
    a4, trajs, _ = wide_model("arx4_hc")
    a7, a10, kp = wide_model("arx7_hc")[0], wide_model("arx10_hc")[0], wide_model("koop_polytrig")[0]
    s = a4.system
    kt = Koopman(s, method="lstsq", trig_basis=True, poly_degree=2)            # id + 2 x (sin 2x, cos 2x): 85 states
    kt.train(ragged_trajs(s, [80] * 12, 31))
    rows = wide_model("arx7_hc", make=lambda sy, p: RowsARX(sy, history=7, precision=p))[0]
    models = [a4, a7, a10, kp, kt, rows]
    assert [MM.linear_state_rule(m)["rule"] for m in models] == [1, 1, 1, 2, 2, 0]
    assert [m.A.shape[0] for m in models] == [87, 156, 225, 102, 85, 156]
    return models, trajs


def test_mixed_batch_equals_single_calls_in_any_order_and_repeats():
    models, trajs = _mixed_batch()
    kmax = 20
    S1, _ = MM.kstep_sums_linear(models, trajs, kmax)
    S2, _ = MM.kstep_sums_linear(models, trajs, kmax)
    assert np.array_equal(S1, S2) and np.all(np.isfinite(S1))                  # run to run
    perm = [4, 2, 0, 5, 3, 1]
    Sp, _ = MM.kstep_sums_linear([models[i] for i in perm], trajs, kmax)
    for pos, i in enumerate(perm):
        assert np.array_equal(Sp[pos], S1[i])                                   # any order
    for i, m in enumerate(models):
        S, _ = MM.kstep_sums_linear([m], trajs, kmax)
        assert np.array_equal(S[0], S1[i]), i                                   # one call of six = six calls
    assert np.array_equal(S1[1], S1[5])                # the gather on the device = the uploaded traj_to_states rows
    assert len({S1[i, 3] for i in range(5)}) == 5
    out = _score(models, trajs, [1, 4, 20])
    N = MM.row_counts(trajs, kmax)
    np.testing.assert_array_equal(out, np.sqrt(S1 / N)[:, [0, 3, 19]])


def _host_sums(model, trajs, kmax, delta):
    """The reference's loop over model.pred_batch, as sums per horizon (S_h, D_h of the module docstring)."""
    no = trajs[0].system.obs_dim
    std = MM._increment_stats(trajs)[1]
    S, D = np.zeros(kmax), np.zeros(kmax)
    for h in range(1, kmax + 1):
        for t in trajs:
            if len(t) <= h:
                continue
            state = model.traj_to_states(t[:-h]) if hasattr(model, "traj_to_states") else t.obs[:-h, :]
            for k in range(h):
                prev = state
                state = model.pred_batch(state, t.ctrls[k:-(h - k), :])
            S[h - 1] += np.sum((state[:, :no] - t.obs[h:]) ** 2)
            if delta:
                D[h - 1] += np.sum((((state - prev) - (t.obs[h:] - t.obs[h - 1:-1])) / std) ** 2)
    return S, D


@pytest.mark.parametrize("tag", ["arx4_hc", "arx10_hc", "koop_polytrig", "koop_id70"])
def test_device_sums_equal_host_composition_over_pred_batch(tag):
    m, trajs, g = wide_model(tag)
    delta = tag == "koop_id70"
    kmax = 20
    S, D = MM.kstep_sums_linear([m], trajs, kmax, delta=delta)
    Sh, Dh = _host_sums(m, trajs, kmax, delta)
    print("kstep wide %s vs pred_batch: S bitwise equal %s (max rel %.1e)"
          % (tag, np.array_equal(S[0], Sh), np.max(np.abs(S[0] / Sh - 1))))
    np.testing.assert_allclose(S[0], Sh, rtol=1e-9, atol=0)
    if delta:
        print("kstep wide %s vs pred_batch: D bitwise equal %s (max rel %.1e)"
              % (tag, np.array_equal(D[0], Dh), np.max(np.abs(D[0] / Dh - 1))))
        np.testing.assert_allclose(D[0], Dh, rtol=1e-9, atol=0)


def test_f32_handles_agree_with_f64():
    """test_gpu_model_metrics.py's reasoning: an f32 model carries about 1e-7 relative error per step in its state
    (f32 weights and state, exact f32 MFMA), growing roughly linearly over 20 steps, and the RMSE compares states
    with a spread of ~1: 1e-4 relative bounds it with margin while any indexing or precision-mixing slip gives
    O(1) differences."""
    hs = list(range(1, 11)) + [20]
    for tag in ("arx4_hc", "koop_polytrig"):
        m64, trajs, _ = wide_model(tag)
        m32, _, _ = wide_model(tag, precision="f32")
        a, b = _score([m64], trajs, hs)[0], _score([m32], trajs, hs)[0]
        print("kstep wide %s f32 vs f64: max rel %.2e" % (tag, np.max(np.abs(b / a - 1))))
        np.testing.assert_allclose(b, a, rtol=1e-4)
        assert not np.array_equal(a, b)


def test_holdout_evaluator_device_scores_equal_host_scores():
    s = system(17, 6)
    trajs = ragged_trajs(s, [60] * 12, 11)
    cfgs = [DictConfiguration(history=k) for k in range(1, 11)]
    kw = dict(horizon=5, holdout_prop=0.25, linear_fit="device")
    host = HoldoutModelEvaluator(s, trajs, "rmse", np.random.default_rng(3), **kw)
    dev = HoldoutModelEvaluator(s, trajs, "rmse", np.random.default_rng(3), linear_kstep="device", **kw)
    a = np.asarray(host.evaluate_batch(ARXFactory(s), cfgs))
    b = np.asarray(dev.evaluate_batch(ARXFactory(s), cfgs))
    rep = dev.last_kstep
    print("evaluator: max relative score difference %.2e; %r; host evaluator %r"
          % (np.max(np.abs(b / a - 1)), rep, host.last_kstep))
    assert rep.host_fallbacks == 0 and rep.wide_models == 7 and rep.wide_calls == 1 and rep.device_models == 3
    assert host.last_kstep.host_fallbacks == 7 and host.last_kstep.wide_models == 0
    assert np.all(np.isfinite(a))
    np.testing.assert_allclose(b, a, rtol=1e-9, atol=0)
    one = HoldoutModelEvaluator(s, trajs, "rmse", np.random.default_rng(3), linear_kstep="device", horizon=5,
                                holdout_prop=0.25)
    assert one(ARXFactory(s), cfgs[3]) == pytest.approx(MM.host_rmse(ARXFactory(s)(cfgs[3], one.training_set),
                                                                       one.holdout, 5), rel=1e-9)


def test_refusals(monkeypatch):
    a4, trajs, _ = wide_model("arx4_hc")
    s = a4.system
    narrow = ARX(s, history=2)
    narrow.A, narrow.B = 0.5 * np.eye(41), np.zeros((41, 6))
    with pytest.raises(_lib.AmpcError, match="wide linear models only"):
        MM.kstep_sums_linear([a4, narrow], trajs, 3)
    p = golden_params(17, 6, [16], "relu", 5)
    mlp = MLP(s, n_hidden_layers=1, nonlintype="relu", hidden_size_1=16)
    mlp.jit_kernels = False
    mlp.weights, mlp.biases = [w.copy() for w in p["weights"]], [b.copy() for b in p["biases"]]
    mlp.xu_means, mlp.xu_std, mlp.dy_means, mlp.dy_std = p["xu_means"], p["xu_std"], p["dy_means"], p["dy_std"]
    with pytest.raises(_lib.AmpcError, match="wide linear models only"):
        MM.kstep_sums_linear([mlp], trajs, 3)
    other = ARX(system(17, 2), history=5)                        # 94 states, two controls
    other.A, other.B = 0.5 * np.eye(94), np.zeros((94, 2))
    with pytest.raises(_lib.AmpcError, match="share ctrl_dim"):
        MM.kstep_sums_linear([a4, other], trajs, 3)
    with pytest.raises(_lib.AmpcError, match="one device and one precision"):
        MM.kstep_sums_linear([a4, wide_model("arx7_hc", precision="f32")[0]], trajs, 3)
    monkeypatch.setattr(MM, "linear_state_rule", lambda m, no=None: {"rule": 1, "history": 5})
    with pytest.raises(_lib.AmpcError, match="does not have the handle's state dim"):
        MM.kstep_sums_linear([a4], trajs, 3)
    monkeypatch.setattr(MM, "linear_state_rule", lambda m, no=None: {
        "rule": 2, "kinds": np.array([0, 2], dtype=np.int32), "params": np.array([1.0, 1.0])})
    with pytest.raises(_lib.AmpcError, match="does not have the handle's state dim"):
        MM.kstep_sums_linear([a4], trajs, 3)
    monkeypatch.undo()
    # the old entry keeps refusing wide linear models, in its own words
    import ctypes
    hp = (ctypes.c_void_p * 1)(a4._dev()._h.value)
    lens, obs, ctrls = MM._concat(trajs)
    S = np.empty((1, 3))
    with pytest.raises(_lib.AmpcError, match="MLP models and linear models of at most 64 states only"):
        _lib.check(a4._dev().lib.ampc_kstep_errors(hp, 1, len(trajs), _lib.iptr(lens), 17, _lib.dptr(obs),
                                                   _lib.dptr(ctrls), None, 3, None, _lib.dptr(S), None))
