"""k-step accuracy of MLP models of any mix of shapes in one launch (ampc_kstep_errors_mlp,
csrc/kstep_mlp_kernels.hpp) through ``model_errors(..., mlp_kstep="batch")``: the reference's get_model_rmse /
get_model_rmsmens of seeded MLPs (tests/golden/kstep_mlp_*.npz), the host loop over pred_batch, the per-shape device
path, mixed batches against single calls, a diverging model, the data edges, parameters straight from the device fit,
the evaluator, and the refusals.  Needs MI355X.

The fixtures' shapes: width 16 (one column tile), 37 (ragged tile and ragged reduction), 200, 256 (the maximum), depths
1 and 4, the four activations, nx + nu = 5 (one mostly empty reduction block) and 66 (over 64), nx = 64 (four output
tiles), 129 start points (no multiple of the 16-row tile), trajectories of 7 and 12 rows under horizon 20.

Tolerances.  1e-9 relative against the reference, the host loop and the per-shape path: the bound
test_gpu_model_metrics.py and test_gpu_kstep_sindy.py hold this quantity to.  A plain f64 evaluation with a reordered,
16-blocked sum deviates from these goldens by at most 4.4e-16, so all of it is rounding allowance.  Bitwise claims are
exact.

The shape sweep (tests 8 to 10) is held tighter, against kstep_mlp_cases.kstep_sums_ref in long double: the raw sums S and
D to max(1e-13, 100 x cond) relative, cond the deviation of the reference's own f64 run from its long-double run on
that case (at most 3.0e-16 on the sweep, so the floor decides).  test_kstep_mlp_host.py holds the reference to the
goldens (1.8e-16) and every case's cond to 1e-14.  Measured on the MI355X: DESIGN 6k.
"""
import numpy as np
import pytest
import torch  # noqa: F401  (before the library, as in test_gpu_mlp_fit_device.py: the device fit runs on torch's GPU)

from autompc_amd import MLP, MLPFactory, _lib
from autompc_amd.evaluation import HoldoutModelEvaluator, model_errors
from autompc_amd.evaluation import model_metrics as MM
from autompc_amd.tuning.configs import DictConfiguration
from helpers import golden_params, make_system
import kstep_mlp_cases as K
from kstep_mlp_cases import TAGS, fixture_model, mlp_of, synthetic_trajs

pytestmark = pytest.mark.gpu


def _score(models, trajs, hs, metric="rmse"):
    rep = MM.KstepReport()
    out = model_errors(models, trajs, hs, metric, mlp_kstep="batch", report=rep)
    assert rep.mlp_batch_calls == 1 and rep.mlp_batch_models == len(models), rep
    assert rep.device_models == 0 and rep.host_fallbacks == 0, rep
    return out


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) / np.asarray(b) - 1)))


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_every_fixture_alone_against_the_reference_the_host_loop_and_the_shape_path(tag):
    m, trajs, g = fixture_model(tag)
    hs = [int(h) for h in g["horizons"]]
    for metric, host_fn in (("rmse", MM.host_rmse), ("rmsmens", MM.host_rmsmens)):
        dev = _score([m], trajs, hs, metric)[0]
        assert m._handle is None                                            # scored without a staged handle
        shape = model_errors([m], trajs, hs, metric)[0]                     # the default path
        assert MM.last_report.device_models == 1 and MM.last_report.mlp_batch_calls == 0
        host = np.array([host_fn(m, trajs, h) for h in hs])
        m._invalidate()
        print("kstep mlp batch %s %s: largest relative deviation from the reference %.2e, from the host loop %.2e, "
              "from the per-shape path %.2e" % (tag, metric, _rel(dev, g[metric]), _rel(dev, host), _rel(dev, shape)))
        np.testing.assert_allclose(dev, g[metric], rtol=1e-9, atol=0)
        np.testing.assert_allclose(dev, host, rtol=1e-9, atol=0)
        np.testing.assert_allclose(dev, shape, rtol=1e-9, atol=0)


# 2 ---------------------------------------------------------------------------------------------------------------
def _hc_batch():
    a, trajs, _ = fixture_model("hc_relu2")
    models = [fixture_model("hc_selu4")[0], a, fixture_model("hc_tanh1")[0]]
    models += [fixture_model("hc_relu2", seed=100 + k)[0] for k in range(3)]
    return models, trajs, [4, 1, 5, 0, 3, 2]


def _c4_batch():
    a, trajs, _ = fixture_model("c4_relu1")
    return [a, fixture_model("c4_tanh2")[0], fixture_model("c4_sigmoid3")[0]], trajs, [2, 0, 1]


@pytest.mark.parametrize("batch", [_hc_batch, _c4_batch])
def test_mixed_batch_is_one_call_and_equals_single_calls_in_any_order_and_repeats(batch):
    models, trajs, perm = batch()
    kmax = 20
    assert len({MM.device_shape_key(m) for m in models}) >= 3
    S1, D1 = MM.kstep_sums_mlp(models, trajs, kmax, delta=True)
    S2, D2 = MM.kstep_sums_mlp(models, trajs, kmax, delta=True)
    assert np.array_equal(S1, S2) and np.array_equal(D1, D2)                # run to run
    assert np.all(np.isfinite(S1)) and np.all(np.isfinite(D1)) and np.all(S1 > 0) and np.all(D1 > 0)
    Sp, Dp = MM.kstep_sums_mlp([models[i] for i in perm], trajs, kmax, delta=True)
    for pos, i in enumerate(perm):
        assert np.array_equal(Sp[pos], S1[i]) and np.array_equal(Dp[pos], D1[i])     # any order
    for i, m in enumerate(models):
        S, D = MM.kstep_sums_mlp([m], trajs, kmax, delta=True)
        assert np.array_equal(S[0], S1[i]) and np.array_equal(D[0], D1[i]), i        # one call of n = n calls
    assert len({S1[i, 3] for i in range(len(models))}) == len(models)
    S0, none = MM.kstep_sums_mlp(models, trajs, kmax)                       # without the delta sums: the same S
    assert none is None and np.array_equal(S0, S1)
    out = _score(models, trajs, [1, 4, 20])                                 # one call, no per-shape launch
    N = MM.row_counts(trajs, kmax)
    np.testing.assert_array_equal(out, np.sqrt(S1 / N)[:, [0, 3, 19]])
    assert all(m._handle is None for m in models)
    out_m = _score(models, trajs, [1, 4, 20], "rmsmens")
    np.testing.assert_array_equal(out_m, np.sqrt(D1 / (N * trajs[0].system.obs_dim))[:, [0, 3, 19]])


# 3 ---------------------------------------------------------------------------------------------------------------
def test_diverging_model_overflows_alone():
    """Output-layer weights scaled by 1e30 on a relu net: the state grows by about that factor per step, its square
    leaves f64 after about five steps and the state itself after about ten.  Until then the map is positively
    homogeneous in the (huge) state, so a rounding difference stays a relative one."""
    a, trajs, _ = fixture_model("hc_relu2")
    b = fixture_model("hc_relu2", seed=101)[0]
    bad = fixture_model("hc_relu2", seed=102)[0]
    bad.weights = bad.weights[:-1] + [bad.weights[-1] * 1e30]
    hs = list(range(1, 21))
    for metric in ("rmse", "rmsmens"):
        with np.errstate(all="ignore"):
            host = model_errors([bad], trajs, hs, metric)[0]                # (the per-shape device path)
            host_loop = np.array([(MM.host_rmse if metric == "rmse" else MM.host_rmsmens)(bad, trajs, h) for h in hs])
            dev = _score([a, bad, b], trajs, hs, metric)
        fin = np.isfinite(host_loop)
        print("kstep mlp batch diverging %s: host loop finite to horizon %d, per-shape path to %d, batch to %d; "
              "finite horizons vs host loop %.2e" % (metric, int(np.sum(fin)), int(np.sum(np.isfinite(host))),
                                                     int(np.sum(np.isfinite(dev[1]))), _rel(dev[1][fin], host_loop[fin])))
        assert fin[:3].all() and not fin[-1] and not np.any(fin[np.argmin(fin):])
        np.testing.assert_allclose(dev[1][fin], host_loop[fin], rtol=1e-9, atol=0)
        assert not np.any(np.isfinite(dev[1][~fin]))
        assert np.array_equal(dev[0], _score([a], trajs, hs, metric)[0]) and np.all(np.isfinite(dev[0]))
        assert np.array_equal(dev[2], _score([b], trajs, hs, metric)[0]) and np.all(np.isfinite(dev[2]))
        bad._invalidate()


# 4 ---------------------------------------------------------------------------------------------------------------
METRICS = ("rmse", "rmsmens")


def _host(m, trajs, hs, metric):
    fn = MM.host_rmse if metric == "rmse" else MM.host_rmsmens
    return np.array([fn(m, trajs, h) for h in hs])


@pytest.mark.parametrize("tag", ["c4_tanh2", "hc_selu4"])
def test_data_edges_against_the_host_loop(tag):
    m, trajs, _ = fixture_model(tag)
    one_row = trajs[0][:1]
    assert len(one_row) == 1
    # (RMSMENS divides by the spread of the data's increments, which is zero when the data holds ONE increment: the
    #  metric is undefined there -- 0 / 0 or x / 0 on either path -- so a single start point is scored by RMSE, and
    #  by RMSMENS next to a second trajectory that contributes start points to horizon 1 only)
    cases = {"a one-row trajectory in the list": ([trajs[1], one_row, trajs[3], one_row], [1, 2, 6, 11], METRICS),
             "kmax = 1": (trajs, [1], METRICS),
             "a single start point": ([trajs[2][3:5]], [1], ("rmse",)),
             "a single start point under kmax = 3": ([one_row, trajs[2][3:5]], [1, 3], ("rmse",)),
             "a single start point at horizon 3": ([one_row, trajs[2][3:5], trajs[2][8:12]], [1, 3], METRICS)}
    for what, (tr, hs, metrics) in cases.items():
        for metric in metrics:
            with np.errstate(all="ignore"):
                dev = _score([m], tr, hs, metric)[0]
                host = _host(m, tr, hs, metric)
            both = np.isfinite(host)
            print("kstep mlp batch %s, %s, %s: %s vs host loop %s" % (tag, what, metric, dev, host))
            assert np.array_equal(np.isnan(dev), np.isnan(host)) and both[0]
            np.testing.assert_allclose(dev[both], host[both], rtol=1e-9, atol=0)
    with np.errstate(all="ignore"):                                          # the undefined case stays non-finite
        assert not np.isfinite(_score([m], [trajs[2][3:5]], [1], "rmsmens")[0, 0])
    # horizons larger than every trajectory: nan, as the default path gives
    dev = _score([m], trajs, [40, 41], "rmse")[0]
    assert np.all(np.isnan(dev)) and np.all(np.isnan(model_errors([m], trajs, [40, 41], "rmse")[0]))
    mixed = _score([m], trajs, [39, 40], "rmse")[0]                         # 40 rows: one start point at horizon 39
    assert np.isfinite(mixed[0]) and np.isnan(mixed[1])
    np.testing.assert_allclose(mixed[0], MM.host_rmse(m, trajs, 39), rtol=1e-9, atol=0)


# 5 ---------------------------------------------------------------------------------------------------------------
def test_straight_from_the_device_fit_without_a_handle():
    from autompc_amd.sysid.mlp_fit import fit_mlps
    s = make_system(3, 2)
    trajs = synthetic_trajs(s, seed=5)
    models = [MLP(s, n_hidden_layers=1, hidden_size_1=20, nonlintype="tanh", n_train_iters=3, n_batch=32, lr=1e-3, seed=1),
              MLP(s, n_hidden_layers=3, hidden_size_1=17, hidden_size_2=33, hidden_size_3=16, nonlintype="selu",
                  n_train_iters=3, n_batch=32, lr=3e-4, seed=2),
              MLP(s, n_hidden_layers=2, hidden_size_1=64, hidden_size_2=31, nonlintype="sigmoid", n_train_iters=3,
                  n_batch=32, lr=1e-3, seed=3)]
    for m in models:
        m.jit_kernels = False
    rep = fit_mlps(models, trajs, fit="device")
    assert rep["device_models"] == 3
    hs = [1, 2, 5, 16]
    args = MM.mlp_batch_args(models)
    assert args["on_device"].tolist() == [1, 1, 1]
    assert int(args["weights"][0, 0]) == models[0]._dev_params["w"][0].data_ptr()
    assert int(args["norms"][2, 3]) == models[2]._dev_params["norm_dev"][3].data_ptr()
    for metric in ("rmse", "rmsmens"):
        dev = _score(models, trajs, hs, metric)
        # nothing of the call was staged or fetched: no handle, no host copy of the parameters
        assert all(m._handle is None and m._weights is None for m in models)
        shape = model_errors(models, trajs, hs, metric)
        assert MM.last_report.device_models == 3 and all(m._handle is not None for m in models)
        for m in models:
            m._invalidate()
        print("kstep mlp batch from the fit, %s: vs the per-shape path %.2e" % (metric, _rel(dev, shape)))
        np.testing.assert_allclose(dev, shape, rtol=1e-9, atol=0)
        # the same models from host parameters: the same bits
        twins = []
        for m in models:
            t = MLP(s, n_hidden_layers=len(m.hidden_sizes), nonlintype=m.nonlintype,
                    **{"hidden_size_%d" % (i + 1): h for i, h in enumerate(m.hidden_sizes)})
            t.jit_kernels = False
            t.set_parameters(m.get_parameters())
            twins.append(t)
        assert not MM.mlp_batch_args(twins)["on_device"].any()
        assert np.array_equal(_score(twins, trajs, hs, metric), dev)
        assert np.array_equal(_score([twins[0], models[1], twins[2]], trajs, hs, metric), dev)     # mixed residence
        for m in models:
            m._weights = m._biases = None                                   # (get_parameters fetched them)
    # a model whose normalisers were changed after the fit no longer stands on the device copy
    models[0].dy_std = models[0].dy_std * 2.0
    assert MM.mlp_batch_args(models)["on_device"].tolist() == [0, 1, 1]
    np.testing.assert_allclose(_score(models, trajs, hs), model_errors(models, trajs, hs), rtol=1e-9, atol=0)


# 6 ---------------------------------------------------------------------------------------------------------------
def test_holdout_evaluator_routes_a_mixed_batch_to_one_call():
    s = make_system(3, 2)
    trajs = synthetic_trajs(s, lens=(40, 23, 31, 17, 28, 35, 22, 30), seed=6)
    cfgs = [DictConfiguration(n_hidden_layers="1", hidden_size_1=16, nonlintype="relu", lr=1e-3),
            DictConfiguration(n_hidden_layers="2", hidden_size_1=37, hidden_size_2=20, nonlintype="tanh", lr=1e-3),
            DictConfiguration(n_hidden_layers="3", hidden_size_1=24, hidden_size_2=16, hidden_size_3=40,
                              nonlintype="sigmoid", lr=3e-3),
            DictConfiguration(n_hidden_layers="4", hidden_size_1=16, hidden_size_2=17, hidden_size_3=18, hidden_size_4=19,
                              nonlintype="selu", lr=1e-4),
            DictConfiguration(n_hidden_layers="1", hidden_size_1=65, nonlintype="tanh", lr=1e-2),
            DictConfiguration(n_hidden_layers="2", hidden_size_1=37, hidden_size_2=20, nonlintype="tanh", lr=1e-4)]
    kw = dict(horizon=5, holdout_prop=0.25, mlp_fit="device")
    factory = MLPFactory(s, n_train_iters=2, n_batch=32)
    for metric in ("rmse", "rmsmens"):
        shape = HoldoutModelEvaluator(s, trajs, metric, np.random.default_rng(3), mlp_kstep="shape", **kw)
        batch = HoldoutModelEvaluator(s, trajs, metric, np.random.default_rng(3), mlp_kstep="batch", **kw)
        assert len(batch.holdout) == 2
        a = np.asarray(shape.evaluate_batch(factory, cfgs))
        b = np.asarray(batch.evaluate_batch(factory, cfgs))
        rep = batch.last_kstep
        print("evaluator %s: scores %s; max relative score difference %.2e; %r; per-shape evaluator %r"
              % (metric, np.array2string(b, precision=4), _rel(b, a), rep, shape.last_kstep))
        assert rep.mlp_batch_calls == 1 and rep.mlp_batch_models == 6 and rep.device_models == 0
        assert shape.last_kstep.device_models == 6 and shape.last_kstep.mlp_batch_calls == 0
        assert batch.last_mlp_fit["device_models"] == 6 and np.all(np.isfinite(a)) and len(set(b)) == 6
        np.testing.assert_allclose(b, a, rtol=1e-9, atol=0)


# 7 ---------------------------------------------------------------------------------------------------------------
def test_refusals():
    a, trajs, _ = fixture_model("c4_relu1")
    s = a.system
    # an f32 model is not refused: it keeps the per-shape path
    f32 = fixture_model("c4_relu1", precision="f32")[0]
    rep = MM.KstepReport()
    out = model_errors([a, f32], trajs, [1, 5], "rmse", mlp_kstep="batch", report=rep)
    assert rep.mlp_batch_models == 1 and rep.mlp_batch_calls == 1 and rep.device_models == 1
    np.testing.assert_allclose(out[1], out[0], rtol=1e-4)
    with pytest.raises(ValueError, match="f64"):
        MM.kstep_sums_mlp([f32], trajs, 3)
    # width 257: the per-shape path through model_errors, refused by the entry itself
    wide = mlp_of(s, golden_params(4, 1, [257], "relu", 7), [257], "relu")
    assert MM.mlp_batch_key(wide) is None
    with pytest.raises(_lib.AmpcError, match="hidden widths must be in 1..256"):
        MM.kstep_sums_mlp([a, wide], trajs, 3)
    # five hidden layers
    deep = MLP(s, n_hidden_layers=5, hidden_size=16)
    with pytest.raises(ValueError, match="1..4 hidden layers"):
        MM.kstep_sums_mlp([deep], trajs, 3)
    args = MM.mlp_batch_args([a])
    lens, obs, ctrls = MM._concat(trajs)
    S = np.empty((1, 3))
    lib = _lib.load()
    import ctypes
    vpp = lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_void_p))

    def call(n_hidden=args["n_hidden"], nx=4, nu=1, obs_dim=4, on_device=args["on_device"], kmax=3):
        return lib.ampc_kstep_errors_mlp(0, 1, _lib.iptr(n_hidden), _lib.iptr(args["dims"]), _lib.iptr(args["acts"]),
                                         vpp(args["weights"]), vpp(args["biases"]), vpp(args["norms"]),
                                         _lib.iptr(on_device), nx, nu, len(trajs), _lib.iptr(lens), obs_dim,
                                         _lib.dptr(obs), _lib.dptr(ctrls), kmax, None, _lib.dptr(S), None)
    with pytest.raises(_lib.AmpcError, match="1..4 hidden layers"):
        _lib.check(call(n_hidden=np.array([5], dtype=np.int32)))
    with pytest.raises(_lib.AmpcError, match="obs_dim must be the models' state dim"):
        _lib.check(call(obs_dim=3))
    with pytest.raises(_lib.AmpcError, match="kmax must be >= 1"):
        _lib.check(call(kmax=0))
    with pytest.raises(_lib.AmpcError, match="not device memory"):
        _lib.check(call(on_device=np.array([1], dtype=np.int32)))          # host arrays flagged as device memory
    # obs_dim != nx through the Python entry: data of another system
    with pytest.raises(_lib.AmpcError, match="obs_dim must be the models' state dim"):
        MM.kstep_sums_mlp([a], fixture_model("hc_relu2")[1], 3)
    # mismatched nx inside one call
    with pytest.raises(_lib.AmpcError, match="nx \\+ nu inputs and gives nx outputs"):
        MM.kstep_sums_mlp([a, mlp_of(make_system(3, 2), golden_params(3, 2, [16], "relu", 5), [16], "relu")], trajs, 3)
    with pytest.raises(ValueError, match="mlp_kstep"):
        model_errors([a], trajs, [1], "rmse", mlp_kstep="device")
    # and after the refusals the entry still scores
    _lib.check(call())
    assert np.all(np.isfinite(S)) and np.array_equal(S, MM.kstep_sums_mlp([a], trajs, 3)[0])


# 8 ---------------------------------------------------------------------------------------------------------------
def test_the_sweep_covers_what_it_claims():
    ins = {nx + nu for nx, nu, _, _ in K.SWEEP}
    hidden = {h for _, _, hs, _ in K.SWEEP for h in hs}
    assert {16, 32, 48, 64, 80} <= ins and {2, 17, 33, 79} <= ins            # 1..5 blocks without a ragged one, and ragged
    assert {1, 15, 16, 17, 32, 48, 63, 64} <= {nx for nx, *_ in K.SWEEP}
    assert {-(-nx // 16) for nx, *_ in K.SWEEP} == {1, 2, 3, 4}               # output tiles: waves without one
    assert {1, 2, 16} <= {nu for _, nu, _, _ in K.SWEEP}
    assert {1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 192, 193, 240, 241, 255, 256} <= hidden
    assert {48, 80, 112} <= hidden                                           # the next layer's unragged `in`, odd blocks
    assert {-(-h // 16) % 4 for h in hidden} == {0, 1, 2, 3}                  # the waves' tile counts differ, or not
    assert {(-(-h // 16) - w + 3) // 4 for h in hidden for w in range(min(4, -(-h // 16)))} == {1, 2, 3, 4}   # km_layer<NT>
    assert {len(hs) for _, _, hs, _ in K.SWEEP} == {1, 2, 3, 4}
    assert {a for *_, a in K.SWEEP} == {"relu", "tanh", "sigmoid", "selu"}
    for act in ("relu", "tanh", "sigmoid", "selu"):                          # the error buffer: (n_layers - 1) & 1
        assert {len(hs) & 1 for _, _, hs, a in K.SWEEP if a == act} == {0, 1}, act
    # both exits of the two-block pipeline, in the first layer and behind a hidden one
    assert {-(-i // 16) & 1 for i in ins} == {0, 1} and {-(-h // 16) & 1 for h in hidden} == {0, 1}
    assert [K.SWEEP[i][:2] for i in K.BATCHES["64x16"][0]] == [(64, 16)] * 3
    assert K.SWEEP[K.BATCHES["16x16"][0][0]][:2] == (16, 16) and all(K.EXTRA[j][0] == 3 for j in K.BATCHES["16x16"][1])


def _held(what, S, D, ref):
    """Device sums against the long-double reference: every figure printed, then held to the bound."""
    S_ref, D_ref, cond = ref
    tol = K.bound(cond)
    dS, dD = K.deviation(S, S_ref), K.deviation(D, D_ref)
    print("kstep mlp %s: S %.2e D %.2e from the long-double reference; cond %.2e, bound %.2e" % (what, dS, dD, cond, tol))
    assert np.all(np.isfinite(S)) and np.all(np.isfinite(D))
    assert dS <= tol and dD <= tol, (what, dS, dD, tol)


@pytest.mark.parametrize("case", range(len(K.SWEEP)))
def test_shape_sweep_against_the_long_double_reference(case):
    m = K.sweep_model(case)
    S, D = MM.kstep_sums_mlp([m], list(K.sweep_data(case)), K.SWEEP_KMAX, delta=True)
    assert m._handle is None
    _held("sweep %d %r" % (case, K.SWEEP[case]), S[0], D[0], K.sweep_reference(case))


# 9 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.EDGE_MODELS)
def test_row_and_horizon_edges_against_the_long_double_reference(case):
    m = K.sweep_model(case)
    for lens, kmax in K.EDGE_DATA:
        trajs = list(K.sweep_data(case, lens))
        assert MM.row_counts(trajs, 1)[0] == sum(L - 1 for L in lens)
        S, D = MM.kstep_sums_mlp([m], trajs, kmax, delta=True)
        _held("sweep %d on lengths %r, kmax %d" % (case, lens, kmax), S[0], D[0], K.sweep_reference(case, lens, kmax))
        S0, none = MM.kstep_sums_mlp([m], trajs, kmax)                      # without the delta sums: the same S
        assert none is None and np.array_equal(S0, S)


def test_rows_past_their_horizon_are_selected_away_not_multiplied_by_zero():
    """A two-row trajectory at 1e149: its start point counts at horizon 1 only, with a squared error of 1.4e299; the
    kernel rolls it on with clamped indices and its error leaves f64 from step 5 on (test_kstep_mlp_host.py asserts
    both on an f64 emulation).  0 x inf would make every later sum NaN; the reference never forms those values.

    The model is a synthetic one, not a sweep model: the relu sweep case's shape and weights with its dy_std widened
    by 8192 (kstep_mlp_cases.select_case).  The sweep's models change a state by a few percent per step, so scaling the
    observations alone, whatever the scale, overflows nothing within six steps."""
    p, act, trajs, scale = K.select_case()
    nx, nu, hidden, _ = K.SWEEP[K.SELECT_CASE]
    m = mlp_of(trajs[0].system, p, hidden, act)
    ref = K.reference(p, act, list(trajs), K.SWEEP_KMAX)
    with np.errstate(all="ignore"):
        S, D = MM.kstep_sums_mlp([m], list(trajs), K.SWEEP_KMAX, delta=True)
    print("kstep mlp select: scale %g, S %s, D %s" % (scale, S[0], D[0]))
    assert np.all(np.isfinite(S)) and np.all(np.isfinite(D)) and S[0, 0] > 1e298
    _held("select, horizons 2..", S[0, 1:], D[0, 1:], (ref[0][1:], ref[1][1:], ref[2]))
    _held("select, horizon 1", S[0, :1], D[0, :1], (ref[0][:1], ref[1][:1], ref[2]))


# 10 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(K.BATCHES))
def test_batches_at_the_new_shapes_are_the_same_bits_alone_in_any_order_and_again(name):
    import itertools
    cases, extras = K.BATCHES[name]
    models = [K.sweep_model(i) for i in cases] + [K.extra_model(j) for j in extras]
    trajs = list(K.sweep_data(cases[0]))
    assert len(models) == 3 and len({MM.device_shape_key(m) for m in models}) == 3
    S1, D1 = MM.kstep_sums_mlp(models, trajs, K.SWEEP_KMAX, delta=True)
    S2, D2 = MM.kstep_sums_mlp(models, trajs, K.SWEEP_KMAX, delta=True)
    assert np.array_equal(S1, S2) and np.array_equal(D1, D2)                # run to run
    assert np.all(np.isfinite(S1)) and np.all(np.isfinite(D1)) and np.all(S1 > 0) and np.all(D1 > 0)
    assert len({S1[i, 3] for i in range(3)}) == 3
    for perm in itertools.permutations(range(3)):
        Sp, Dp = MM.kstep_sums_mlp([models[i] for i in perm], trajs, K.SWEEP_KMAX, delta=True)
        for pos, i in enumerate(perm):
            assert np.array_equal(Sp[pos], S1[i]) and np.array_equal(Dp[pos], D1[i]), perm     # any order
    for i, m in enumerate(models):
        S, D = MM.kstep_sums_mlp([m], trajs, K.SWEEP_KMAX, delta=True)
        assert np.array_equal(S[0], S1[i]) and np.array_equal(D[0], D1[i]), i                # one call of n = n calls
    # and the batch's first model and the extra ones are what the reference says, on this data
    _held("batch %s, model 0" % name, S1[0], D1[0], K.sweep_reference(cases[0]))
    for pos, j in enumerate(extras):
        _held("batch %s, extra model %d" % (name, j), S1[len(cases) + pos], D1[len(cases) + pos], K.extra_reference(j))
