"""The host side of the device MLP fit (``fit_mlps(..., fit="device")``, ampc_mlpfit_*): option validation through the
stack, the pure-Python descriptor / offset packing, the routing of models over the kernels' limits, the loud failure
without a GPU, and the deep sigmoid golden (tests/golden/gen_golden_mlpfit_deep.py) held by the two torch fits.  No GPU
here."""
import numpy as np
import pytest
import torch

from autompc_amd import MLP, _lib
from autompc_amd.evaluation import HoldoutModelEvaluator
from autompc_amd.sysid import mlp_fit as F
from autompc_amd.sysid.mlp import MLPFactory
from helpers import make_system
from test_mlp_fit import TOL, _case, _interleave


def _trajs(system, n=3, rows=20, seed=0):
    from autompc_amd import zeros
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        t = zeros(system, rows)
        t.obs[:] = 0.1 * rng.normal(size=(rows, system.obs_dim)).cumsum(axis=0)
        t.ctrls[:] = rng.normal(size=(rows, system.ctrl_dim))
        out.append(t)
    return out


def test_fit_option_is_validated_everywhere_and_stored():
    system = make_system(3, 2)
    trajs = _trajs(system)
    m = MLP(system, n_hidden_layers=1, hidden_size=16, n_train_iters=1)
    with pytest.raises(ValueError, match="fit must be"):
        F.fit_mlps([m], trajs, fit="gpu")
    with pytest.raises(ValueError, match="fit must be"):
        m.train(trajs, fit="gpu")
    rng = np.random.default_rng(0)
    with pytest.raises(ValueError, match="mlp_fit must be"):
        HoldoutModelEvaluator(system, trajs, "rmse", rng, mlp_fit="gpu")
    ev = HoldoutModelEvaluator(system, trajs, "rmse", rng, mlp_fit="device")
    assert ev.mlp_fit == "device"
    assert HoldoutModelEvaluator(system, trajs, "rmse", rng).mlp_fit == "torch"
    from autompc_amd.tuning import BatchModelTuner, BatchPipelineTuner

    class _Ev:                                   # the tuner only stores its evaluator here
        accepts_global_ids = True
    with pytest.raises(ValueError, match="mlp_fit must be"):
        BatchPipelineTuner(system, _Ev(), mlp_fit="gpu")
    tuner = BatchPipelineTuner(system, _Ev(), model_factory=MLPFactory(system), trajs=trajs, mlp_fit="device")
    assert tuner.mlp_fit == "device" and tuner.mlp_device_fits == 0
    assert BatchPipelineTuner(system, _Ev()).mlp_fit == "torch"
    assert BatchModelTuner is not None           # (follows its evaluator's option: nothing of its own to validate)


def test_descriptor_packing_of_a_mixed_batch():
    dims_list = [[5, 17, 3], [5, 64, 15, 33, 16, 3], [5, 256, 256, 3], [5, 31, 3]]
    lay = F.pack_device_models(dims_list)
    assert list(lay["n_hidden"]) == [1, 4, 2, 1] and lay["dims"].shape == (4, 6) and lay["dims"].dtype == np.int32
    np.testing.assert_array_equal(lay["dims"][0], [5, 17, 3, 0, 0, 0])
    np.testing.assert_array_equal(lay["dims"][1], [5, 64, 15, 33, 16, 3])
    # every double of the flat buffer belongs to exactly one array of one model
    owner = np.zeros(lay["n_params"], dtype=np.int64)
    for k, (d, layers) in enumerate(zip(dims_list, lay["layers"])):
        assert lay["offsets"][k] == layers[0][0] and len(layers) == len(d) - 1
        for l, (w, b, fo, fi) in enumerate(layers):
            assert (fo, fi) == (d[l + 1], d[l]) and b == w + fo * fi             # the bias follows its weight
            owner[w:w + fo * fi] += 1
            owner[b:b + fo] += 1
    np.testing.assert_array_equal(owner, 1)
    assert lay["n_params"] == sum(o * i + o for d in dims_list for i, o in zip(d[:-1], d[1:]))
    # the per-layer views alias the flat buffer and have torch.nn.Linear's shapes
    flat = torch.arange(lay["n_params"], dtype=torch.float64)
    for k, d in enumerate(dims_list):
        ws, bs = F.layer_views(flat, lay["layers"][k])
        assert [tuple(w.shape) for w in ws] == [(o, i) for i, o in zip(d[:-1], d[1:])]
        assert [tuple(b.shape) for b in bs] == [(o,) for o in d[1:]]
        assert all(w.is_contiguous() and w.data_ptr() == flat.data_ptr() + 8 * lw[0]
                   for w, lw in zip(ws, lay["layers"][k]))
        assert float(ws[0][0, 0]) == float(lay["offsets"][k])
    with pytest.raises(ValueError):
        F.pack_device_models([[5, 3]])
    with pytest.raises(ValueError):
        F.pack_device_models([[5, 8, 8, 8, 8, 8, 3]])


def test_models_over_the_limits_are_routed_to_the_torch_list():
    ok = [([80, 256, 64], 128), ([2, 15, 16, 17, 255, 1], 1), ([23, 256, 256, 17], 4096)]
    over = [([23, 300, 17], 64), ([23, 16, 16, 16, 16, 16, 17], 64), ([81, 16, 64], 64), ([80, 16, 65], 64),
            ([23, 256, 17], 4097), ([23, 17], 64)]
    assert all(F.device_fit_supports(d, nb) for d, nb in ok)
    assert not any(F.device_fit_supports(d, nb) for d, nb in over)
    assert (F.DEVICE_MAX_HIDDEN, F.DEVICE_MAX_WIDTH, F.DEVICE_MAX_IN, F.DEVICE_MAX_OUT) == (
        _lib.MlpFitPlan.MAX_HIDDEN, _lib.MlpFitPlan.MAX_WIDTH, _lib.MlpFitPlan.MAX_IN, _lib.MlpFitPlan.MAX_OUT)
    assert F.DEVICE_MAX_BATCH == _lib.MlpFitPlan.MAX_BATCH >= 128


def test_the_plan_symbols_are_bound():
    for name in ("ampc_mlpfit_create", "ampc_mlpfit_run_epoch", "ampc_mlpfit_destroy"):
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["ampc_mlpfit_create"][1]) == 15


def test_device_fit_without_a_gpu_raises_instead_of_training_on_the_cpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)       # (a no-op on a machine without one)
    system = make_system(3, 2)
    trajs = _trajs(system)
    m = MLP(system, n_hidden_layers=1, hidden_size=16, n_train_iters=1)
    before = [w.copy() for w in m.weights]
    with pytest.raises(_lib.AmpcError, match="needs a usable GPU"):
        m.train(trajs, fit="device")
    with pytest.raises(_lib.AmpcError, match="needs a usable GPU"):
        F.fit_mlps([m], trajs, fit="device")
    XU, dY, xm, xs, dm, ds = F.training_arrays(trajs)
    feed, target = [torch.from_numpy(v) for v in F.normalised(XU, dY, xm, xs, dm, ds)]
    with pytest.raises(_lib.AmpcError, match="needs a usable GPU"):
        F.DeviceFit([[5, 16, 3]], "relu", [1e-3], [1], feed, target, 8)
    assert m._dev_params is None and all(np.array_equal(a, b) for a, b in zip(m.weights, before))   # untouched


def test_the_torch_result_reports_where_the_models_were_fitted():
    system = make_system(3, 2)
    trajs = _trajs(system)
    ms = [MLP(system, n_hidden_layers=1, hidden_size=16, n_train_iters=1, n_batch=16, seed=s) for s in (1, 2)]
    info = F.fit_mlps(ms, trajs, device="cpu")
    assert info["groups"] == 1 and info["device_models"] == 0 and info["torch_models"] == 2


def test_reference_style_and_lockstep_fits_reproduce_the_deep_sigmoid_golden():
    """Four sigmoid hidden layers [17, 64, 15, 33], n_batch 16, 81 rows: a ragged last batch of ONE row."""
    g, system, trajs, hidden, init, final = _case("p_sig4")
    assert hidden == [17, 64, 15, 33] and str(g["activation"]) == "sigmoid" and int(g["n_batch"]) == 16
    dims = [system.obs_dim + system.ctrl_dim] + hidden + [system.obs_dim]
    XU, dY, xm, xs, dm, ds = F.training_arrays(trajs)
    assert XU.shape[0] % 16 == 1
    feed, target = [torch.from_numpy(v) for v in F.normalised(XU, dY, xm, xs, dm, ds)]
    lr, seed, n_iter = float(g["lr"]), int(g["seed"]), int(g["n_train_iters"])
    ws, bs = F.initial_parameters(seed, dims)
    for a, b in zip(_interleave([w.numpy() for w in ws], [b.numpy() for b in bs]), init):
        np.testing.assert_array_equal(a, b)
    rw, rb = F.fit_reference_style(dims, "sigmoid", feed, target, n_iter, 16, lr, seed)
    for a, b in zip(_interleave([w.numpy() for w in rw], [b.numpy() for b in rb]), final):
        np.testing.assert_allclose(a, b, rtol=0, atol=TOL)
    fit = F.LockstepFit([dims], "sigmoid", [lr], [seed], feed, target, 16, device="cpu")
    fit.run(n_iter)
    lw, lb = fit.parameters(0)
    for a, b in zip(_interleave([w.numpy() for w in lw], [b.numpy() for b in lb]), final):
        np.testing.assert_allclose(a, b, rtol=0, atol=TOL)
    assert fit.steps_done == 18
