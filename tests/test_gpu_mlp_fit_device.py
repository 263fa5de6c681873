"""The device MLP fit (``fit_mlps(..., fit="device")``, ``DeviceFit``, ampc_mlpfit_*; csrc/mlpfit_kernels.hpp) against
the reference's goldens, against ``fit_reference_style`` on the CPU across the kernels' tile edges, one mixed batch in
one call, determinism / continuation, the fall-back for models over the limits, through the evaluator and the tuner,
and its rate against the torch lockstep path.  ``-m gpu``.

Tolerances are those of the torch GPU path for the same comparisons (test_gpu_mlp_fit.py): weights 1e-9 against the
reference's trained net and against any CPU fit of <= 25 steps, predictions 1e-8, 1e-7 for the 150-step 2 x 256 fit.
Every comparison prints its measured maximum before it asserts.
"""
import time

import numpy as np
import pytest
import torch

from autompc_amd import MLP, _lib
from autompc_amd.sysid import mlp_fit as F
from autompc_amd.sysid.mlp import MLPFactory
from helpers import make_system
from test_mlp_fit import _case, _interleave
from test_gpu_mlp_fit import _halfcheetah_like_trajs, _torch_forward

pytestmark = pytest.mark.gpu

W_TOL, P_TOL, LONG_TOL = 1e-9, 1e-8, 1e-7


def _maxdiff(ours, ref):
    return max(float(np.max(np.abs(np.asarray(a) - np.asarray(b)))) for a, b in zip(ours, ref))


def _np(parts):
    ws, bs = parts
    return _interleave([w.detach().cpu().numpy() for w in ws], [b.detach().cpu().numpy() for b in bs])


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["p_tanh", "hc_relu3", "p_selu1", "p_sig4"])
def test_device_train_reproduces_the_references_trained_net(tag):
    g, system, trajs, hidden, _, final = _case(tag)
    act = str(g["activation"])
    kw = {"hidden_size_%d" % (i + 1): h for i, h in enumerate(hidden)}
    m = MLP(system, n_hidden_layers=len(hidden), nonlintype=act, n_train_iters=int(g["n_train_iters"]),
            n_batch=int(g["n_batch"]), lr=float(g["lr"]), seed=int(g["seed"]), **kw)
    m.train(trajs, fit="device")
    dp = m._dev_params
    assert dp is not None and dp["w"][0].is_cuda and m._weights is None      # parameters stayed on the device
    pred = m.pred_batch(g["states"], g["ctrls_q"])                          # staged through ampc_set_mlp_dev
    assert m._weights is None                                               # ... without a host copy
    want = _torch_forward(dp["w"], dp["b"], act, dp["norm_np"], g["states"], g["ctrls_q"])
    dw = _maxdiff(_interleave(m.weights, m.biases), final)
    print("%s: weights vs reference %.3e, predictions vs reference %.3e, vs torch forward %.3e"
          % (tag, dw, np.max(np.abs(pred - g["pred"])), np.max(np.abs(pred - want))))
    np.testing.assert_allclose(pred, want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(pred, g["pred"], rtol=0, atol=P_TOL)
    assert dw <= W_TOL


# 2 ---------------------------------------------------------------------------------------------------------------
# (layer widths, activation, n_batch, rows, lr, epochs): at most 6 optimiser steps each.  Hidden widths cover
# {15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256} (a hidden width is one layer's `out` and the next one's `in`), inputs
# 2 and 80, outputs 1 and 64, depths 1-4, the four activations, n_batch in {1, 15, 16, 17, 63, 64, 128}, ragged last
# batches of one row and of n_batch - 1 rows, learning rates 1e-2 and 1e-5.
SWEEP = [
    ([2, 15, 1], "relu", 1, 3, 1e-2, 2),
    ([2, 16, 17, 1], "tanh", 15, 31, 1e-2, 2),                  # 15 + 15 + 1
    ([80, 31, 64], "sigmoid", 16, 47, 1e-5, 2),                 # 16 + 16 + 15
    ([80, 32, 33, 63, 64], "selu", 17, 35, 1e-2, 2),            # 17 + 17 + 1; depth 3 at lr 1e-2
    ([5, 64, 65, 255, 256, 3], "relu", 63, 188, 1e-2, 2),       # 63 + 63 + 62; depth 4 at lr 1e-2
    ([23, 256, 255, 17], "tanh", 64, 129, 1e-5, 2),             # 64 + 64 + 1
    ([23, 65, 64, 63, 17], "sigmoid", 128, 257, 1e-2, 2),       # 128 + 128 + 1
    ([7, 33, 32, 31, 17, 4], "selu", 16, 48, 1e-2, 2),
    ([80, 256, 64], "relu", 128, 255, 1e-2, 3),                 # 128 + 127
    ([2, 255, 1], "selu", 64, 65, 1e-5, 3),                     # 64 + 1
    ([4, 17, 16, 15, 2], "relu", 1, 5, 1e-2, 1),
    ([6, 63, 3], "tanh", 17, 50, 1e-2, 2),                      # 17 + 17 + 16
    ([23, 256, 256, 17], "relu", 64, 192, 1e-2, 2),
    ([9, 15, 255, 5], "sigmoid", 15, 45, 1e-5, 2),
    ([12, 16, 256, 33, 8], "tanh", 63, 64, 1e-2, 3),            # 63 + 1
    ([3, 64, 64, 2], "selu", 128, 128, 1e-2, 6),
    ([80, 65, 17, 64], "sigmoid", 16, 17, 1e-2, 3),             # 16 + 1
    ([2, 32, 31, 1], "relu", 17, 34, 1e-5, 3),
]


def test_the_sweep_covers_what_it_claims():
    hidden = {h for d, *_ in SWEEP for h in d[1:-1]}
    assert {15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256} <= hidden
    assert {d[0] for d, *_ in SWEEP} >= {2, 80} and {d[-1] for d, *_ in SWEEP} >= {1, 64}
    assert {len(d) - 2 for d, *_ in SWEEP} == {1, 2, 3, 4} and {a for _, a, *_ in SWEEP} == set(F.ACTS)
    assert {nb for _, _, nb, *_ in SWEEP} == {1, 15, 16, 17, 63, 64, 128}
    assert {lr for *_, lr, _ in SWEEP} == {1e-2, 1e-5}
    rag = {(nb, rows % nb) for _, _, nb, rows, _, _ in SWEEP if rows % nb}
    assert any(r == 1 and nb > 2 for nb, r in rag) and any(r == nb - 1 and nb > 2 for nb, r in rag)
    assert any(len(d) - 2 >= 3 and lr == 1e-2 for d, _, _, _, lr, _ in SWEEP)
    assert all(ep * -(-rows // nb) <= 6 for _, _, nb, rows, _, ep in SWEEP)


@pytest.mark.parametrize("case", range(len(SWEEP)))
def test_shape_edges_against_the_cpu_reference_style_fit(case):
    dims, act, nb, rows, lr, epochs = SWEEP[case]
    rng = np.random.default_rng(100 + case)
    feed = torch.from_numpy(rng.normal(size=(rows, dims[0])))
    target = torch.from_numpy(rng.normal(size=(rows, dims[-1])))
    seed, train_seed = 40 + case, 7 + case
    rw, rb = F.fit_reference_style(dims, act, feed, target, epochs, nb, lr, seed, train_seed=train_seed)
    fit = F.DeviceFit([dims], act, [lr], [seed], feed, target, nb, train_seeds=[train_seed])
    fit.run(epochs)
    assert fit.steps_done == epochs * -(-rows // nb) == fit._plan.steps
    d = _maxdiff(_np(fit.parameters(0)), _interleave([w.numpy() for w in rw], [b.numpy() for b in rb]))
    ws0, bs0 = F.initial_parameters(seed, dims)
    moved = _maxdiff(_np(fit.parameters(0)), _interleave([w.numpy() for w in ws0], [b.numpy() for b in bs0]))
    print("sweep %2d %-26s %-7s nb %3d rows %3d lr %g: departure %.3e (parameters moved %.3e)"
          % (case, dims, act, nb, rows, lr, d, moved))
    fit.close()
    assert moved > 0.5 * lr                      # Adam's first steps move a parameter by about lr each
    assert d <= W_TOL


# 3 ---------------------------------------------------------------------------------------------------------------
MIXED = [  # hidden sizes, activation, lr, init seed
    ([17], "relu", 1e-2, 1), ([64, 15], "tanh", 3e-3, 2), ([33, 16, 65], "sigmoid", 1e-2, 3),
    ([32, 31, 17, 63], "selu", 1e-3, 4), ([256], "tanh", 1e-5, 5), ([255, 256], "relu", 1e-2, 6),
    ([16, 16, 16], "selu", 3e-2, 7),
]


def _mixed_models(system, which=None):
    out = []
    for k, (hidden, act, lr, seed) in enumerate(MIXED):
        if which is not None and k != which:
            continue
        kw = {"hidden_size_%d" % (i + 1): h for i, h in enumerate(hidden)}
        out.append(MLP(system, n_hidden_layers=len(hidden), nonlintype=act, n_train_iters=2, n_batch=16, lr=lr,
                       seed=seed, **kw))
    return out


def test_one_mixed_batch_is_one_group_and_every_model_its_own_fit():
    system = make_system(3, 2)
    trajs = _halfcheetah_like_trajs(system, 3, 18, seed=5)              # 51 rows: 16 + 16 + 16 + 3 per epoch
    models = _mixed_models(system)
    info = F.fit_mlps(models, trajs, fit="device")
    assert info["groups"] == 1 and info["device_models"] == len(models) == 7 and info["torch_models"] == 0
    assert info["steps"] == 8
    XU, dY, xm, xs, dm, ds = F.training_arrays(trajs)
    feed, target = [torch.from_numpy(v) for v in F.normalised(XU, dY, xm, xs, dm, ds)]
    worst = 0.0
    for k, m in enumerate(models):
        alone = _mixed_models(system, k)[0]
        one = F.fit_mlps([alone], trajs, fit="device")
        assert one["groups"] == 1 and one["device_models"] == 1
        for a, b in zip(_interleave(m.weights, m.biases), _interleave(alone.weights, alone.biases)):
            np.testing.assert_array_equal(a, b)                          # a neighbour changes nothing
        hidden, act, lr, seed = MIXED[k]
        rw, rb = F.fit_reference_style([5] + hidden + [3], act, feed, target, 2, 16, lr, seed)
        d = _maxdiff(_interleave(m.weights, m.biases), _interleave([w.numpy() for w in rw], [b.numpy() for b in rb]))
        print("mixed %d %-20s %-7s lr %g: departure %.3e" % (k, hidden, act, lr, d))
        worst = max(worst, d)
    assert worst <= W_TOL


# 4 ---------------------------------------------------------------------------------------------------------------
def test_the_fit_is_deterministic_and_continues():
    rng = np.random.default_rng(3)
    feed, target = torch.from_numpy(rng.normal(size=(70, 6))), torch.from_numpy(rng.normal(size=(70, 2)))
    dims, acts = [[6, 33, 2], [6, 64, 17, 2], [6, 16, 255, 31, 2]], ["selu", "tanh", "relu"]
    args = (dims, acts, [1e-2, 1e-3, 3e-3], [1, 2, 3], feed, target, 32)

    def bits(*runs):
        fit = F.DeviceFit(*args, train_seeds=[100, 100, 9])
        for n in runs:
            fit.run(n)
        out = [p for k in range(3) for p in _np(fit.parameters(k))]
        fit.close()
        return out
    once, again, split = bits(3), bits(3), bits(2, 1)
    for a, b, c in zip(once, again, split):
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, c)


def test_the_plan_refuses_host_pointers_and_shapes_over_the_limits():
    feed, target, flat = np.zeros((8, 3)), np.zeros((8, 2)), np.zeros(200)
    lay = F.pack_device_models([[3, 16, 2]])
    with pytest.raises(_lib.AmpcError, match="device memory"):
        _lib.MlpFitPlan(lay["n_hidden"], lay["dims"], ["relu"], [1e-3], lay["offsets"], feed.ctypes.data,
                        target.ctypes.data, 8, 4, flat.ctypes.data, lay["n_params"])
    dfeed, dtarget, dflat = [torch.from_numpy(v).cuda() for v in (feed, target, flat)]
    dims = np.array([[3, 300, 2, 0, 0, 0]], dtype=np.int32)
    with pytest.raises(_lib.AmpcError, match="hidden widths"):
        _lib.MlpFitPlan([1], dims, ["relu"], [1e-3], [0], dfeed.data_ptr(), dtarget.data_ptr(), 8, 4,
                        dflat.data_ptr(), 2000)
    with pytest.raises(_lib.AmpcError, match="past the parameter buffer"):
        _lib.MlpFitPlan(lay["n_hidden"], lay["dims"], ["relu"], [1e-3], lay["offsets"], dfeed.data_ptr(),
                        dtarget.data_ptr(), 8, 4, dflat.data_ptr(), lay["n_params"] - 1)
    plan = _lib.MlpFitPlan(lay["n_hidden"], lay["dims"], ["relu"], [1e-3], lay["offsets"], dfeed.data_ptr(),
                           dtarget.data_ptr(), 8, 4, dflat.data_ptr(), lay["n_params"])
    with pytest.raises(_lib.AmpcError, match="device memory"):
        plan.run_epoch(np.zeros(8, dtype=np.int32).ctypes.data)
    assert plan.steps == 0
    plan.close()


# 5 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("odd", [dict(n_hidden_layers=5, hidden_size=16), dict(n_hidden_layers=1, hidden_size=300)])
def test_models_over_the_limits_fall_back_to_the_torch_path(odd):
    system = make_system(3, 2)
    trajs = _halfcheetah_like_trajs(system, 3, 18, seed=6)

    def build():
        common = dict(n_train_iters=2, n_batch=16, lr=3e-3)
        return [MLP(system, n_hidden_layers=2, hidden_size=24, nonlintype="tanh", seed=1, **common),
                MLP(system, nonlintype="relu", seed=2, **odd, **common),
                MLP(system, n_hidden_layers=3, hidden_size=17, nonlintype="selu", seed=3, **common)]
    models = build()
    info = F.fit_mlps(models, trajs, fit="device")
    assert info["device_models"] == 2 and info["torch_models"] == 1 and info["groups"] == 2
    for m, own in zip(models, build()):
        own.train(trajs)
        d = _maxdiff(_interleave(m.weights, m.biases), _interleave(own.weights, own.biases))
        print("fall-back %s: departure from its own train() %.3e" % (m.hidden_sizes, d))
        assert d <= W_TOL


# 6 ---------------------------------------------------------------------------------------------------------------
def _stack_setup():
    from autompc_amd.tuning import sample_pipeline_configs
    system = make_system(3, 2)
    trajs = _halfcheetah_like_trajs(system, 4, 60, seed=3)
    cfgs = sample_pipeline_configs(system, 10, np.random.default_rng(4), model_axis=True)
    for c in cfgs:                                       # cost gains that keep a 12-step episode finite
        for k in c:
            if k.startswith("_cost:"):
                c[k] = float(c[k] ** 0.25)
        c["_ctrlr:num_path"] = 128
    return system, trajs, cfgs


def test_holdout_evaluator_scores_with_the_device_fit():
    from autompc_amd.evaluation import HoldoutModelEvaluator
    from autompc_amd.tuning import DictConfiguration, candidate_from_config
    system, trajs, cfgs = _stack_setup()
    factory = MLPFactory(system, n_train_iters=2, n_batch=32)
    mcfgs = [DictConfiguration(candidate_from_config(system, c)["model_cfg"]) for c in cfgs]
    scores = {}
    for how in ("torch", "device"):
        ev = HoldoutModelEvaluator(system, trajs, "rmse", np.random.default_rng(2), horizon=3, holdout_prop=0.25,
                                   mlp_fit=how)
        scores[how] = np.asarray(ev.evaluate_batch(factory, mcfgs))
        assert ev.last_mlp_fit["device_models"] == (len(mcfgs) if how == "device" else 0)
        if how == "device":
            assert ev.last_mlp_fit["groups"] == 1
    rel = np.max(np.abs(scores["device"] - scores["torch"]) / np.abs(scores["torch"]))
    print("holdout scores: torch %s device %s, relative departure %.3e" % (scores["torch"], scores["device"], rel))
    np.testing.assert_allclose(scores["device"], scores["torch"], rtol=1e-7, atol=0)


def test_pipeline_tuner_model_axis_with_the_device_fit():
    from autompc_amd import QuadCost, Task
    from autompc_amd.tuning import BatchPipelineTuner, CandidateEvaluator
    system, trajs, cfgs = _stack_setup()
    surrogate = MLP(system, n_hidden_layers=2, hidden_size=32, nonlintype="tanh", n_train_iters=2, n_batch=32)
    surrogate.train(trajs)
    task = Task(system)
    task.set_cost(QuadCost(system, np.eye(3), 0.1 * np.eye(2), np.eye(3)))
    task.set_ctrl_bounds(-np.ones(2), np.ones(2))
    task.set_num_steps(12)
    task.set_init_obs(np.array([0.3, -0.2, 0.1]))
    factory = MLPFactory(system, n_train_iters=2, n_batch=32)
    ev = CandidateEvaluator(system, task, surrogate)
    costs = {}
    for how in ("torch", "device"):
        tuner = BatchPipelineTuner(system, ev, batch_size=5, model_factory=factory, trajs=trajs, mlp_fit=how)
        _, res = tuner.run(10, np.random.default_rng(0), seed=7, configs=cfgs)
        assert tuner.models_fitted == 10 and np.all(np.isfinite(res.costs))
        assert tuner.mlp_device_fits == (10 if how == "device" else 0)
        costs[how] = np.asarray(res.costs, dtype=float)
    rel = np.max(np.abs(costs["device"] - costs["torch"]) / np.maximum(1.0, np.abs(costs["torch"])))
    print("tuner costs: relative departure %.3e" % rel)
    assert rel <= 1e-7


# 7 ---------------------------------------------------------------------------------------------------------------
def test_eight_2x256_models_fit_faster_than_the_torch_lockstep_path():
    """K = 8, [23, 256, 256, 17], 3200 rows, batch 64: both paths warmed with one epoch, then two epochs timed.  The
    150-step device fit is also held to fit_reference_style on the GPU at 1e-7 (models 0 and 7)."""
    system = make_system(17, 6)
    trajs = _halfcheetah_like_trajs(system, 16, 201)
    XU, dY, xm, xs, dm, ds = F.training_arrays(trajs)
    feed, target = [torch.from_numpy(v).cuda() for v in F.normalised(XU, dY, xm, xs, dm, ds)]
    dims = [[23, 256, 256, 17]] * 8
    lrs = [1e-3 * (1 + k) for k in range(8)]
    seeds = list(range(20, 28))
    lock = F.LockstepFit(dims, "relu", lrs, seeds, feed, target, 64, device="cuda")
    lock.run(1)                                                     # (captures the chunk graphs)
    dfit = F.DeviceFit(dims, "relu", lrs, seeds, feed, target, 64)
    dfit.run(1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lock.run(2)
    torch.cuda.synchronize()
    t_lock = time.perf_counter() - t0
    t0 = time.perf_counter()
    dfit.run(2)
    torch.cuda.synchronize()
    t_dev = time.perf_counter() - t0
    print("two epochs (100 steps): torch lockstep %.4f s = %.1f us / step, device %.4f s = %.1f us / step: %.2fx"
          % (t_lock, 1e4 * t_lock, t_dev, 1e4 * t_dev, t_lock / t_dev))
    worst = 0.0
    for k in (0, 7):
        rw, rb = F.fit_reference_style(dims[k], "relu", feed, target, 3, 64, lrs[k], seeds[k], device="cuda")
        dw, db = dfit.parameters(k)
        worst = max(worst, max(float((a - b).abs().max()) for a, b in zip(dw + db, rw + rb)))
    print("150 steps: departure from fit_reference_style %.3e" % worst)
    dfit.close()
    assert worst < LONG_TOL
    assert t_dev < t_lock
